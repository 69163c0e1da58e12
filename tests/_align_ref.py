"""numpy restatement of the alignment of a reference (include/psgsdf_align.h, DESIGN.md "Alignment of a reference"): float64 throughout, every row
operation for operation as the header states it, the correspondences by tests/_compare_ref.py's exhaustive nearest (`search=cref.nearest`, the
default) or by `pruned_nearest`, which evaluates the same pair function on a superset of the targets within the radius and therefore returns the
same matches (tests/test_align_cpu.py checks that it does).  It is the yardstick of tests/test_align_cpu.py and tests/test_align_gpu.py.

    move(M, pts)                      -> float32 points under the 3x4 transform M
    inverse(T)                        -> [R^T | -R^T t]
    rows(...)                         -> J [m, 6], rho [m] of one direction at T, and what they were formed from
    system(J, rho)                    -> the 28 sums (A's upper triangle row-major, g, e), the same sums of the terms' magnitudes, n
    solve(sys)                        -> (degenerate, min_pivot, xi)
    exp_so3(omega), compose(T, omega, v, c)
    align(...)                        -> dict like capi.Api.align_reference's
"""
import numpy as np

import _compare_ref as cref

f32, f64 = np.float32, np.float64
CONVERGED, MAX_ITERS, DEGENERATE, TOO_FEW = 0, 1, 2, 3
PIVOT_MIN = 1e-6
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def apply(M, P):
    """the 3x4 transform M on float64 points, unrounded"""
    M = np.asarray(M, f64)
    return np.stack([((M[k, 0] * P[:, 0] + M[k, 1] * P[:, 1]) + M[k, 2] * P[:, 2]) + M[k, 3] for k in range(3)], 1)


def move(M, pts):
    with np.errstate(invalid="ignore", over="ignore"):
        return apply(M, np.asarray(pts, f32).reshape(-1, 3).astype(f64)).astype(f32)


def inverse(T):
    T = np.asarray(T, f64)
    Ti = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            Ti[i, j] = T[j, i]
        Ti[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return Ti


def bbox_centre(xyz):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(1)
    if not ok.any():
        return np.zeros(3)
    X = xyz[ok].astype(f64)
    return (X.min(0) + X.max(0)) / 2.0


def pruned_nearest(queries, xyz, faces, max_dist):
    """cref.nearest's matches from the targets whose centroid lies within max_dist + the largest centroid-to-corner distance of the query (a
    superset of the targets within max_dist), by scipy's k-d tree; without scipy the exhaustive search itself"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return cref.nearest(queries, xyz, faces, max_dist)
    P = np.asarray(queries, f32).reshape(-1, 3).astype(f64)
    a, b, c, tri = cref.corners(xyz, faces)
    n = len(P)
    valid = np.isfinite(P).all(1)
    best = np.full(n, np.inf); idx = np.full(n, -1, np.int64)
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    if fin.any() and valid.any():
        t = np.nonzero(fin)[0]
        cen = (a[t] + b[t] + c[t]) / 3.0
        reach = max(float(np.linalg.norm(x[t] - cen, axis=1).max()) for x in (a, b, c))
        vq = np.nonzero(valid)[0]
        lists = cKDTree(cen).query_ball_point(P[vq], max_dist * (1 + 1e-9) + reach * (1 + 1e-9) + 1e-12)
        cnt = np.array([len(l) for l in lists])
        if cnt.sum():
            qi = np.repeat(vq, cnt); tj = t[np.concatenate([np.asarray(l, np.int64) for l in lists if len(l)])]
            D2, _, _ = cref.pair(P[qi], a[tj], b[tj], c[tj])
            D2 = np.where(np.isfinite(D2), D2, np.inf)
            order = np.lexsort((tj, D2, qi))                # per query: the smallest D2, ties to the smaller index
            first = order[np.r_[True, qi[order][1:] != qi[order][:-1]]]
            best[qi[first]] = D2[first]; idx[qi[first]] = tj[first]
    with np.errstate(invalid="ignore"):
        d = np.sqrt(best)
    matched = valid & np.isfinite(best) & (d <= max_dist)
    dd = np.where(valid, np.where(matched, d, np.inf), np.nan)
    return dict(d=dd, dist=dd.astype(f32), nearest=np.where(matched, idx, -1).astype(np.int32), valid=valid, matched=matched)


def rows(direction, T, mesh_xyz, mesh_nrm, mesh_faces, ref_xyz, ref_faces, radius, c, vs, search=cref.nearest):
    """the rows of one direction at the 3x4 transform T: dict of J [m, 6], rho [m], query (their queries' indices), target, moved (all the
    direction's queries as float32)"""
    vs = float(f32(vs))
    mesh_xyz = np.asarray(mesh_xyz, f32).reshape(-1, 3); ref_xyz = np.asarray(ref_xyz, f32).reshape(-1, 3)
    empty = dict(J=np.zeros((0, 6)), rho=np.zeros(0), query=np.zeros(0, np.int64), target=np.zeros(0, np.int64))
    with np.errstate(all="ignore"):
        if direction == 1:
            moved = move(T, ref_xyz)
            if len(moved) == 0 or mesh_faces is None or len(mesh_faces) == 0:
                return dict(empty, moved=moved)
            r = search(moved, mesh_xyz, mesh_faces, radius)
            m = np.nonzero(r["matched"])[0]; j = r["nearest"][m].astype(np.int64)
            a, b, cc, _ = cref.corners(mesh_xyz, mesh_faces)
            x = moved[m].astype(f64)
            _, q, _ = cref.pair(x, a[j], b[j], cc[j])
            nn = cross(b[j] - a[j], cc[j] - a[j])
            d = x - q
        else:
            moved = move(inverse(T), mesh_xyz)
            if len(moved) == 0 or len(ref_xyz) == 0:
                return dict(empty, moved=moved)
            r = search(moved, ref_xyz, ref_faces, radius)
            m = np.nonzero(r["matched"])[0]; j = r["nearest"][m].astype(np.int64)
            a, b, cc, _ = cref.corners(ref_xyz, ref_faces)
            _, q, _ = cref.pair(moved[m].astype(f64), a[j], b[j], cc[j])
            x = apply(T, q)
            nn = np.asarray(mesh_nrm, f32).reshape(-1, 3)[m].astype(f64)
            d = x - mesh_xyz[m].astype(f64)
        n = nn / np.sqrt(dot(nn, nn))[:, None]
        keep = np.isfinite(n).all(1)
        n, x, d, m, j = n[keep], x[keep], d[keep], m[keep], j[keep]
        rho = dot(n, d) / vs
        y = (x - np.asarray(c, f64)) / vs
        J = np.concatenate([cross(y, n), n], 1)
    return dict(J=J, rho=rho, query=m, target=j, moved=moved)


def system(J, rho):
    """(sys [28], the same sums over the terms' magnitudes [28], n)"""
    terms = [J[:, i] * J[:, j] for i, j in UPPER] + [J[:, i] * rho for i in range(6)] + [rho * rho]
    return np.array([t.sum() for t in terms], f64), np.array([np.abs(t).sum() for t in terms], f64), len(rho)


def solve(sys):
    """the step of the header: (degenerate, min_pivot, xi)"""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(UPPER):
        A[i, j] = A[j, i] = sys[k]
    g = np.asarray(sys[21:27], f64)
    if not (np.diag(A) > 0).all():
        return True, 0.0, np.zeros(6)
    s = np.sqrt(np.diag(A))
    S = A / (s[:, None] * s[None, :])
    L = np.zeros((6, 6)); mp = np.inf
    for j in range(6):
        d = S[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not d >= mp:
            mp = d
        if not d > PIVOT_MIN:
            return True, float(mp), np.zeros(6)
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            v = S[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    b = -(g / s)
    z = np.zeros(6); w = np.zeros(6)
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i, k] * z[k]
        z[i] = v / L[i, i]
    for i in range(5, -1, -1):
        v = z[i]
        for k in range(i + 1, 6):
            v = v - L[k, i] * w[k]
        w[i] = v / L[i, i]
    return False, float(mp), w / s


def exp_so3(om):
    om = np.asarray(om, f64)
    th2 = float(dot(om, om)); th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    return (np.eye(3) + a * K) + b * (np.outer(om, om) - th2 * np.eye(3))


def delta(om, v, c):
    """Delta(x) = c + Exp(omega)(x - c) + v as a 3x4"""
    E = exp_so3(om); c = np.asarray(c, f64)
    return np.concatenate([E, ((c - np.array([dot(E[i], c) for i in range(3)])) + np.asarray(v, f64))[:, None]], 1)


def compose(T, om, v, c):
    """Delta o T"""
    T = np.asarray(T, f64); E = exp_so3(om); c = np.asarray(c, f64)
    N = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            N[i, j] = (E[i, 0] * T[0, j] + E[i, 1] * T[1, j]) + E[i, 2] * T[2, j]
        N[i, 3] = dot(E[i], T[:, 3]) + ((c[i] - dot(E[i], c)) + v[i])
    return N


def evaluate(T, mesh, ref, radius, c, vs, directions, search=cref.nearest):
    mesh_xyz, mesh_nrm, mesh_faces = mesh; ref_xyz, ref_faces = ref
    parts = [rows(d, T, mesh_xyz, mesh_nrm, mesh_faces, ref_xyz, ref_faces, radius, c, vs, search) if directions & d else None for d in (1, 2)]
    J = np.concatenate([p["J"] for p in parts if p is not None]); rho = np.concatenate([p["rho"] for p in parts if p is not None])
    sys, mag, n = system(J, rho)
    vsd = float(f32(vs))
    it = dict(radius=float(radius), rms=vsd * float(np.sqrt(sys[27] / n)) if n else 0.0, n_pairs=[len(p["rho"]) if p is not None else 0 for p in parts], min_pivot=0.0, step=np.zeros(6))
    return sys, mag, n, it, parts


def align(mesh_xyz, mesh_nrm, mesh_faces, ref_xyz, ref_faces, vs, init=None, max_dist=None, min_dist=None, shrink=1.0, directions=3, max_iters=30, eps_rot=1e-5, eps_trans=None,
          search=cref.nearest):
    vsd = float(f32(vs))
    max_dist = 8 * vsd if max_dist is None else max_dist; min_dist = vsd if min_dist is None else min_dist; eps_trans = 1e-3 * vsd if eps_trans is None else eps_trans
    T4 = np.eye(4) if init is None else np.asarray(init, f64).reshape(4, 4)
    T = T4[:3].copy()
    mesh = (np.asarray(mesh_xyz, f32).reshape(-1, 3), mesh_nrm, mesh_faces); ref = (np.asarray(ref_xyz, f32).reshape(-1, 3), ref_faces)
    c = bbox_centre(mesh[0])
    out = dict(centre=c, status=MAX_ITERS, n_iters=0, iters=[])
    last = max_iters == 0
    pw = 1.0
    k = 0
    while True:
        radius = max(min_dist, max_dist * pw)
        sys, mag, n, it, parts = evaluate(T, mesh, ref, radius, c, vsd, directions, search)
        if k == 0:
            out["system0"], out["system0_abs"], out["n0"] = sys, mag, n
        out["final"] = dict(it)
        if last:
            if out["n_iters"] == 0 and n < 6:
                out["status"] = TOO_FEW
            break
        if n < 6:
            out["status"] = TOO_FEW; out["iters"].append(it); break
        deg, mp, xi = solve(sys)
        it["min_pivot"] = mp
        if deg:
            out["status"] = DEGENERATE; out["iters"].append(it); break
        v = xi[3:] * vsd
        it["step"] = np.concatenate([xi[:3], v])
        out["iters"].append(it); out["n_iters"] = k + 1
        T = compose(T, xi[:3], v, c)
        conv = np.sqrt(dot(xi[:3], xi[:3])) <= eps_rot and np.sqrt(dot(v, v)) <= eps_trans
        if conv:
            out["status"] = CONVERGED
        last = conv or k + 1 == max_iters
        pw *= shrink
        k += 1
    out["transform"] = np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]])
    out["aligned_xyz"] = move(T, ref[0])
    return out


def rigid(axis, degrees, translation, through):
    """the 4x4 rotation by `degrees` about `axis` through the point `through`, followed by `translation`"""
    axis = np.asarray(axis, f64); om = axis / np.linalg.norm(axis) * np.deg2rad(degrees)
    M = np.eye(4); M[:3] = delta(om, np.asarray(translation, f64), np.asarray(through, f64))
    return M


def rigid_inverse(M):
    N = np.eye(4); N[:3] = inverse(M[:3])
    return N
