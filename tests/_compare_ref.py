"""numpy restatement of the comparison with a reference (include/psgsdf_compare.h, DESIGN.md "Comparison with a reference"): float64 throughout,
the pair function vectorised over pairs with np.where in the stated test order, the nearest target by an exhaustive minimum over ALL targets (no
grid), in chunks of at most CHUNK pairs.  It is the yardstick of tests/test_compare_cpu.py and tests/test_compare_gpu.py.

    pair(p, a, b, c)                        -> (D2, q, region) of pairs [m, 3] each
    nearest(queries, xyz, faces, max_dist)  -> dict of d (float64: NaN invalid, inf unmatched), dist, nearest, side
    side_stats(r, vs, max_dist, tau)        -> the integers and doubles of psgsdf_compare_side
    compare(mesh_xyz, mesh_faces, ref_xyz, ref_faces, vs, max_dist, tau) -> both directions and the scores
"""
import numpy as np

f32, f64 = np.float32, np.float64
CHUNK = 4_000_000                     # pairs of one exhaustive call
REGIONS = ("vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "interior")
UNIT = 1048576.0                      # 2^20


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def pair(p, a, b, c):
    """Ericson 5.1.5 with the header's rules; p, a, b, c broadcast to [..., 3] float64.  Returns (D2, q, region index into REGIONS)."""
    p, a, b, c = (np.asarray(x, f64) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
        denom = 1.0 / ((va + vb) + vc)
        qs = [a + 0 * p, b + 0 * p, a + ab * (d1 / (d1 - d3))[..., None], c + 0 * p, a + ac * (d2 / (d2 - d6))[..., None],
              b + (c - b) * (e1 / (e1 + e2))[..., None], (a + ab * (vb * denom)[..., None]) + ac * (vc * denom)[..., None]]
        shape = np.broadcast(d1, d1).shape
        region = np.full(shape, 6, np.int64)
        q = np.broadcast_to(qs[6], shape + (3,)).copy()
        for k in range(5, -1, -1):      # the first test that holds decides: apply them last to first
            m = np.broadcast_to(conds[k], shape)
            region = np.where(m, k, region)
            q = np.where(m[..., None], np.broadcast_to(qs[k], shape + (3,)), q)
        pq = p - q
        return dot(pq, pq), q, region


def corners(xyz, faces):
    """the targets' corners a, b, c [t, 3] float64: triangles, or (faces None or empty) the points as degenerate triangles"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3).astype(f64)
    if faces is None or len(faces) == 0:
        return xyz, xyz, xyz, False
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]], True


def nearest(queries, xyz, faces, max_dist):
    """every query against every target: the smallest finite D2, ties to the smaller index"""
    P = np.asarray(queries, f32).reshape(-1, 3).astype(f64)
    a, b, c, tri = corners(xyz, faces)
    n, t = len(P), len(a)
    valid = np.isfinite(P).all(1)
    best = np.full(n, np.inf); idx = np.full(n, -1, np.int64)
    if t:
        rows = max(1, CHUNK // t)
        for s in range(0, n, rows):
            e = min(n, s + rows)
            D2, _, _ = pair(P[s:e, None, :], a[None], b[None], c[None])
            D2 = np.where(np.isfinite(D2), D2, np.inf)
            j = np.argmin(D2, axis=1)                      # (the first of equal minima: the smaller index)
            best[s:e] = D2[np.arange(e - s), j]; idx[s:e] = j
    with np.errstate(invalid="ignore"):
        d = np.sqrt(best)
    matched = valid & np.isfinite(best) & (d <= max_dist)
    side = np.zeros(n, np.int8)
    if tri and matched.any():
        m = np.nonzero(matched)[0]; j = idx[m]
        _, q, _ = pair(P[m], a[j], b[j], c[j])
        ab, ac, pq = b[j] - a[j], c[j] - a[j], P[m] - q
        nrm = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        side[m] = np.sign(dot(pq, nrm)).astype(np.int8)
    dd = np.where(valid, np.where(matched, d, np.inf), np.nan)
    return dict(d=dd, d_all=np.where(valid, d, np.nan), dist=dd.astype(f32), nearest=np.where(matched, idx, -1).astype(np.int32), side=side, valid=valid, matched=matched)


def hist_bin(d, max_dist):
    return np.minimum(15, (16.0 * d / max_dist).astype(np.int64))


def side_stats(r, vs, max_dist, tau):
    vs = float(f32(vs))
    m = r["matched"]
    d = r["d"][m]
    u = d / vs
    f = np.rint(u * UNIT).astype(np.int64)
    s = dict(n=len(r["d"]), n_valid=int(r["valid"].sum()), n_matched=int(m.sum()), n_within_tau=int((d <= tau).sum()),
             sum_d=int(f.sum()), sum_d2=int(np.rint(u * u * UNIT).astype(np.int64).sum()), sum_signed=int((r["side"][m].astype(np.int64) * f).sum()),
             hist=np.bincount(hist_bin(d, max_dist), minlength=16).astype(np.int64), max=float(d.max()) if len(d) else 0.0, mean=0.0, rms=0.0, mean_signed=0.0)
    if s["n_matched"]:
        k = float(s["n_matched"])
        s["mean"] = vs * (float(s["sum_d"]) / UNIT) / k
        s["rms"] = vs * float(np.sqrt((float(s["sum_d2"]) / UNIT) / k))
        s["mean_signed"] = vs * (float(s["sum_signed"]) / UNIT) / k
    return s


def scores(to_ref, to_rec):
    P = to_ref["n_within_tau"] / to_ref["n_valid"] if to_ref["n_valid"] else 0.0
    R = to_rec["n_within_tau"] / to_rec["n_valid"] if to_rec["n_valid"] else 0.0
    return P, R, (2.0 * P * R / (P + R) if P + R > 0 else 0.0)


def check_params(vs, max_dist, tau, grid_cell=0.0, reserved=(0, 0)):
    vs = float(f32(vs))
    if not (np.isfinite(max_dist) and 0 < max_dist <= 64 * vs and np.isfinite(tau) and 0 < tau <= max_dist and np.isfinite(grid_cell) and grid_cell >= 0 and not any(reserved)):
        raise ValueError((max_dist, tau, grid_cell, reserved))


def compare(mesh_xyz, mesh_faces, ref_xyz, ref_faces, vs, max_dist, tau):
    check_params(vs, max_dist, tau)
    v = nearest(mesh_xyz, ref_xyz, ref_faces, max_dist)
    r = nearest(ref_xyz, mesh_xyz, mesh_faces, max_dist) if len(mesh_faces) else nearest(ref_xyz, np.zeros((0, 3), f32), None, max_dist)
    sv, sr = side_stats(v, vs, max_dist, tau), side_stats(r, vs, max_dist, tau)
    P, R, F = scores(sv, sr)
    return dict(vertex=v, ref=r, to_reference=sv, to_reconstruction=sr, precision=P, recall=R, fscore=F)


def fibonacci(n, centre, radius):
    """n points on a sphere (the golden-angle spiral), float32"""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = np.pi * (1 + 5 ** 0.5) * i
    s = np.sqrt(1 - z * z)
    return (np.asarray(centre, f64) + radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(f32)


def icosphere(centre, radius, subdivisions=2):
    """an icosphere (20 4^subdivisions faces, outward winding) as (xyz float32, faces int32)"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, f64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []
        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                w = v[i] + v[j]; v.append(w / np.linalg.norm(w)); mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(centre, f64) + radius * np.array(v)).astype(f32), np.array(f, np.int32)
