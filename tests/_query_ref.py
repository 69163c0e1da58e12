"""Yardstick of the field queries (include/psgsdf_query.h, DESIGN.md 22 "Field queries"), in numpy float64, written from the definitions: the two
models, the projection loop and the rays, whose walk is tests/_bake_ref.py walk() as tests/_occlusion_ref.py uses it (float64, no brick map, no cut).
Shared by tests/test_query_cpu.py and tests/test_query_gpu.py.

    query_points(v, dim, vs, xyz, model)                          -> dict of status, dist, normal, rgb, weight, voxel, counts
    project_points(v, dim, vs, xyz, model, tol, max_iters)        -> dict of status, xyz, residual, normal, voxel, iterations, distance, counts
    cast_rays(v, dim, vs, origins, directions, t_min, t_max)      -> dict of status, t, xyz, normal, rgb, voxel, counts (+ t_walk: the walk's own float64 t)
    ray_outputs(v, vs, origins, directions, t_min, t, voxel)      -> xyz, normal, rgb as they follow from the walk's float32 t and the hit voxel
v: dict of dist [n], grad [3, n], weight [n], rgb [3, n] (x fastest; what Api.download_volume returns).  model: 0 / "cell", 1 / "trilinear"."""
import numpy as np

import _bake_ref as bref

f32 = np.float32
CELL, TRILINEAR = 0, 1
MODELS = {"cell": CELL, "trilinear": TRILINEAR, 0: CELL, 1: TRILINEAR}
OK, OUTSIDE, UNOBSERVED, INVALID, NOT_CONVERGED = 0, 1, 2, 3, 4
HIT, MISS, BURIED, RAY_INVALID = 0, 1, 2, 3
POINT_COUNTS = ("n", "n_ok", "n_outside", "n_unobserved", "n_invalid")
PROJECT_COUNTS = ("n", "n_converged", "n_left", "n_not_converged", "n_invalid")
RAY_COUNTS = ("n", "n_valid", "n_hits", "n_buried")


def unit(v, lin):
    """m(v) of voxels lin [n]: [n, 3] float64"""
    g = np.asarray(v["grad"])[:, lin].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        ok = s > 0
        r = np.sqrt(np.where(ok, s, 1.0))
        return np.where(ok[None, :], g / r[None, :], 0.0).T


def lerp(A, B, t):
    return A + t * (B - A)


def evaluate(v, dim, vs, p, model, full=False):
    """the model at p [n, 3] float64: status [n], phi [n], normal [n, 3], voxel [n] (and rgb [n, 3], weight [n] if full); phi, normal, rgb and
    weight are zero unless the status is 0"""
    dim = np.asarray(dim, np.int64)
    nx, nxy = int(dim[0]), int(dim[0]) * int(dim[1])
    n = len(p)
    status = np.full(n, OUTSIDE, np.uint8); phi = np.zeros(n); nrm = np.zeros((n, 3)); vox = np.full(n, -1, np.int64)
    col = np.zeros((n, 3)); wgt = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore"):
        u = p / vs + 0.5 if model == CELL else p / vs
        c = np.floor(u)
        fr = u - c
        inside = ((c >= 0) & (c < (dim if model == CELL else dim - 1)[None, :])).all(1)
    a = np.nonzero(inside)[0]
    ci = c[a].astype(np.int64)
    lin = (ci[:, 2] * int(dim[1]) + ci[:, 1]) * nx + ci[:, 0]
    weight = np.asarray(v["weight"]); dist = np.asarray(v["dist"]); rgb = np.asarray(v["rgb"])
    if model == CELL:
        vox[a] = lin
        obs = weight[lin] > 0
        status[a] = np.where(obs, OK, UNOBSERVED)
        a, lin, ci = a[obs], lin[obs], ci[obs]
        m = unit(v, lin)
        e = p[a] - vs * ci.astype(np.float64)
        phi[a] = dist[lin].astype(np.float64) + ((m[:, 0] * e[:, 0] + m[:, 1] * e[:, 1]) + m[:, 2] * e[:, 2])
        nrm[a] = m
        if full:
            col[a] = rgb[:, lin].astype(np.float64).T; wgt[a] = weight[lin].astype(np.float64)
    else:
        corner = [lin + (i & 1) + ((i >> 1) & 1) * nx + (i >> 2) * nxy for i in range(8)]      # i = x + 2 y + 4 z
        obs = np.all([weight[cr] > 0 for cr in corner], axis=0) if len(a) else np.zeros(0, bool)
        status[a] = np.where(obs, OK, UNOBSERVED)
        a, lin = a[obs], lin[obs]
        corner = [cr[obs] for cr in corner]
        f = fr[a]
        vox[a] = lin

        def tri(X):      # X: the eight corners' values, each [n]
            Xyz = [lerp(X[2 * yz], X[2 * yz + 1], f[:, 0]) for yz in range(4)]
            return lerp(lerp(Xyz[0], Xyz[1], f[:, 1]), lerp(Xyz[2], Xyz[3], f[:, 1]), f[:, 2])
        phi[a] = tri([dist[cr].astype(np.float64) for cr in corner])
        ms = [unit(v, cr) for cr in corner]
        S = np.stack([tri([m[:, k] for m in ms]) for k in range(3)], 1) if len(a) else np.zeros((0, 3))
        with np.errstate(invalid="ignore", over="ignore"):
            ss = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
            ok = ss > 0
            nrm[a] = np.where(ok[:, None], S / np.sqrt(np.where(ok, ss, 1.0))[:, None], 0.0)
        if full and len(a):
            col[a] = np.stack([tri([rgb[k, cr].astype(np.float64) for cr in corner]) for k in range(3)], 1)
            wgt[a] = tri([weight[cr].astype(np.float64) for cr in corner])
    return (status, phi, nrm, vox, col, wgt) if full else (status, phi, nrm, vox)


def _points(xyz):
    q32 = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    return q32, np.isfinite(q32).all(1)


def query_points(v, dim, vs, xyz, model):
    model = MODELS[model]
    vs = float(f32(vs))
    q32, finite = _points(xyz)
    n = len(q32)
    status = np.full(n, INVALID, np.uint8); dist = np.zeros(n, f32); nrm = np.zeros((n, 3), f32); col = np.zeros((n, 3), f32); wgt = np.zeros(n, f32)
    vox = np.full(n, -1, np.int64)
    a = np.nonzero(finite)[0]
    s, phi, m, vx, c, w = evaluate(v, dim, vs, q32[a].astype(np.float64), model, full=True)
    status[a] = s; dist[a] = phi.astype(f32); nrm[a] = m.astype(f32); col[a] = c.astype(f32); wgt[a] = w.astype(f32); vox[a] = vx
    counts = dict(n=n, n_ok=int((status == OK).sum()), n_outside=int((status == OUTSIDE).sum()), n_unobserved=int((status == UNOBSERVED).sum()), n_invalid=int((status == INVALID).sum()))
    return dict(status=status, dist=dist, normal=nrm, rgb=col, weight=wgt, voxel=vox, counts=counts)


def check_project_params(model, tol, max_iters, reserved=0.0):
    if model not in MODELS:
        raise ValueError("model")
    if not (1 <= int(max_iters) <= 64):
        raise ValueError("max_iters")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tol")
    if reserved != 0:
        raise ValueError("reserved")


def project_points(v, dim, vs, xyz, model, tol, max_iters):
    check_project_params(model, tol, max_iters)
    model = MODELS[model]
    vs = float(f32(vs))
    q32, finite = _points(xyz)
    n = len(q32)
    status = np.full(n, INVALID, np.uint8)
    p = q32.astype(np.float64); p0 = p.copy()
    res = np.zeros(n); nrm = np.zeros((n, 3)); vox = np.full(n, -1, np.int64); its = np.zeros(n, np.uint8)
    sg = np.ones(n); started = np.zeros(n, bool)
    active = finite.copy()
    k = 0
    while active.any():
        a = np.nonzero(active)[0]
        s, phi, m, vx = evaluate(v, dim, vs, p[a], model)
        vox[a] = vx
        if k == 0:
            started[a[s == OK]] = True
            sg[a[(s == OK) & (phi < 0)]] = -1.0
        left = s != OK
        with np.errstate(invalid="ignore"):
            conv = ~left & (np.abs(phi) <= tol)
        notc = ~left & ~conv & (k == max_iters)
        stop = left | conv | notc
        status[a[left]] = s[left]; status[a[conv]] = OK; status[a[notc]] = NOT_CONVERGED
        fin = conv | notc
        res[a[fin]] = phi[fin]; nrm[a[fin]] = m[fin]; its[a[stop]] = k
        go = ~stop
        p[a[go]] = p[a[go]] - phi[go, None] * m[go]
        active[a[stop]] = False
        k += 1
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - p0
        moved = np.where(started, sg * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), 0.0)
        out = np.where(finite[:, None], p.astype(f32), q32)
    left = (status == OUTSIDE) | (status == UNOBSERVED)
    counts = dict(n=n, n_converged=int((status == OK).sum()), n_left=int(left.sum()), n_not_converged=int((status == NOT_CONVERGED).sum()), n_invalid=int((status == INVALID).sum()))
    return dict(status=status, xyz=out, residual=res.astype(f32), normal=nrm.astype(f32), voxel=vox, iterations=its, distance=moved.astype(f32), counts=counts)


def check_ray_params(t_min, t_max):
    if not (np.isfinite(t_min) and t_min >= 0):
        raise ValueError("t_min")
    if not (t_max > t_min):
        raise ValueError("t_max")


def _rays(origins, directions):
    """o, w [n, 3] float64 (w of unit length where valid), valid [n]"""
    o32 = np.ascontiguousarray(origins, f32).reshape(-1, 3); w32 = np.ascontiguousarray(directions, f32).reshape(-1, 3)
    o, w = o32.astype(np.float64), w32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        ok = ln > 0
        w = np.where(ok[:, None], w / np.where(ok, ln, 1.0)[:, None], w)
    return o, w, ok & np.isfinite(o32).all(1) & np.isfinite(w32).all(1)


def ray_outputs(v, vs, origins, directions, t_min, t, voxel):
    """xyz, normal, rgb [n, 3] float32 as the definition derives them from the WALK's float32 parameter t (T = (double) t + t_min) and the hit
    voxel; with t_min == 0 the call's own output t is that parameter.  Rows without a hit (voxel < 0) are zero."""
    vs = float(f32(vs))
    o, w, _ = _rays(origins, directions)
    hit = np.asarray(voxel) >= 0
    T = np.asarray(t, f32).astype(np.float64) + float(t_min)
    n = len(o)
    xyz = np.zeros((n, 3), f32); nrm = np.zeros((n, 3), f32); col = np.zeros((n, 3), f32)
    h = np.nonzero(hit)[0]
    lin = np.asarray(voxel)[h]
    xyz[h] = (o[h] + T[h, None] * w[h]).astype(f32)
    nrm[h] = unit(v, lin).astype(f32)
    col[h] = np.asarray(v["rgb"])[:, lin].T
    return xyz, nrm, col


def cast_rays(v, dim, vs, origins, directions, t_min=0.0, t_max=np.inf):
    check_ray_params(t_min, t_max)
    vs = float(f32(vs))
    o, w, valid = _rays(origins, directions)
    n = len(o)
    span = float(t_max) - float(t_min)
    status = np.full(n, RAY_INVALID, np.uint8); t = np.zeros(n, f32); vox = np.full(n, -1, np.int64); t_walk = np.zeros(n)
    a = np.nonzero(valid)[0]
    if len(a):
        os_ = o[a] + float(t_min) * w[a]
        uo = (os_ / vs + 0.5).astype(f32); uw = (w[a] / vs).astype(f32)
        tt, vx, found = bref.walk(v["dist"], v["grad"], v["weight"], dim, vs, uo, uw)
        t32 = tt.astype(f32)
        hit = found & (t32.astype(np.float64) <= span)
        status[a] = np.where(hit, np.where(t32 == 0, BURIED, HIT), MISS)
        t_walk[a] = np.where(hit, tt, 0.0)
        t[a] = np.where(hit, (t32.astype(np.float64) + float(t_min)).astype(f32), f32(0))
        vox[a] = np.where(hit, vx, -1)
        tw32 = np.zeros(n, f32); tw32[a] = np.where(hit, t32, f32(0))
    else:
        tw32 = np.zeros(n, f32)
    xyz, nrm, col = ray_outputs(v, vs, origins, directions, t_min, tw32, vox)
    hits = (status == HIT) | (status == BURIED)
    counts = dict(n=n, n_valid=int(valid.sum()), n_hits=int(hits.sum()), n_buried=int((status == BURIED).sum()))
    return dict(status=status, t=t, xyz=xyz, normal=nrm, rgb=col, voxel=vox, counts=counts, t_walk=t_walk, t_walk32=tw32)
