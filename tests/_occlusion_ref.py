"""Yardstick of the ambient occlusion (include/psgsdf_occlusion.h, DESIGN.md "Ambient occlusion"), in numpy float64, written from the definition: the
direction table, the frame of a normal, the rays set up in double and rounded to float32 exactly as the definition says, and the renderer's walk as
tests/_bake_ref.py restates it (float64, no brick map, NO cut at the radius: the device's cut must not change a bit).  Shared by
tests/test_occlusion_cpu.py and tests/test_occlusion_gpu.py.

    dirs(K)                       -> [K, 3] float64
    frame(m)                      -> t1, t2 [n, 3] of unit normals m [n, 3]
    byte(K, c)                    -> the occlusion byte of c occluded rays of K
    occlusion(v, dim, vs, q, m, K, radius, bias, dirs=None) -> dict of mask [n] uint64, occlusion [n] uint8, bits, buried, t, found [n, K], valid [n], counts
    bake_ao(v, dim, vs, mesh, bake_planes, R, K, radius, bias, dirs=None) -> the same over the atlas [H, W] of the given bake planes
v: dict of dist [n], grad [3, n], weight [n] (x fastest; what Api.download_volume returns).  q: positions, m: normals (any length)."""
import numpy as np

import _bake_ref as bref

f32 = np.float32
KS = (8, 16, 32, 64)
GOLDEN = 0.6180339887498949
COUNTS = ("n_samples", "n_valid", "n_rays", "n_occluded", "n_buried")


def dirs(K):
    i = np.arange(int(K), dtype=np.float64)
    u = (i + 0.5) / float(K)
    r, z = np.sqrt(u), np.sqrt(1.0 - u)
    phi = 2.0 * np.pi * (i * GOLDEN - np.floor(i * GOLDEN))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def frame(m):
    m = np.asarray(m, np.float64).reshape(-1, 3)
    sg = np.copysign(1.0, m[:, 2])
    a = -1.0 / (sg + m[:, 2])
    b = m[:, 0] * m[:, 1] * a
    t1 = np.stack([1.0 + sg * m[:, 0] * m[:, 0] * a, sg * b, -sg * m[:, 0]], 1)
    t2 = np.stack([b, sg + m[:, 1] * m[:, 1] * a, -m[:, 1]], 1)
    return t1, t2


def byte(K, c):
    return (510 * (int(K) - int(c)) + int(K)) // (2 * int(K))


def check_params(K, radius, bias):
    if int(K) not in KS:
        raise ValueError("n_dirs")
    if not (np.isfinite(radius) and radius > 0 and np.isfinite(bias) and bias > 0):
        raise ValueError("radius / bias")


def rays(q, m, D, vs, bias):
    """the definition's rays of unit normals m at q: uo, uw [n, K, 3] float32"""
    t1, t2 = frame(m)
    o = q + bias * m
    w = (D[None, :, 0, None] * t1[:, None, :] + D[None, :, 1, None] * t2[:, None, :]) + D[None, :, 2, None] * m[:, None, :]
    uo = (o / vs + 0.5).astype(f32)
    uw = (w / vs).astype(f32)
    return np.broadcast_to(uo[:, None, :], uw.shape), uw


def trace(v, dim, vs, q, m, valid, K, radius, bias, D=None):
    """q, m [n, 3] float64 with m of unit length where valid; everything per ray [n, K] and per sample [n]"""
    D = dirs(K) if D is None else np.asarray(D, np.float64)
    n = len(q)
    t = np.zeros((n, K)); found = np.zeros((n, K), bool)
    idx = np.nonzero(valid)[0]
    if len(idx):
        uo, uw = rays(q[idx], m[idx], D, vs, bias)
        tt, _, ff = bref.walk(v["dist"], v["grad"], v["weight"], dim, vs, uo.reshape(-1, 3), uw.reshape(-1, 3))
        t[idx] = tt.reshape(-1, K); found[idx] = ff.reshape(-1, K)
    t = t.astype(f32).astype(np.float64)      # (the device's t is a float32: both are compared with the radius as that)
    bits = found & (t <= radius)
    buried = found & (t == 0)
    mask = (bits.astype(np.uint64) << np.arange(K, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64) if n else np.zeros(0, np.uint64)
    c = bits.sum(1)
    occ = ((510 * (K - c) + K) // (2 * K)).astype(np.uint8)
    nv = int(valid.sum())
    return dict(mask=mask, occlusion=occ, bits=bits, buried=buried, t=t, found=found, valid=valid, dirs=D, q=q, m=m,
                n_samples=n, n_valid=nv, n_rays=K * nv, n_occluded=int(bits.sum()), n_buried=int(buried.sum()))


def normalise(nrm):
    """float32 rows widened and divided by their length sqrt((x^2 + y^2) + z^2); ok: the length is > 0"""
    m = np.asarray(nrm, f32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = ln > 0
        return np.where(ok[:, None], m / np.where(ok, ln, 1.0)[:, None], m), ok


def occlusion(v, dim, vs, q, m, K, radius, bias, dirs=None):
    check_params(K, radius, bias)
    vs = float(f32(vs))
    q32, m32 = np.asarray(q, f32).reshape(-1, 3), np.asarray(m, f32).reshape(-1, 3)
    mm, ok = normalise(m32)
    valid = ok & np.isfinite(q32).all(1) & np.isfinite(m32).all(1)
    return trace(v, dim, vs, q32.astype(np.float64), mm, valid, int(K), float(radius), float(bias), dirs)


def bake_ao(v, dim, vs, mesh, bake_planes, R, K, radius, bias, dirs=None):
    """mesh: dict of xyz, normals, faces (the level-of-detail mesh); bake_planes: dict of face, voxel, displacement, normal [H, W(, 3)] -- the
    device's own, or the yardstick's.  Planes [H, W]; padding: byte 0, mask 0."""
    check_params(K, radius, bias)
    vs = float(f32(vs))
    face = np.asarray(bake_planes["face"])
    H, W = face.shape
    L = bref.layout(len(mesh["faces"]), R)
    assert (L["H"], L["W"]) == (H, W) and np.array_equal(L["face"], face)
    own = np.nonzero(face.ravel() >= 0)[0]
    _, p, n, ray = bref.sample(mesh["xyz"], mesh["normals"], mesh["faces"], face.ravel()[own], L["a"].ravel()[own], L["b"].ravel()[own], R)
    hit = np.asarray(bake_planes["voxel"]).ravel()[own] >= 0
    d = np.asarray(bake_planes["displacement"], f32).ravel()[own].astype(np.float64)
    mh, ok = normalise(np.asarray(bake_planes["normal"], f32).reshape(-1, 3)[own])
    q = np.where(hit[:, None], p + d[:, None] * n, p)
    m = np.where((hit & ok)[:, None], mh, n)
    r = trace(v, dim, vs, q, m, ray, int(K), float(radius), float(bias), dirs)

    def plane(x, dt):
        out = np.zeros((H * W,) + x.shape[1:], dt)
        out[own] = x
        return out.reshape((H, W) + x.shape[1:])
    out = {k: r[k] for k in COUNTS}
    out.update(mask=plane(r["mask"], np.uint64), occlusion=plane(r["occlusion"], np.uint8), bits=plane(r["bits"], bool), buried=plane(r["buried"], bool),
               t=plane(r["t"], np.float64), found=plane(r["found"], bool), valid=plane(r["valid"], bool), dirs=r["dirs"], q=plane(q, np.float64), m=plane(m, np.float64))
    return out
