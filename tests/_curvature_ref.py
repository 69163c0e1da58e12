"""Yardstick of the surface curvature (include/psgsdf_curvature.h, DESIGN.md "Surface curvature"): the definition in numpy float64, one IEEE operation
per step in the order the header writes them, rounded to float32 at the end; the vertex rule from per-voxel float arrays with tests/_mesh_ref.py's
keys and interpolation parameter; and the adjugate formulation of the same two invariants, which the frame formulation must reproduce.  Shared by
tests/test_curvature_cpu.py and tests/test_curvature_gpu.py.

    voxels(v, dim, vs, lin)           -> dict of valid [n] uint8, mean, gauss, k1, k2 [n] float32, dir1 [n, 3] float32 (+ "f64": the same before rounding)
    adjugate(v, dim, vs, lin)         -> (mean, gauss) [n] float64 by (G2 tr H - g'Hg) / (2 G2 G) and g' adj(H) g / G2^2 (NaN where invalid)
    mesh_keys(v, dim, vs)             -> the keys 4 lin + e of the welded mesh's vertices, in vertex order
    vertices(v, dim, vkeys, per_voxel) -> dict of valid [V] uint8, mean, gauss, k1, k2 [V] float32; per_voxel(lin) returns voxels()'s dict for lin
    png_byte(mean, valid, vs, S)      -> the grey byte of voxelPS --mesh-bake-curvature S
v: dict of dist [n], weight [n] (x fastest; what Api.download_volume returns); dim = (nx, ny, nz)."""
import numpy as np

import _mesh_ref as mref

f32, f64 = np.float32, np.float64
SCALARS = ("mean", "gauss", "k1", "k2")
AXES = ((0, 1), (0, 2), (1, 2))


def _stencil(v, dim, lin):
    """valid-so-far [n] and D: a function of an offset (di, dj, dk) giving the distances [n] in double (zeros where the voxel cannot be evaluated)"""
    nx, ny, nz = (int(x) for x in dim)
    lin = np.asarray(lin, np.int64).reshape(-1)
    dist, weight = np.asarray(v["dist"], f32).reshape(-1), np.asarray(v["weight"], f32).reshape(-1)
    ok = (lin >= 0) & (lin < nx * ny * nz)
    l0 = np.where(ok, lin, 0)
    k, rest = np.divmod(l0, nx * ny)
    j, i = np.divmod(rest, nx)
    ok &= (i >= 1) & (i <= nx - 2) & (j >= 1) & (j <= ny - 2) & (k >= 1) & (k <= nz - 2)
    l0 = np.where(ok, l0, (ny + 1) * nx + 1)      # (a voxel whose stencil is in range, to keep the gathers legal; masked out below)
    if nx < 3 or ny < 3 or nz < 3:
        return np.zeros(len(lin), bool), None
    off = lambda o: l0 + (o[2] * ny + o[1]) * nx + o[0]
    offs = [(0, 0, 0)]
    for a in range(3):
        for s in (1, -1):
            o = [0, 0, 0]; o[a] = s; offs.append(tuple(o))
    for a, b in AXES:
        for sa in (1, -1):
            for sb in (1, -1):
                o = [0, 0, 0]; o[a] = sa; o[b] = sb; offs.append(tuple(o))
    assert len(set(offs)) == 19
    for o in offs:
        ok &= weight[off(o)] > 0
    return ok, (lambda o: dist[off(o)].astype(f64))


def _derivatives(v, dim, vs, lin):
    ok, D = _stencil(v, dim, lin)
    n = len(ok)
    if D is None:
        return ok, np.zeros((3, n)), np.zeros((3, 3, n))
    h = float(f32(vs))
    unit = lambda a, s=1: tuple(s if q == a else 0 for q in range(3))
    d0 = D((0, 0, 0))
    g = np.zeros((3, n)); H = np.zeros((3, 3, n))
    for a in range(3):
        p, m = D(unit(a)), D(unit(a, -1))
        g[a] = (p - m) / (2.0 * h)
        H[a, a] = ((p + m) - 2.0 * d0) / (h * h)
    for a, b in AXES:
        o = lambda sa, sb: tuple(sa if q == a else sb if q == b else 0 for q in range(3))
        H[a, b] = H[b, a] = ((D(o(1, 1)) + D(o(-1, -1))) - (D(o(1, -1)) + D(o(-1, 1)))) / (4.0 * h * h)
    return ok, g, H


def voxels(v, dim, vs, lin):
    ok, g, H = _derivatives(v, dim, vs, lin)
    n = len(ok)
    with np.errstate(all="ignore"):
        G2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        ok = ok & (G2 > 0)
        G2 = np.where(ok, G2, 1.0)
        G = np.sqrt(G2)
        m = g / G
        sg = np.copysign(1.0, m[2])
        a_ = -1.0 / (sg + m[2])
        b_ = m[0] * m[1] * a_
        t1 = np.stack([1.0 + sg * m[0] * m[0] * a_, sg * b_, -sg * m[0]])
        t2 = np.stack([b_, sg + m[1] * m[1] * a_, -m[1]])
        Ht = lambda t: np.stack([(H[r, 0] * t[0] + H[r, 1] * t[1]) + H[r, 2] * t[2] for r in range(3)])
        dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
        u1, u2 = Ht(t1), Ht(t2)
        a, b, c = dot(t1, u1) / G, dot(t1, u2) / G, dot(t2, u2) / G
        mean = (a + c) / 2.0
        gauss = a * c - b * b
        hd = (a - c) / 2.0
        s = np.sqrt(hd * hd + b * b)
        k1, k2 = mean + s, mean - s
        e0 = np.where(s == 0, 1.0, np.where(hd >= 0, hd + s, b))
        e1 = np.where(s == 0, 0.0, np.where(hd >= 0, b, s - hd))
        en = np.sqrt(e0 * e0 + e1 * e1)
        e0, e1 = e0 / en, e1 / en
        dir1 = e0 * t1 + e1 * t2
    z = lambda x: np.where(ok, x, 0.0)
    full = dict(mean=z(mean), gauss=z(gauss), k1=z(k1), k2=z(k2), dir1=z(dir1).T.copy())
    out = {k: x.astype(f32) for k, x in full.items()}
    out["valid"] = ok.astype(np.uint8)
    out["f64"] = full
    return out


def adjugate(v, dim, vs, lin):
    ok, g, H = _derivatives(v, dim, vs, lin)
    with np.errstate(all="ignore"):
        G2 = (g * g).sum(0)
        ok = ok & (G2 > 0)
        G2 = np.where(ok, G2, 1.0)
        G = np.sqrt(G2)
        Hg = np.einsum("abn,bn->an", H, g)
        mean = (G2 * (H[0, 0] + H[1, 1] + H[2, 2]) - (g * Hg).sum(0)) / (2.0 * G2 * G)
        adj = np.empty_like(H)
        for a in range(3):
            for b in range(3):
                r = [q for q in range(3) if q != b]; c = [q for q in range(3) if q != a]
                adj[a, b] = (-1) ** (a + b) * (H[r[0], c[0]] * H[r[1], c[1]] - H[r[0], c[1]] * H[r[1], c[0]])
        gauss = (g * np.einsum("abn,bn->an", adj, g)).sum(0) / (G2 * G2)
    return np.where(ok, mean, np.nan), np.where(ok, gauss, np.nan)


def mesh_keys(v, dim, vs):
    """the welded mesh's vertex keys, in vertex order: what tests/_mesh_ref.py's mesh() hands to its vertices()"""
    seen = []
    keep = mref.vertices
    def spy(v_, dim_, vkeys, *rest):
        seen.append(np.asarray(vkeys, np.int64).copy())
        return keep(v_, dim_, vkeys, *rest)
    mref.vertices = spy
    try:
        mref.mesh(v, dim, vs)
    finally:
        mref.vertices = keep
    return seen[0] if seen else np.zeros(0, np.int64)


def vertices(v, dim, vkeys, per_voxel):
    nx, ny, nz = (int(x) for x in dim)
    vkeys = np.asarray(vkeys, np.int64)
    typ, lin = vkeys & 3, vkeys >> 2
    corner = typ == 3
    step = np.array([1, nx, nx * ny, 0], np.int64)[typ]
    linh = lin + step
    lo, hi = per_voxel(lin), per_voxel(linh)
    dist = np.asarray(v["dist"], f32).reshape(-1)
    tl, th = -dist[lin], -dist[linh]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = ((f32(0) - tl) / (th - tl)).astype(f32).astype(f64)
    m = np.clip(mu, 0.0, 1.0).astype(f32).astype(f64)      # (mesh_ref.vertices' mu and m)
    vl, vh = lo["valid"] != 0, hi["valid"] != 0
    both = ~corner & vl & vh
    only_hi = ~corner & ~vl & vh
    out = dict(valid=np.where(corner, 2 * vl.astype(int), vl.astype(int) + vh.astype(int)).astype(np.uint8))
    for name in SCALARS:
        cl, ch = lo[name].astype(f32).astype(f64), hi[name].astype(f32).astype(f64)
        with np.errstate(invalid="ignore"):
            mix = (cl + m * (ch - cl)).astype(f32)
        out[name] = np.where(both, mix, np.where(only_hi, hi[name].astype(f32), lo[name].astype(f32))).astype(f32)      # (an invalid voxel holds zeros)
    return out


def png_byte(mean, valid, vs, S):
    """byte = floor(255 clamp(0.5 + 0.5 (double) mean vs / S, 0, 1) + 0.5); 128 where not valid.  vs: the float32 voxel size, widened"""
    x = 0.5 + 0.5 * np.asarray(mean, f32).astype(f64) * float(f32(vs)) / float(S)
    b = np.floor(255.0 * np.minimum(np.maximum(x, 0.0), 1.0) + 0.5).astype(np.uint8)
    return np.where(np.asarray(valid) != 0, b, np.uint8(128)).astype(np.uint8)
