"""Yardstick of the baked detail maps (include/psgsdf_bake.h psgsdf_bake_lod, DESIGN.md "Baked detail maps"), in numpy float64, written from the
definition: the atlas layout and the texture coordinates by integer arithmetic, the sample point and normal of every owned texel, the ray set up in
double and rounded to float32 exactly as the definition says, and the renderer's walk as tests/_render_ref.py restates it (float64, no brick map),
generalised here to one origin per ray.  Shared by tests/test_bake_cpu.py and tests/test_bake_gpu.py.

    layout(F, R)                  -> B, nblk, bpr, W, H and per texel face [H, W] (-1: padding), a, b [H, W]
    uv(F, R)                      -> [F, 3, 2] float32
    lod_mesh(v, dim, vs, cell, **filter) -> the input mesh from the mesh yardsticks (_mesh_ref, _mesh_components_ref, _mesh_lod_ref)
    bake(v, dim, vs, mesh, R, reach, band_lin=None) -> what Api.bake_lod returns for the atlas (plus on_band [H, W])
v: dict of dist [n], grad [3, n], weight [n], rgb [3, n] (x fastest; what Api.download_volume returns)."""
import numpy as np

MAX_SIDE = 16384
f32 = np.float32


def layout(F, R):
    F, R = int(F), int(R)
    if R < 1:
        raise ValueError("res")
    B = R + 1
    nblk = (F + 1) // 2
    bpr = 0
    while bpr * bpr < nblk:
        bpr += 1
    W = bpr * B
    H = -(-nblk // bpr) * B if nblk else 0
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError("atlas beyond 16384")
    Y, X = np.mgrid[0:H, 0:W]
    i, j = X % B, Y % B
    q = (Y // B) * bpr + X // B
    even = i + j <= R
    face = np.where(even, 2 * q, 2 * q + 1)
    a = np.where(even, i, R - i)
    b = np.where(even, j, R - j)
    pad = (q >= nblk) | (face >= F)
    face = np.where(pad, -1, face).astype(np.int32)
    return dict(B=B, nblk=nblk, bpr=bpr, W=W, H=H, face=face, a=np.where(pad, 0, a), b=np.where(pad, 0, b))


def uv(F, R):
    """corners in sixths of a texel: one division of two integers per coordinate"""
    L = layout(F, R)
    B, bpr, W, H = L["B"], L["bpr"], L["W"], L["H"]
    f = np.arange(F, dtype=np.int64)
    q = f >> 1
    x0, y0 = 6 * (q % max(bpr, 1)) * B, 6 * (q // max(bpr, 1)) * B
    R6 = 6 * int(R)
    even = np.array([[1, 1], [R6 + 7, 1], [1, R6 + 7]], np.int64)
    odd = np.array([[R6 + 5, R6 + 5], [-1, R6 + 5], [R6 + 5, -1]], np.int64)
    m = np.where((f & 1)[:, None, None] == 1, odd[None], even[None])
    out = np.empty((F, 3, 2), np.float64)
    out[:, :, 0] = (x0[:, None] + m[:, :, 0]).astype(np.float64) / float(6 * W) if F else 0
    out[:, :, 1] = (y0[:, None] + m[:, :, 1]).astype(np.float64) / float(6 * H) if F else 0
    return out.astype(f32)


def weights(a, b, R):
    w1 = (3.0 * a + 1.0) / (3.0 * (R + 1))
    w2 = (3.0 * b + 1.0) / (3.0 * (R + 1))
    return 1.0 - w1 - w2, w1, w2


def _unit(v):
    """v / |v| per row; ok = |v| > 0 (rows with |v| = 0 are left as they are)"""
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    ok = ln > 0
    return np.where(ok[:, None], v / np.where(ok, ln, 1.0)[:, None], v), ok


def sample(xyz, normals, faces, face, a, b, R):
    """the owned texels (face, a, b: flat arrays) -> w [T, 3], p [T, 3], n [T, 3] (zero rows: no ray), ray [T]"""
    w0, w1, w2 = weights(a.astype(np.float64), b.astype(np.float64), R)
    fv = np.asarray(faces, np.int64)[face]
    x = np.asarray(xyz, f32).astype(np.float64)[fv]          # [T, 3 corners, 3]
    nn = np.asarray(normals, f32).astype(np.float64)[fv]
    p = (w0[:, None] * x[:, 0] + w1[:, None] * x[:, 1]) + w2[:, None] * x[:, 2]
    n = (w0[:, None] * nn[:, 0] + w1[:, None] * nn[:, 1]) + w2[:, None] * nn[:, 2]
    n, ok = _unit(n)
    e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    cr, ok2 = _unit(cr)
    n = np.where(ok[:, None], n, np.where(ok2[:, None], cr, 0.0))
    return np.stack([w0, w1, w2], 1), p, n, ok | ok2


def walk(dist, grad, weight, dim, vs, uo, uw):
    """tests/_render_ref.py trace() with one origin per ray.  uo, uw [n, 3].  Returns (t [n], voxel [n] (-1), found [n])."""
    dim = np.asarray(dim, np.int64)
    vs = float(vs)
    uo = np.asarray(uo, np.float64); uw = np.asarray(uw, np.float64)
    n = len(uo)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(uw != 0, 1.0 / np.where(uw != 0, uw, 1.0), 0.0)
        ta = (0.0 - uo) * inv
        tb = (dim[None, :] - uo) * inv
    inside = (uo >= 0) & (uo < dim)
    lo_t = np.where(uw != 0, np.minimum(ta, tb), -np.inf)
    hi_t = np.where(uw != 0, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf))
    t0 = np.maximum(0.0, lo_t.max(1)) if n else np.zeros(0)
    t1 = hi_t.min(1) if n else np.zeros(0)
    step = np.sign(uw).astype(np.int64)
    c = np.clip(np.floor(uo + t0[:, None] * uw).astype(np.int64), 0, dim - 1)
    t = t0.copy()
    active = t0 < t1
    t_hit = np.zeros(n)
    vox = np.full(n, -1, np.int64)
    g = np.asarray(grad).astype(np.float64)
    d64 = np.asarray(dist).astype(np.float64)
    for _ in range(int(dim.sum()) + 8):
        a = np.nonzero(active)[0]
        if len(a) == 0:
            break
        ca, ua, sa, ia, ta_, oa = c[a], uw[a], step[a], inv[a], t[a], uo[a]
        bound = ca + (sa > 0)
        with np.errstate(invalid="ignore"):
            tt = np.where(sa != 0, (bound - oa) * ia, np.inf)
        ax = tt.argmin(1)
        te = tt[np.arange(len(a)), ax]
        lin = ca[:, 0] + ca[:, 1] * dim[0] + ca[:, 2] * dim[0] * dim[1]
        obs = weight[lin] > 0
        gr = g[:, lin].T
        nrm = np.linalg.norm(gr, axis=1)
        gn = np.where(nrm[:, None] > 0, gr / np.where(nrm > 0, nrm, 1.0)[:, None], gr)
        loc = (oa + ta_[:, None] * ua) - (ca + 0.5)
        phi0 = d64[lin] + vs * (gn * loc).sum(1)
        s = vs * (gn * ua).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            th = ta_ - phi0 / s
        h0 = obs & (phi0 <= 0)
        h1 = obs & ~h0 & (s < 0) & (th <= te)
        hit = h0 | h1
        t_hit[a[h0]] = ta_[h0]
        t_hit[a[h1]] = th[h1]
        vox[a[hit]] = lin[hit]
        active[a[hit]] = False
        rest = ~hit
        ar, axr = a[rest], ax[rest]
        c[ar, axr] += step[ar, axr]
        out = (c[ar, axr] < 0) | (c[ar, axr] >= dim[axr])
        active[ar[out]] = False
        t[ar] = np.maximum(t[ar], te[rest])
    return t_hit, vox, vox >= 0


def lod_mesh(v, dim, vs, cell, **flt):
    """the input mesh of the definition: the welded mesh, filtered by its components if a filter is given, clustered"""
    import _mesh_components_ref as cref
    import _mesh_lod_ref as lref
    import _mesh_ref as ref
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    if flt:
        m = cref.components(xyz, faces, vs, nrm, rgb, **flt)
        xyz, nrm, rgb, faces = m["xyz"], m["normals"], m["rgb"], m["faces"]
    return lref.lod(xyz, nrm, rgb, faces, vs, cell)


def unit_f32(g):
    """device_common.h normalized3 on float32 rows [T, 3]"""
    g = np.asarray(g, f32)
    z = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    s = np.sqrt(np.where(z > 0, z, f32(1)))
    return np.where((z > 0)[:, None], g / s[:, None], g).astype(f32)


def colour_byte(c):
    c = np.asarray(c, f32)
    return np.floor(f32(255.0) * np.clip(c, f32(0), f32(1)) + f32(0.5)).astype(np.uint8)


def bake(v, dim, vs, mesh, R, reach, band_lin=None):
    """mesh: dict of xyz, normals, rgb, faces.  band_lin: the band's linear voxel indices (hits there are on the band: their normal and albedo are
    the band's, which this yardstick does not have -- it fills in the off-band values and says so in on_band)."""
    vs = float(f32(vs))
    reach = float(reach)
    if not (np.isfinite(reach) and reach > 0):
        raise ValueError("reach")
    F = len(mesh["faces"])
    L = layout(F, R)
    W, H = L["W"], L["H"]
    own = np.nonzero(L["face"].ravel() >= 0)[0]
    face, a, b = L["face"].ravel()[own], L["a"].ravel()[own], L["b"].ravel()[own]
    w, p, n, ray = sample(mesh["xyz"], mesh["normals"], mesh["faces"], face, a, b, R)
    o = p + reach * n
    uo = (o / vs + 0.5).astype(f32)
    uw = (-n / vs).astype(f32)
    t = np.zeros(len(own)); vox = np.full(len(own), -1, np.int64); found = np.zeros(len(own), bool)
    r = np.nonzero(ray)[0]
    t[r], vox[r], found[r] = walk(v["dist"], v["grad"], v["weight"], dim, vs, uo[r], uw[r])
    hit = found & (t > 0) & (t <= 2.0 * reach)
    buried = found & (t == 0)
    T = len(own)
    albedo = np.zeros((T, 3), np.uint8); normal = np.zeros((T, 3), f32); disp = np.zeros(T, f32); voxel = np.full(T, -1, np.int32)
    h = np.nonzero(hit)[0]
    voxel[h] = vox[h]
    disp[h] = (reach - t[h]).astype(f32)
    normal[h] = unit_f32(np.asarray(v["grad"], f32)[:, vox[h]].T)
    albedo[h] = colour_byte(np.asarray(v["rgb"], f32)[:, vox[h]].T)
    m = np.nonzero(~hit)[0]
    normal[m] = n[m].astype(f32)
    cb = np.asarray(mesh["rgb"], np.uint8).astype(np.float64)[np.asarray(mesh["faces"], np.int64)[face[m]]]      # [M, 3 corners, 3]
    albedo[m] = np.floor(((w[m, 0, None] * cb[:, 0] + w[m, 1, None] * cb[:, 1]) + w[m, 2, None] * cb[:, 2]) + 0.5).astype(np.uint8)
    on_band = np.zeros(T, bool)
    if band_lin is not None:
        on_band[h] = np.isin(vox[h], np.asarray(band_lin, np.int64))

    def plane(x, fill, dt):
        out = np.full((H * W,) + x.shape[1:], fill, dt)
        out[own] = x
        return out.reshape((H, W) + x.shape[1:])
    return dict(width=W, height=H, uv=uv(F, R), face=L["face"], albedo=plane(albedo, 0, np.uint8), normal=plane(normal, 0, f32), displacement=plane(disp, 0, f32),
                voxel=plane(voxel, -1, np.int32), on_band=plane(on_band, False, bool), t=plane(t, 0.0, np.float64),
                n_texels=T, n_hits=int(hit.sum()), n_hits_off_band=int((hit & ~on_band).sum()), n_buried=int(buried.sum()), n_misses=int(T - hit.sum() - buried.sum()))
