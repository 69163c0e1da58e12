"""numpy restatement, in float64, of the photometric fit per band row and per welded-mesh vertex (include/psgsdf_fit.h; DESIGN.md "Photometric fit per
voxel and vertex").  The yardstick of tests/test_fit_cpu.py and tests/test_fit_gpu.py.

    band_fit(state)                      -> dict n_obs [S] int64, loss [S] float64, sum_r2 [S, 3] float64, margin_px, min_depth
    vertex_fit(rows, band, keys, dim)    -> (n_obs [V] int64, rms [V] float32, loss [V] float32) from per-row arrays and the vertices' keys
    mesh_keys(v, dim, vs)                -> the keys of the welded mesh's vertices, ascending (tests/_mesh_ref.py's own)

state: dict of band [S] (linear voxel indices, ascending), dist [n], grad [3, n], rgb [3, n], vis [n, words] uint64 (the layout of Api.download_volume),
dim, vs, origin [3] (Api.info), poses [F, 16] camera->world, light ([F, nb] SH; [3] LED), images [F, H, W, 3] float, K = (fx, fy, cx, cy), model
(0 SH1, 1 SH2, 2 LED), loss (0 L2, 1 Cauchy, 2 Huber, 3 Tukey, 4 truncated L2), lam.

The forward model of the energy, row by row: surface point xs = x_v - d normalised(stored gradient); the finite-difference normal (forward where
the +axis neighbour is a band row, otherwise backward, from the dense distances); per visible frame the projection, the bilinear sample, the model's
rendered colour and the residual.  tests/_render_ref.py has the ray traversal and the cameras, no shading: the three shading models are restated here."""
import numpy as np

import _mesh_ref as mref

f64 = np.float64


def _normalised(v):
    z = (v * v).sum(-1, keepdims=True)
    return np.where(z > 0, v / np.sqrt(np.where(z > 0, z, 1.0)), v)


def robust_loss(r, loss, lam):
    x = r / lam
    if loss == 1:
        return np.log1p(x * x)
    if loss == 3:
        u = 1.0 - x * x
        return np.where(r * r < lam * lam, 1.0 - u * u * u, 1.0)
    if loss == 2:
        return np.where(r * r < lam * lam, 0.5 * r * r, lam * (np.abs(r) - 0.5 * lam))
    if loss == 4:
        return np.clip(r, -lam, lam) ** 2
    return r * r


def popcount_below(vis_rows, F):
    """set bits below F of every row's visibility words"""
    n = np.zeros(len(vis_rows), np.int64)
    for f in range(F):
        n += ((vis_rows[:, f >> 6] >> np.uint64(f & 63)) & np.uint64(1)).astype(np.int64)
    return n


def band_fit(st, need_margin=2.0):
    """need_margin: every candidate projection must lie at least that many pixels away from the image border -- inside it, or (a frame that does not
    see the object at all) outside -- and at positive depth, so that no in / out decision of the float32 engine is a near-tie; asserted here."""
    nx, ny, nz = (int(x) for x in st["dim"])
    band = np.asarray(st["band"], np.int64)
    S = len(band)
    vs = float(np.float32(st["vs"]))
    dist = np.asarray(st["dist"], f64)
    row = np.full(nx * ny * nz, -1, np.int64); row[band] = np.arange(S)
    k, rest = np.divmod(band, nx * ny); j, i = np.divmod(rest, nx)
    idx = np.stack([i, j, k], 1)
    assert (idx >= 1).all() and (idx < np.array([nx, ny, nz]) - 1).all(), "the band touches the grid's faces"
    d = dist[band]
    stride = (1, nx, nx * ny)
    n = np.zeros((S, 3))
    for a in range(3):      # forward difference iff the +axis neighbour is a band row, else backward
        fwd = row[band + stride[a]] >= 0
        n[:, a] = np.where(fwd, dist[band + stride[a]] - d, -(dist[band - stride[a]] - d)) / vs
    nfd = _normalised(n)
    gn = _normalised(np.asarray(st["grad"], f64)[:, band].T)
    xs = np.asarray(st["origin"], f64) + vs * idx - d[:, None] * gn
    rho = np.asarray(st["rgb"], f64)[:, band].T
    img = np.asarray(st["images"], f64)
    F, H, W = img.shape[:3]
    fx, fy, cx, cy = (float(x) for x in st["K"])
    model, loss, lam = int(st["model"]), int(st["loss"]), float(np.float32(st["lam"]))
    light = np.asarray(st["light"], f64)
    sh = np.concatenate([np.ones((S, 1)), nfd], 1)
    if model == 1:
        sh = np.concatenate([sh, np.stack([nfd[:, 0] * nfd[:, 1], nfd[:, 0] * nfd[:, 2], nfd[:, 1] * nfd[:, 2], nfd[:, 0] ** 2 - nfd[:, 1] ** 2, nfd[:, 0] ** 2 - nfd[:, 2] ** 2], 1)], 1)
    vis = np.asarray(st["vis"])[band]
    n_obs = np.zeros(S, np.int64); L = np.zeros(S); Q = np.zeros((S, 3))
    margin, zmin = np.inf, np.inf
    for f in range(F):
        seen = ((vis[:, f >> 6] >> np.uint64(f & 63)) & np.uint64(1)).astype(bool)
        if not seen.any():
            continue
        P = np.asarray(st["poses"], f64)[f].reshape(4, 4)
        R, t = P[:3, :3], P[:3, 3]
        p = (xs[seen] - t) @ R                      # camera coordinates R^T (xs - t)
        zmin = min(zmin, p[:, 2].min())
        m = fx * p[:, 0] / p[:, 2] + cx             # column
        q = fy * p[:, 1] / p[:, 2] + cy             # row
        edge = np.minimum(np.minimum(m, W - 1 - m), np.minimum(q, H - 1 - q))      # > 0: that far inside the last row / column, < 0: outside
        margin = min(margin, np.abs(edge).min())
        ok = edge > 0
        r_ = np.nonzero(seen)[0][ok]
        m, q, p = m[ok], q[ok], p[ok]
        y0, x0 = np.floor(q).astype(np.int64), np.floor(m).astype(np.int64)
        fq, fm = (q - y0)[:, None], (m - x0)[:, None]
        im = img[f]
        I = (im[y0 + 1, x0] * fq * (1 - fm) + im[y0, x0] * (1 - fq) * (1 - fm)) + im[y0 + 1, x0 + 1] * fq * fm + im[y0, x0 + 1] * (1 - fq) * fm
        if model == 2:
            irr = -(nfd[r_] * (p @ R.T)).sum(1) / np.linalg.norm(p, axis=1) ** 3
            ren = rho[r_] * light[None, :3] * irr[:, None]
        else:
            ren = rho[r_] * (sh[r_] * light[f][None, :sh.shape[1]]).sum(1)[:, None]
        res = I - ren
        n_obs[r_] += 1
        L[r_] += robust_loss(res, loss, lam).sum(1)
        Q[r_] += res * res
    assert zmin > 0 and margin >= need_margin, (zmin, margin)
    return dict(n_obs=n_obs, loss=L, sum_r2=Q, margin_px=float(margin), min_depth=float(zmin))


def vertex_fit(n_obs, loss, sum_r2, band, keys, dim):
    """the definition of include/psgsdf_fit.h from per-row arrays: every operation a correctly rounded double one, then one rounding to float32"""
    nx, ny, nz = (int(x) for x in dim)
    band = np.asarray(band, np.int64); keys = np.asarray(keys, np.int64)
    row = np.full(nx * ny * nz, -1, np.int64); row[band] = np.arange(len(band))
    typ, lin = keys & 3, keys >> 2
    step = np.array([1, nx, nx * ny, 0])[typ]
    n = np.zeros(len(keys), np.int64); L = np.zeros(len(keys)); Q = np.zeros(len(keys))
    r2 = np.asarray(sum_r2, np.float32).astype(f64)
    for e in range(2):
        r = row[lin + e * step]
        use = (r >= 0) & ((e == 0) | (typ != 3))
        rr = r[use]
        n[use] += np.asarray(n_obs, np.int64)[rr]
        L[use] += np.asarray(loss, f64)[rr]
        for c in range(3):
            Q[use] += r2[rr, c]
    has = n > 0
    nn = np.where(has, n, 1).astype(f64)
    rms = np.where(has, np.sqrt(Q / (3.0 * nn)), 0.0).astype(np.float32)
    vl = np.where(has, L / nn, 0.0).astype(np.float32)
    return n, rms, vl


def mesh_keys(v, dim, vs):
    """the ascending keys 4 * lin + e of the welded mesh's vertices: what tests/_mesh_ref.py hands to its vertices() (spied on, the module is left as it is)"""
    seen = {}
    orig = mref.vertices

    def spy(v_, dim_, vkeys, *rest):
        seen["keys"] = np.asarray(vkeys, np.int64).copy()
        return orig(v_, dim_, vkeys, *rest)
    mref.vertices = spy
    try:
        out = mref.mesh(v, dim, vs)
    finally:
        mref.vertices = orig
    return seen.get("keys", np.zeros(0, np.int64)), out
