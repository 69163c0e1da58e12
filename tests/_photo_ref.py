"""Yardstick of the albedo texture solved from the keyframes (include/psgsdf_photo.h psgsdf_bake_lod_photo), in numpy, written from the
definition: the sample of every hit texel from the bake's public planes (tests/_bake_ref.py sample, as tests/_occlusion_ref.py bake_ao takes it), the
energy's projection, the angle test, relight's point-light ray towards the camera centre (tests/_relight_ref.py's arithmetic: unit, dot) through the
renderer's walk as tests/_bake_ref.py restates tests/_render_ref.py's (float64, no brick map, no cut), the forward model's shading, the bilinear
sample with its border rule, the robust weight and the two sums in double over the frames in ascending order.
Shared by tests/test_photo_bake_cpu.py and tests/test_photo_bake_gpu.py.

Two modes.  "f32": every step the definition names as float is taken in np.float32 in the device's order of operations (projection, shading,
sample, residual, weight; the ray's uo, uw and hit parameter rounded to float32).  "f64": the same formulas with nothing rounded -- everything in
double.  The difference of the two is the reference's own error: tests take their tolerance from it.

    photo(v, dim, vs, origin, mesh, planes, R, poses, light, images, intr, model, loss, lam, bias, cos_min, shade_min, mode) -> dict
v: dict of dist [n], grad [3, n], weight [n] (x fastest; Api.download_volume).  mesh: the level-of-detail mesh (xyz, normals, faces).  planes: the bake's
face, voxel, displacement, normal, albedo [H, W(, 3)].  poses [F, 16] camera->world float32; light [F, nb] (SH) or [3] (LED); images [F, h, w, 3] the
floats the energy samples; intr = (fx, fy, cx, cy); model 0 SH1, 1 SH2, 2 LED; loss 0 L2, 1 Cauchy, 2 Huber, 3 Tukey, 4 truncated L2."""
import numpy as np

import _bake_ref as bref
import _occlusion_ref as oref
import _relight_ref as lref

f32 = np.float32
USED, OUTSIDE, GRAZING, OCCLUDED, DARK, NO_SAMPLE = 0, 1, 2, 3, 4, 255
COUNTS = ("n_samples", "n_pairs", "n_used", "n_outside", "n_grazing", "n_occluded", "n_buried", "n_dark", "n_texels_solved")


def check_params(bias, cos_min, shade_min):
    if not (np.isfinite(bias) and bias > 0 and np.isfinite(cos_min) and -1 <= cos_min < 1 and np.isfinite(shade_min) and shade_min > 0):
        raise ValueError("bias / cos_min / shade_min")


def project(xs, R, t, intr, w, h, T):
    """device_common.h project: p = R^T (xs - t), z_inv = 1 / p[2], (m, n) = (fx p[0] z_inv + cx, fy p[1] z_inv + cy), all in T"""
    fx, fy, cx, cy = (T(f32(x)) for x in intr)
    tmp = xs - t[None, :]
    p = np.stack([(R[0, i] * tmp[:, 0] + R[1, i] * tmp[:, 1]) + R[2, i] * tmp[:, 2] for i in range(3)], 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z_inv = T(1) / p[:, 2]
        m = fx * p[:, 0] * z_inv + cx
        n = fy * p[:, 1] * z_inv + cy
        ok = (m >= 0) & (m < T(w)) & (n >= 0) & (n < T(h))
    return p, m, n, ok


def shading(model, nf, p, R, light_f, T):
    """device_common.h rendered<MODEL> under albedo (1, 1, 1): [n, 3] in T.  nf: the stored float normals; light_f: the frame's light record"""
    one = T(1)
    if model == 2:
        Rp = np.stack([(R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2] for i in range(3)], 1)
        irr = -((nf[:, 0] * Rp[:, 0] + nf[:, 1] * Rp[:, 1]) + nf[:, 2] * Rp[:, 2])
        pn = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        pd = pn.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            irr = irr / (pd * pd * pd).astype(T)
        return np.stack([one * light_f[c] * irr for c in range(3)], 1)
    b = lref.sh_basis(nf, 9 if model == 1 else 4).astype(T) if T is f32 else _sh64(nf, model)
    irr = np.zeros(len(nf), T)
    for i in range(b.shape[1]):
        irr = irr + light_f[i] * b[:, i]
    return np.stack([one * irr] * 3, 1)


def _sh64(n, model):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    b = [np.ones_like(x), x, y, z]
    if model == 1:
        b += [x * y, x * z, y * z, x * x - y * y, x * x - z * z]
    return np.stack(b, 1)


def bilinear(img, m_col, n_row, T):
    """device_common.h sample_cell without a gradient: img [h, w, 3] in T; the last row / column: the nearest sample"""
    h, w = img.shape[:2]
    x = np.floor(n_row).astype(np.int64); y = np.floor(m_col).astype(np.int64)      # row, column
    cell = (x + 1 < h) & (y + 1 < w)
    xc, yc = np.clip(x, 0, h - 2), np.clip(y, 0, w - 2)
    fm, fn = (n_row - x.astype(T))[:, None], (m_col - y.astype(T))[:, None]
    one = T(1)
    w1, w2, w3, w4 = (one - fn) * fm, (one - fn) * (one - fm), fn * fm, fn * (one - fm)
    a00, a01, a10, a11 = img[xc, yc], img[xc, yc + 1], img[xc + 1, yc], img[xc + 1, yc + 1]
    I = ((a10 * w1 + a00 * w2) + a11 * w3) + a01 * w4
    return np.where(cell[:, None], I, img[np.clip(x, 0, h - 1), np.clip(y, 0, w - 1)]).astype(T)


def robust_weight(r, loss, lam, T):
    """device_common.h robust_weight: x = r * (1 / lambda)"""
    lam = T(f32(lam))
    inv = T(1) / lam
    x = r * inv
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == 1:
            return T(1) / (T(1) + x * x)
        if loss == 3:
            u = T(1) - x * x
            return np.where(r * r < lam * lam, u * u, T(0)).astype(T)
        if loss == 2:
            return np.where(r * r < lam * lam, T(1), lam * np.abs(T(1) / r)).astype(T)
        if loss == 4:
            return np.where(r * r < lam * lam, T(1), T(0)).astype(T)
    return np.ones_like(r)


def sample_points(mesh, planes, R, origin):
    """the samples of the definition: flat texel indices smp [S], q, m, n [S, 3] (mesh frame), nf [S, 3] float32 (the stored normals), a0 [S, 3], xw [S, 3]"""
    origin = np.asarray(origin, f32).astype(np.float64)
    face = np.asarray(planes["face"])
    H, W = face.shape
    L = bref.layout(len(mesh["faces"]), R)
    assert (L["H"], L["W"]) == (H, W) and np.array_equal(L["face"], face)
    smp = np.nonzero((face.ravel() >= 0) & (np.asarray(planes["voxel"]).ravel() >= 0))[0]
    _, p, n, ray = bref.sample(mesh["xyz"], mesh["normals"], mesh["faces"], face.ravel()[smp], L["a"].ravel()[smp], L["b"].ravel()[smp], R)
    assert ray.all()      # (a hit texel had a ray)
    d = np.asarray(planes["displacement"], f32).ravel()[smp].astype(np.float64)
    nf = np.asarray(planes["normal"], f32).reshape(-1, 3)[smp]
    mh, ok = oref.normalise(nf)
    q = p + d[:, None] * n
    m = np.where(ok[:, None], mh, n)
    a0 = np.asarray(planes["albedo"], np.uint8).reshape(-1, 3)[smp].astype(np.float64) / 255.0
    return smp, q, m, n, nf, a0, q + origin[None, :]


def photo(v, dim, vs, origin, mesh, planes, R, poses, light, images, intr, model, loss, lam, bias, cos_min=0.2, shade_min=0.05, mode="f32"):
    check_params(bias, cos_min, shade_min)
    T = {"f32": f32, "f64": np.float64}[mode]
    vs = float(f32(vs))
    origin = np.asarray(origin, f32).astype(np.float64)
    H, W = np.asarray(planes["face"]).shape
    images = np.asarray(images, f32)
    F, h, w = images.shape[:3]
    poses = np.asarray(poses, f32).reshape(F, 4, 4)
    light = np.asarray(light, f32)
    byte = np.asarray(planes["albedo"], np.uint8).reshape(-1, 3)
    smp, q, m, n, nf, a0, xw = sample_points(mesh, planes, R, origin)
    S = len(smp)
    xs = xw.astype(T)
    nfT = nf.astype(T)
    o = q + float(bias) * m
    status = np.full((F, H * W), NO_SAMPLE, np.uint8)
    num = np.zeros((S, 3)); den = np.zeros((S, 3)); n_obs = np.zeros(S, np.int64)
    n_buried = 0
    for f in range(F):
        Rf, tf = poses[f, :3, :3].astype(T), poses[f, :3, 3].astype(T)
        t64 = poses[f, :3, 3].astype(np.float64)
        st = np.full(S, USED, np.uint8)
        pc, mc, nr, inside = project(xs, Rf, tf, intr, w, h, T)
        outside = ~((pc[:, 2] > 0) & inside)
        with np.errstate(divide="ignore", invalid="ignore"):
            wc = t64[None, :] - xw
            wc = wc / np.sqrt((wc[:, 0] * wc[:, 0] + wc[:, 1] * wc[:, 1]) + wc[:, 2] * wc[:, 2])[:, None]
            cosv = lref.dot(m, wc)
        grazing = ~outside & ~(cosv > cos_min)
        st[outside] = OUTSIDE; st[grazing] = GRAZING
        r = np.nonzero(~outside & ~grazing)[0]
        dd = (t64 - origin)[None, :] - o[r]
        ln = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        can = ln > 0
        uo = o[r] / vs + 0.5
        uw = (dd / np.where(can, ln, 1.0)[:, None]) / vs
        if T is f32:
            uo, uw = uo.astype(f32), uw.astype(f32)
        occ = np.zeros(len(r), bool); bur = np.zeros(len(r), bool)
        if can.any():
            tt, _, ff = bref.walk(v["dist"], v["grad"], v["weight"], dim, vs, uo[can], uw[can])
            if T is f32:
                tt = tt.astype(f32).astype(np.float64)
            occ[can] = ff & (tt <= ln[can])
            bur[can] = occ[can] & (tt == 0)
        st[r[occ]] = OCCLUDED
        n_buried += int(bur.sum())
        r = r[~occ]
        lf = (light if model == 2 else light[f]).astype(T)
        sh = shading(model, nfT[r], pc[r], Rf, lf, T)
        dark = ~(sh >= T(shade_min)).all(1)
        st[r[dark]] = DARK
        r, sh = r[~dark], sh[~dark]
        I = bilinear(images[f].astype(T), mc[r], nr[r], T)
        res = I - a0[r].astype(T) * sh
        wgt = robust_weight(res, loss, lam, T)
        num[r] += (wgt.astype(np.float64) * sh.astype(np.float64)) * I.astype(np.float64)
        den[r] += (wgt.astype(np.float64) * sh.astype(np.float64)) * sh.astype(np.float64)
        n_obs[r] += 1
        status[f, smp] = st
    with np.errstate(divide="ignore", invalid="ignore"):
        solved = np.where((n_obs > 0)[:, None] & (den > 0), (num / den).astype(f32), a0.astype(f32)).astype(f32)
    ph = (byte.astype(np.float64) / 255.0).astype(f32)
    ph[smp] = solved
    rgb = byte.copy()
    rgb[smp] = bref.colour_byte(solved)
    nobs = np.zeros(H * W, np.int32); nobs[smp] = n_obs
    xwp = np.zeros((H * W, 3)); xwp[smp] = xw
    ss = status[:, smp]
    counts = dict(n_samples=S, n_pairs=S * F, n_used=int((ss == USED).sum()), n_outside=int((ss == OUTSIDE).sum()), n_grazing=int((ss == GRAZING).sum()),
                  n_occluded=int((ss == OCCLUDED).sum()), n_buried=n_buried, n_dark=int((ss == DARK).sum()), n_texels_solved=int((n_obs > 0).sum()))
    return dict(photo=ph.reshape(H, W, 3), photo_rgb=rgb.reshape(H, W, 3), n_obs=nobs.reshape(H, W), status=status.reshape(F, H, W), counts=counts,
                xw=xwp.reshape(H, W, 3), sample=np.isin(np.arange(H * W), smp).reshape(H, W))


def compare_modes(a, b):
    """two results on the same inputs: (share of pairs whose status differs, E = max |photo_a - photo_b| over the texels whose statuses all agree, that mask)"""
    sa, sb = a["status"], b["status"]
    smp = a["sample"]
    pairs = max(int(smp.sum()) * sa.shape[0], 1)
    differ = (sa != sb)
    agree = smp & ~differ.any(0)
    E = float(np.abs(a["photo"][agree].astype(np.float64) - b["photo"][agree].astype(np.float64)).max()) if agree.any() else 0.0
    return differ.sum() / pairs, E, agree


def gain_rms(x, truth):
    """rms of g x - truth per channel, with the least-squares gain g of each channel (albedo and light share a scale); x, truth [n, 3]"""
    x, truth = np.asarray(x, np.float64), np.asarray(truth, np.float64)
    g = (x * truth).sum(0) / (x * x).sum(0)
    return float(np.sqrt(((g[None, :] * x - truth) ** 2).mean()))
