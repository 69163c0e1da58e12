"""Yardstick of the relighting call (include/psgsdf_relight.h psgsdf_relight), in numpy float64, written from the definition: the hit
point of every pixel from the geometry planes, the centre direction, cosine and fall-off of each light, the shadow rays set up in double and rounded
to float32 exactly as the definition says, and the renderer's walk as tests/_bake_ref.py restates it (float64, no brick map, NO cut at the limit:
the device's cut must not change a bit).  Shared by tests/test_relight_cpu.py and tests/test_relight_gpu.py.

    table(K)                      -> (a, b) [K, 2]: the first two components of the occlusion's direction table; K = 1: (0, 0)
    geometry(v, dim, vs, origin, pose, intr, W, H) -> the planes depth, normal, albedo, voxel of tests/_render_ref.py trace() (off-band values)
    relight(v, dim, vs, origin, pose, intr, geo, lights, bias, reach) -> one dict per light
v: dict of dist [n], grad [3, n], weight [n], rgb [3, n] (x fastest).  pose: 4x4 camera->world float32; intr = (fx, fy, cx, cy).
geo: dict of depth [H, W] float32, normal [3, H, W] float32, albedo [3, H, W] float32, voxel [H, W] int32 -- the device's own, or geometry()'s.
lights: dicts as psgradientsdf_amd.capi.make_light takes them (kind, sh, vec, colour, ambient, spread, samples)."""
import numpy as np

import _bake_ref as bref
import _occlusion_ref as oref
import _render_ref as rref

f32 = np.float32
KS = (1, 8, 16, 32, 64)
COUNTS = ("n_hits", "n_lit", "n_rays", "n_occluded", "n_buried")


def table(K):
    K = int(K)
    if K not in KS:
        raise ValueError("samples")
    return np.zeros((1, 2)) if K == 1 else oref.dirs(K)[:, :2].copy()


def unit(v):
    """v / sqrt((v0^2 + v1^2) + v2^2) along the last axis; ok: the length is > 0"""
    v = np.asarray(v, np.float64)
    ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    ok = ln > 0
    return np.where(ok[..., None], v / np.where(ok, ln, 1.0)[..., None], v), ok, ln


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pixel_rays(pose, intr, W, H):
    """the renderer's float32 ray direction of every pixel [H, W, 3] (w = R dc) and the camera centre [3], widened"""
    P = np.asarray(pose, f32).reshape(4, 4)
    fx, fy, cx, cy = (f32(x) for x in intr)
    ys, xs = np.mgrid[0:H, 0:W]
    dc = np.stack([(xs.astype(f32) - cx) / fx, (ys.astype(f32) - cy) / fy, np.ones((H, W), f32)], -1).astype(f32)
    R = P[:3, :3]
    w = np.stack([(R[i, 0] * dc[..., 0] + R[i, 1] * dc[..., 1]) + R[i, 2] * dc[..., 2] for i in range(3)], -1).astype(f32)
    return w.astype(np.float64), P[:3, 3].astype(np.float64)


def geometry(v, dim, vs, origin, pose, intr, W, H):
    fx, fy, cx, cy = (float(f32(x)) for x in intr)
    depth, vox = rref.trace(v["dist"], v["grad"], v["weight"], dim, float(f32(vs)), origin, np.asarray(pose, f32).astype(np.float64), fx, fy, cx, cy, W, H)
    hit = vox >= 0
    normal = np.zeros((3, H, W), f32); albedo = np.zeros((3, H, W), f32)
    normal[:, hit] = bref.unit_f32(np.asarray(v["grad"], f32)[:, vox[hit]].T).T
    albedo[:, hit] = np.asarray(v["rgb"], f32)[:, vox[hit]]
    return dict(depth=np.where(hit, depth, 0).astype(f32), normal=normal, albedo=albedo, voxel=vox.astype(np.int32))


def sh_basis(n, n_sh):
    """device_common.h SH<NB> on float32 normals [..., 3]"""
    n = np.asarray(n, f32)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    b = [np.ones_like(x), x, y, z]
    if n_sh == 9:
        b += [x * y, x * z, y * z, x * x - y * y, x * x - z * z]
    return np.stack(b, -1).astype(f32)


def check_light(L):
    kind = L["kind"]
    K = int(L.get("samples", 0 if kind == "sh" else 1))
    spread = float(f32(L.get("spread", 0.0)))
    for k in ("colour", "ambient"):
        c = np.broadcast_to(np.asarray(L.get(k, 1.0 if k == "colour" else 0.0), f32), (3,))
        if not (np.isfinite(c).all() and (c >= 0).all()):
            raise ValueError(k)
    if not (np.isfinite(spread) and spread >= 0):
        raise ValueError("spread")
    if kind == "sh":
        if len(L["sh"]) not in (4, 9) or K != 0 or spread != 0 or not np.isfinite(np.asarray(L["sh"], f32)).all():
            raise ValueError("sh")
        return 0, spread
    if kind not in ("directional", "point"):
        raise ValueError("kind")
    vec = np.asarray(L["vec"], f32)
    if not np.isfinite(vec).all() or (kind == "directional" and not vec.any()):
        raise ValueError("vec")
    if K not in KS or (spread > 0 and K < 8):
        raise ValueError("samples")
    return K, spread


def check_params(bias, reach, n_lights):
    if not (np.isfinite(bias) and bias > 0 and np.isfinite(reach) and reach >= 0 and 1 <= n_lights <= 64):
        raise ValueError("bias / reach / n_lights")


def relight(v, dim, vs, origin, pose, intr, geo, lights, bias, reach):
    check_params(bias, reach, len(lights))
    vs = float(f32(vs))
    origin = np.asarray(origin, f32).astype(np.float64)
    depth = np.asarray(geo["depth"], f32); voxel = np.asarray(geo["voxel"])
    H, W = depth.shape
    hit = voxel >= 0
    nrm = np.moveaxis(np.asarray(geo["normal"], f32), 0, -1)            # [H, W, 3]
    rho = np.moveaxis(np.asarray(geo["albedo"], f32), 0, -1).astype(np.float64)
    w, tc = pixel_rays(pose, intr, W, H)
    q = tc[None, None, :] + depth.astype(np.float64)[..., None] * w
    m, has_normal, _ = unit(nrm.astype(np.float64))
    limit_all = float(reach) if reach > 0 else np.inf
    out = []
    for L in lights:
        K, spread = check_light(L)
        colour = np.broadcast_to(np.asarray(L.get("colour", 1.0), f32), (3,)).astype(np.float64)
        ambient = np.broadcast_to(np.asarray(L.get("ambient", 0.0), f32), (3,)).astype(np.float64)
        if L["kind"] == "sh":
            sh = np.asarray(L["sh"], f32)
            b = sh_basis(nrm, len(sh))
            irr = np.zeros((H, W), f32)
            for i in range(len(sh)):
                irr = (irr + sh[i] * b[..., i]).astype(f32)
            vis = hit.astype(f32)
            s = irr.astype(np.float64)
            ren = np.where(hit[..., None], rho * (ambient + colour * s[..., None]), 0.0).astype(f32)
            out.append(dict(visibility=vis, rendered=np.moveaxis(ren, -1, 0), lit=hit.copy(), K=0, n_hits=int(hit.sum()), n_lit=int(hit.sum()), n_rays=0, n_occluded=0, n_buried=0))
            continue
        vec = np.asarray(L["vec"], f32).astype(np.float64)
        if L["kind"] == "directional":
            wc = np.broadcast_to(unit(vec)[0], (H, W, 3)); reachable = np.ones((H, W), bool); fall = np.ones((H, W))
        else:
            d = vec[None, None, :] - q
            r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            wc, reachable, _ = unit(d)
            with np.errstate(divide="ignore"):
                fall = 1.0 / r2
        cosv = dot(m, wc)
        lit = hit & has_normal & reachable & (cosv > 0)
        idx = np.nonzero(lit.ravel())[0]
        n = len(idx)
        ab = table(K)
        mm, wcl, ql = m.reshape(-1, 3)[idx], wc.reshape(-1, 3)[idx], q.reshape(-1, 3)[idx]
        t1, t2 = oref.frame(wcl)
        o = ql + float(bias) * mm
        e = ab[None, :, 0, None] * t1[:, None, :] + ab[None, :, 1, None] * t2[:, None, :]      # [n, K, 3]
        if L["kind"] == "directional":
            dd = wcl[:, None, :] + spread * e
        else:
            dd = (vec[None, None, :] + spread * e) - o[:, None, :]
        wi, ok, ln = unit(dd)
        limit = np.minimum(limit_all, ln) if L["kind"] == "point" else np.full((n, K), limit_all)
        uo = ((o - origin[None, :]) / vs + 0.5).astype(f32)
        uw = (wi / vs).astype(f32)
        t = np.zeros((n, K)); found = np.zeros((n, K), bool)
        if n:
            tt, _, ff = bref.walk(v["dist"], v["grad"], v["weight"], dim, vs, np.broadcast_to(uo[:, None, :], uw.shape).reshape(-1, 3), uw.reshape(-1, 3))
            t = tt.reshape(n, K).astype(f32).astype(np.float64); found = ff.reshape(n, K) & ok
        occ = found & (t <= limit)
        bur = occ & (t == 0)
        c = occ.sum(1)
        vis = np.zeros(H * W, f32)
        vis[idx] = (K - c).astype(f32) / f32(K)
        vis = vis.reshape(H, W)
        s = np.where(lit, (cosv * fall) * vis.astype(np.float64), 0.0)
        ren = np.where(hit[..., None], rho * (ambient + colour * s[..., None]), 0.0).astype(f32)

        def per_pixel(x, fill, dt):
            full = np.full((H * W,) + x.shape[1:], fill, dt)
            full[idx] = x
            return full.reshape((H, W) + x.shape[1:])
        out.append(dict(visibility=vis, rendered=np.moveaxis(ren, -1, 0), lit=lit, K=K, cosv=cosv, fall=fall,
                        bits=per_pixel(occ, False, bool), buried=per_pixel(bur, False, bool), t=per_pixel(t, 0.0, np.float64), found=per_pixel(found, False, bool),
                        limit=per_pixel(limit, np.inf, np.float64), o=per_pixel(o, 0.0, np.float64), w=per_pixel(wi, 0.0, np.float64), count=per_pixel(c, 0, np.int64),
                        n_hits=int(hit.sum()), n_lit=n, n_rays=K * n, n_occluded=int(occ.sum()), n_buried=int(bur.sum())))
    return out
