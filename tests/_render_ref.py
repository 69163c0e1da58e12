"""Plain numpy restatement of the view renderer's traversal (include/psgsdf_render.h), in float64 and without the brick map:
a DDA over the nearest-voxel cells of the whole grid, hit = first ray parameter with phi_v(p) = d_v + g_v.(p - x_v) <= 0 inside an observed cell.
Shared by tests/test_render_cpu.py and tests/test_render_gpu.py."""
import numpy as np


def trace(dist, grad, weight, dim, vs, origin, pose, fx, fy, cx, cy, W, H):
    """dist / weight [nvox], grad [3, nvox] (x-fastest), pose 4x4 camera->world.  Returns (depth [H, W] camera z, 0 on a miss; voxel [H, W], -1 on a miss)."""
    dim = np.asarray(dim, np.int64)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, tc = P[:3, :3], P[:3, 3]
    origin = np.asarray(origin, np.float64)
    vs = float(vs)
    ys, xs = np.mgrid[0:H, 0:W]
    dc = np.stack([(xs.ravel() - cx) / fx, (ys.ravel() - cy) / fy, np.ones(W * H)], 1)
    uw = (dc @ R.T) / vs
    uo = (tc - origin) / vs + 0.5
    n = W * H
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(uw != 0, 1.0 / uw, 0.0)
        ta = (0.0 - uo) * inv
        tb = (dim[None, :] - uo) * inv
    inside = (uo >= 0) & (uo < dim)
    lo_t = np.where(uw != 0, np.minimum(ta, tb), -np.inf)
    hi_t = np.where(uw != 0, np.maximum(ta, tb), np.where(inside[None, :], np.inf, -np.inf))
    t0 = np.maximum(0.0, lo_t.max(1))
    t1 = hi_t.min(1)
    step = np.sign(uw).astype(np.int64)
    c = np.clip(np.floor(uo + t0[:, None] * uw).astype(np.int64), 0, dim - 1)
    t = t0.copy()
    active = t0 < t1
    depth = np.zeros(n)
    vox = np.full(n, -1, np.int64)
    g = grad.astype(np.float64)
    d64 = dist.astype(np.float64)
    w64 = weight
    for _ in range(int(dim.sum()) + 8):
        a = np.nonzero(active)[0]
        if len(a) == 0:
            break
        ca, ua, sa, ia, ta_ = c[a], uw[a], step[a], inv[a], t[a]
        bound = ca + (sa > 0)
        with np.errstate(invalid="ignore"):
            tt = np.where(sa != 0, (bound - uo) * ia, np.inf)
        ax = tt.argmin(1)
        te = tt[np.arange(len(a)), ax]
        lin = ca[:, 0] + ca[:, 1] * dim[0] + ca[:, 2] * dim[0] * dim[1]
        obs = w64[lin] > 0
        gr = g[:, lin].T
        nrm = np.linalg.norm(gr, axis=1)
        gn = np.where(nrm[:, None] > 0, gr / np.where(nrm > 0, nrm, 1.0)[:, None], gr)
        loc = (uo + ta_[:, None] * ua) - (ca + 0.5)
        phi0 = d64[lin] + vs * (gn * loc).sum(1)
        s = vs * (gn * ua).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            th = ta_ - phi0 / s
        h0 = obs & (phi0 <= 0)
        h1 = obs & ~h0 & (s < 0) & (th <= te)
        hit = h0 | h1
        depth[a[h0]] = ta_[h0]
        depth[a[h1]] = th[h1]
        vox[a[hit]] = lin[hit]
        active[a[hit]] = False
        rest = ~hit
        ar, axr = a[rest], ax[rest]
        c[ar, axr] += step[ar, axr]
        out = (c[ar, axr] < 0) | (c[ar, axr] >= dim[axr])
        active[ar[out]] = False
        t[ar] = np.maximum(t[ar], te[rest])
    return depth.reshape(H, W), vox.reshape(H, W)


def plane_volume(N=48, vs=0.01, normal=(0.25, -0.35, 0.9), offset=0.004, band=3.0):
    """A tilted plane n.x = offset through the grid centre region: d = n.x - offset (exact for the first-order model), grad = n, weight 1 where
    |d| < band * vs.  Returns (dim, origin, dist, grad, weight, n)."""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    dim = np.array([N, N, N], np.int32)
    origin = -0.5 * vs * dim.astype(np.float64)
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    x = origin + vs * np.stack([i, j, k], -1).reshape(-1, 3)
    d = x @ n - offset
    dist = np.clip(d, -band * vs, band * vs).astype(np.float32)
    grad = np.repeat(n.astype(np.float32)[:, None], N ** 3, 1)
    weight = (np.abs(d) < band * vs).astype(np.float32)
    return dim, origin, dist, np.ascontiguousarray(grad), weight, n


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4x4 camera->world pose looking from eye at target (camera z forward, y down)."""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def plane_depth(n, offset, pose, fx, fy, cx, cy, W, H):
    """analytic camera z of the plane n.x = offset along every pixel's ray"""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    dc = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], -1)
    w = dc @ P[:3, :3].T
    return (offset - n @ P[:3, 3]) / (w @ n)
