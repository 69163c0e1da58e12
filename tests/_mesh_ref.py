"""numpy restatement of the welded mesh (include/psgsdf_mesh.h, DESIGN.md "Welded meshes"): float32 where the kernels compute in float, the
interpolation's double step in float64.  It is the yardstick of tests/test_mesh_indexed_gpu.py and of the CPU topology checks.

    mesh(v, dim, vs)             -> (xyz, normals, rgb, faces, first_vertex) of one context
    mesh(v, dim, vs, cuts=[...]) -> one such tuple per z-slab (cuts: the slabs' first planes, then the volume's depth), with the ownership rule
                                    (a cell: the slab of its lower plane; a key: the slab of its voxel's plane) and global face indices
v: dist [n], grad [3, n], weight [n], rgb [3, n] (x fastest, the layout of Api.download_volume); dim = (nx, ny, nz)."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
TRI = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_tritable.npy")).astype(np.int64)
CORNER = np.array([[1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 1, 1]])
EDGE = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4], [0, 4], [1, 5], [2, 6], [3, 7]])


def crop_box(dist, dim, vs):
    """min / max voxel index over |d| <= sqrt(3) vs (the comparison in double); None if no voxel qualifies"""
    m = np.abs(dist.reshape(dim[2], dim[1], dim[0])).astype(f64) <= np.sqrt(3.0) * float(f32(vs))
    if not m.any():
        return None
    idx = [np.nonzero(m.any(axis=ax))[0] for ax in ((0, 1), (0, 2), (1, 2))]      # x, y, z
    return np.array([i[0] for i in idx]), np.array([i[-1] for i in idx])


def frame(lo, d, vs):
    """psgsdf_extract_mesh's vertex frame: voxel = (vs d) / d, origin = -vs lo, in float32"""
    vs = f32(vs)
    voxel = np.array([(vs * f32(d[a])) / f32(d[a]) for a in range(3)], f32)
    origin = np.array([f32(-vs) * f32(lo[a]) for a in range(3)], f32)
    return voxel, origin


def unit(g):
    """normalised stored gradient [3, m] (a zero gradient stays zero), float32 in the kernel's order"""
    g = g.astype(f32)
    z = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    ok = z > 0
    s = np.sqrt(np.where(ok, z, f32(1)), dtype=f32)
    return np.where(ok, g / s, g).astype(f32)


def _empty(cuts):
    e = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32), 0)
    return [e] * (len(cuts) - 1) if cuts is not None else e


def mesh(v, dim, vs, cuts=None):
    nx, ny, nz = (int(x) for x in dim)
    dist = np.asarray(v["dist"], f32).reshape(nz, ny, nx)
    box = crop_box(dist, dim, vs)
    if box is None:
        return _empty(cuts)
    lo, hi = box
    d = hi - lo + 1
    if (d < 3).any():
        return _empty(cuts)
    voxel, origin = frame(lo, d, vs)
    sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    t = (-dist)[sl]
    w = np.asarray(v["weight"], f32).reshape(nz, ny, nx)[sl]
    cz, cy, cx = d[2] - 2, d[1] - 2, d[0] - 2
    corner = lambda a, c: a[CORNER[c][2]:CORNER[c][2] + cz, CORNER[c][1]:CORNER[c][1] + cy, CORNER[c][0]:CORNER[c][0] + cx]
    valid = np.ones((cz, cy, cx), bool)
    cs = np.zeros((cz, cy, cx), np.int64)
    for c in range(8):
        valid &= corner(w, c) != 0
        cs |= (corner(t, c) > 0).astype(np.int64) << c
    act = valid & (cs != 0) & (cs != 255)
    z, y, x = np.nonzero(act)                     # (z, y, x) order: the cells' order
    cs = cs[act]
    base = np.stack([x, y, z], 1)                 # cropped cell coordinates [A, 3]
    gkey = lambda p, typ: 4 * (((p[:, 2] + lo[2]) * ny + (p[:, 1] + lo[1])) * nx + (p[:, 0] + lo[0])).astype(np.int64) + typ
    tv = lambda p: t[p[:, 2], p[:, 1], p[:, 0]]
    keys = np.zeros((len(cs), 12), np.int64)
    for e in range(12):
        a, b = EDGE[e]
        ax = int(np.nonzero(CORNER[a] != CORNER[b])[0][0])
        l, h = (a, b) if CORNER[a][ax] < CORNER[b][ax] else (b, a)
        pl, ph = base + CORNER[l], base + CORNER[h]
        tl, th = tv(pl), tv(ph)
        snap_l = np.abs(f32(0) - tl).astype(f64) < 1e-7
        snap_h = ~snap_l & (np.abs(f32(0) - th).astype(f64) < 1e-7)
        snap_l |= ~snap_h & (np.abs(tl - th).astype(f64) < 1e-7)
        keys[:, e] = np.where(snap_l, gkey(pl, 3), np.where(snap_h, gkey(ph, 3), gkey(pl, ax)))
    fk, kept = np.zeros((len(cs), 5, 3), np.int64), np.zeros((len(cs), 5), bool)
    for q in range(5):
        e = TRI[cs, 3 * q:3 * q + 3]
        have = e[:, 0] >= 0
        k = np.take_along_axis(keys, np.maximum(e, 0), 1)
        fk[:, q] = k
        kept[:, q] = have & (k[:, 0] != k[:, 1]) & (k[:, 0] != k[:, 2]) & (k[:, 1] != k[:, 2])
    face_keys = fk[kept]                                           # [F, 3] in cell / table order
    face_z = np.repeat(z, kept.sum(1)) + lo[2]                     # global lower plane of each face's cell
    vkeys = np.unique(face_keys)
    faces = np.searchsorted(vkeys, face_keys).astype(np.int32)
    xyz, nrm, rgb = vertices(v, dim, vkeys, lo, voxel, origin)
    if cuts is None:
        return xyz, nrm, rgb, faces, 0
    vz = (vkeys >> 2) // (nx * ny)
    out = []
    for r in range(len(cuts) - 1):
        fm = (face_z >= cuts[r]) & (face_z < cuts[r + 1])
        vm = (vz >= cuts[r]) & (vz < cuts[r + 1])
        first = int(np.count_nonzero(vz < cuts[r]))
        out.append((xyz[vm], nrm[vm], rgb[vm], faces[fm], first))
    return out


def vertices(v, dim, vkeys, lo, voxel, origin):
    nx, ny, nz = (int(x) for x in dim)
    dist, grad, rho = np.asarray(v["dist"], f32), np.asarray(v["grad"], f32).reshape(3, -1), np.asarray(v["rgb"], f32).reshape(3, -1)
    typ, lin = vkeys & 3, vkeys >> 2
    k, rest = np.divmod(lin, nx * ny)
    j, i = np.divmod(rest, nx)
    p = np.stack([i, j, k], 1)
    corner = typ == 3
    step = np.zeros((len(vkeys), 3), np.int64)
    step[~corner, typ[~corner]] = 1
    ph = p + step
    linh = (ph[:, 2] * ny + ph[:, 1]) * nx + ph[:, 0]
    pos = lambda q: np.stack([(q[:, a] - lo[a]).astype(f32) * voxel[a] - origin[a] for a in range(3)], 1).astype(f32)
    pl, pu = pos(p), pos(ph)
    tl, th = -dist[lin], -dist[linh]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = ((f32(0) - tl) / (th - tl)).astype(f32).astype(f64)
    mu = np.where(corner, 0.0, np.clip(mu, 0.0, 1.0))
    xyz = (pl.astype(f64) + mu[:, None] * (pu - pl).astype(f64)).astype(f32)
    xyz[corner] = pl[corner]
    m = mu.astype(f32)[None, :]
    gl, gh = unit(grad[:, lin]), unit(grad[:, linh])
    n = (gl + m * (gh - gl)).astype(f32)
    n = np.where(corner[None, :], gl, unit(n))
    c = (rho[:, lin] + m * (rho[:, linh] - rho[:, lin])).astype(f32)
    c = np.where(corner[None, :], rho[:, lin], c)
    rgb = np.floor(f32(255) * np.clip(c, f32(0), f32(1)) + f32(0.5)).astype(np.uint8)
    return xyz, n.T.copy(), rgb.T.copy()


def edges(faces):
    """directed edges [3F, 2] of the faces"""
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def topology(faces, nv):
    """(closed and oriented, Euler characteristic V - E + F, boundary edges [B, 2] (undirected, used once), edges used more than twice)"""
    de = edges(faces).astype(np.int64)
    und = np.sort(de, 1)
    u, cnt = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    dk, dcnt = np.unique(de[:, 0] * nv + de[:, 1], return_counts=True)
    closed = bool((cnt == 2).all() and (dcnt == 1).all())
    b = u[cnt == 1]
    return closed, nv - len(u) + len(faces), np.stack([b // nv, b % nv], 1), int((cnt > 2).sum())
