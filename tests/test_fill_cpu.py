"""The hole filling's definition (include/psgsdf_fill.h, DESIGN.md "Hole filling") as restated in tests/_fill_ref.py, without a GPU: the restatement
against a voxel-by-voxel transcription of the header, the hand-computed cases the device test repeats, and what the filling does to the welded mesh of
the bumpy sphere with a hole (tests/test_mesh_indexed_gpu.py analytic_engine): boundary edges, Euler characteristic, winding, distance to the surface."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _fill_ref as fref
import _mesh_ref as mref
from psgradientsdf_amd import synth
from test_mesh_indexed_cpu import read_ply_indexed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
f32 = np.float32
VS = 0.01


def read_ply_filled(path):
    """(header lines, vertex records, faces) of `voxelPS --mesh-fill`'s file: the welded mesh's records with `filled` behind the colours"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("filled", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize and vt.itemsize == 28
    props = [h for h in head if h.startswith("property")]
    assert props[9:] == ["property uchar filled", "property list uchar int vertex_indices"]
    verts = np.frombuffer(raw, vt, nv, end)
    fc = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (fc["n"] == 3).all()
    return head, verts, fc["v"].copy()


def fill_comment(head):
    """{rounds, sweeps, voxels, before, after} of the file's `comment fill` line"""
    w = next(h for h in head if h.startswith("comment fill ")).split()
    assert w[2:9:2] == ["rounds", "sweeps", "voxels", "boundary_edges"] and len(w) == 11, w
    return dict(rounds=int(w[3]), sweeps=int(w[5]), voxels=int(w[7]), before=int(w[9]), after=int(w[10]))


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_selftest_ply_filled_parses_back(tmp_path):
    """`voxelPS --selftest-ply-filled`: the octahedron of --selftest-ply-indexed with `filled` behind the colours, through the one writer of the welded mesh"""
    out, plain = str(tmp_path / "octa_filled.ply"), str(tmp_path / "octa.ply")
    for flag, path in (("--selftest-ply-filled", out), ("--selftest-ply-indexed", plain)):
        r = subprocess.run([EXE, flag, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
    head, verts, faces = read_ply_filled(out)      # (asserts the property lines, the 28-byte records and the file's length)
    phead, pverts, pfaces = read_ply_indexed(plain)
    assert len(verts) == 6 and np.array_equal(faces, pfaces) and len(faces) == 8
    assert verts.dtype.itemsize == 28 and pverts.dtype.itemsize == 27
    assert [bytes(v.tobytes()[:27]) for v in verts] == [bytes(v.tobytes()) for v in pverts]
    for k in pverts.dtype.names:
        assert np.array_equal(verts[k], pverts[k]), k
    assert verts["filled"].tolist() == [0, 1, 2, 0, 2, 1]
    assert fill_comment(head) == dict(rounds=3, sweeps=4, voxels=17, before=12, after=0)
    assert [h for h in head if not h.startswith(("comment fill", "property"))] == [h for h in phead if not h.startswith("property")]
    assert [h for h in head if h.startswith("property")] == [h for h in phead if h.startswith("property")][:9] + ["property uchar filled", "property list uchar int vertex_indices"]


def volume(dim, observed, dist=None, grad=None, rgb=None, seed=0):
    """a small volume: random values everywhere (what an unobserved voxel holds must not matter), weight 1 at the voxels of `observed`"""
    n = int(np.prod(dim))
    rng = np.random.default_rng(seed)
    v = dict(dist=rng.normal(0, VS, n).astype(f32), grad=rng.normal(0, 1, (3, n)).astype(f32), weight=np.zeros(n, f32), rgb=rng.uniform(0, 1, (3, n)).astype(f32))
    v["weight"][np.asarray(observed, np.int64)] = 1
    for name, a in (("dist", dist), ("grad", grad), ("rgb", rgb)):
        if a is not None:
            for q, x in a.items():
                v[name][..., q] = x
    return v


def fill_by_the_letter(v, dim, vs, R, K):
    """include/psgsdf_fill.h voxel by voxel, in Python floats (IEEE double): (round [n], dist [n], grad [3, n], rgb [3, n]) of the filled state"""
    nx, ny, nz = dim
    h = float(f32(vs))
    n = nx * ny * nz
    dist, grad, rgb = v["dist"].copy(), v["grad"].copy(), v["rgb"].copy()
    rnd = np.zeros(n, np.int64)
    observed = v["weight"] > 0
    known = observed.copy()

    def unit(g):
        gx, gy, gz = float(g[0]), float(g[1]), float(g[2])
        z = (gx * gx + gy * gy) + gz * gz
        return (gx / math.sqrt(z), gy / math.sqrt(z), gz / math.sqrt(z)) if z > 0 else (0.0, 0.0, 0.0)

    def neighbours(u):
        i, j, k = u % nx, (u // nx) % ny, u // (nx * ny)
        for a, s in fref.NEIGHBOURS:
            p = [i, j, k]; p[a] += s
            if 0 <= p[0] < nx and 0 <= p[1] < ny and 0 <= p[2] < nz:
                yield a, s, (p[2] * ny + p[1]) * nx + p[0]

    def gather(u, kn, d, g, c, extend):
        sd, sm, sc, cnt = 0.0, [0.0] * 3, [0.0] * 3, 0
        for a, s, w in neighbours(u):
            if not kn[w]:
                continue
            m = unit(g[:, w])
            sd = sd + (float(d[w]) - (s * h) * m[a] if extend else float(d[w]))
            for q in range(3):
                sm[q] = sm[q] + m[q]; sc[q] = sc[q] + float(c[q, w])
            cnt += 1
        if cnt == 0:
            return None
        z = (sm[0] * sm[0] + sm[1] * sm[1]) + sm[2] * sm[2]
        gm = [x / math.sqrt(z) for x in sm] if z > 0 else [0.0] * 3
        return f32(sd / cnt), f32(gm), f32([x / cnt for x in sc])

    for r in range(1, R + 1):
        new = {}
        for u in range(n):
            if not known[u]:
                got = gather(u, known, dist, grad, rgb, True)
                if got is not None:
                    new[u] = got
        for u, (d, g, c) in new.items():
            dist[u], grad[:, u], rgb[:, u], rnd[u], known[u] = d, g, c, r, True
    filled = np.nonzero(known & ~observed)[0]
    for _ in range(K):
        new = {u: gather(u, known, dist, grad, rgb, False) for u in filled}
        for u, (d, g, c) in new.items():
            dist[u], grad[:, u], rgb[:, u] = d, g, c
    return rnd, dist, grad, rgb


@pytest.mark.parametrize("dim,R,K", [((5, 5, 5), 1, 0), ((5, 5, 5), 3, 2), ((5, 5, 9), 2, 1), ((4, 3, 6), 255, 3)])
def test_restatement_is_the_header_voxel_by_voxel(dim, R, K):
    n = int(np.prod(dim))
    rng = np.random.default_rng(7)
    observed = rng.choice(n, 6, replace=False)
    v = volume(dim, observed, seed=3)
    v["grad"][:, observed[0]] = 0      # one observed voxel without a gradient
    got = fref.fill(v, dim, VS, R, K)
    rnd, dist, grad, rgb = fill_by_the_letter(v, dim, VS, R, K)
    lin = np.nonzero(rnd)[0]
    assert np.array_equal(got["lin"], lin) and np.array_equal(got["round"], rnd[lin]) and len(lin) > 20
    assert got["dist"].tobytes() == dist[lin].tobytes() and got["grad"].tobytes() == grad[:, lin].T.copy().tobytes() and got["rgb"].tobytes() == rgb[:, lin].T.copy().tobytes()
    vol = got["volume"]
    rest = np.ones(n, bool); rest[lin] = False      # every other voxel is bit for bit as before
    for k in ("dist", "grad", "weight", "rgb"):
        assert vol[k][..., rest].tobytes() == v[k][..., rest].tobytes(), k
    assert (vol["weight"][lin] == 1).all()
    assert np.array_equal(got["round"], fref.manhattan(v["weight"], dim, R)[lin])


def test_hand_computed_cases():
    dim = (5, 5, 5)
    at = lambda i, j, k: (k * 5 + j) * 5 + i
    # one observed voxel at the grid corner, R = 3: the round is the city-block distance, nothing wraps around a face of the grid
    r = fref.fill(volume(dim, [at(0, 0, 0)]), dim, VS, 3, 0)
    i, j, k = r["lin"] % 5, (r["lin"] // 5) % 5, r["lin"] // 25
    assert np.array_equal(r["round"], i + j + k) and len(r["lin"]) == 4 + 6 + 10 - 1 and (i + j + k).max() == 3
    # two observed voxels three apart along x: a = (0, 2, 2) with d = 1 vs and gradient +x, b = (3, 2, 2) with d = 5 vs and gradient -x
    a, b = at(0, 2, 2), at(3, 2, 2)
    v = volume(dim, [a, b], dist={a: f32(VS), b: f32(5 * VS)}, grad={a: f32([2, 0, 0]), b: f32([-3, 0, 0])}, rgb={a: f32([0, 0.25, 1]), b: f32([1, 0.75, 0])})
    h = float(f32(VS)); da, db = float(f32(VS)), float(f32(5 * VS))
    r = fref.fill(v, dim, VS, 2, 0)
    val = {int(l): (d, g, c, q) for l, d, g, c, q in zip(r["lin"], r["dist"], r["grad"], r["rgb"], r["round"])}
    # round 1: (1, 2, 2) from a alone, (2, 2, 2) from b alone -- although each has the other as a neighbour by the end of the round
    assert val[at(1, 2, 2)][3] == 1 and val[at(1, 2, 2)][0] == f32(da - (-h) * 1.0) and np.array_equal(val[at(1, 2, 2)][1], f32([1, 0, 0])) and np.array_equal(val[at(1, 2, 2)][2], f32([0, 0.25, 1]))
    assert val[at(2, 2, 2)][3] == 1 and val[at(2, 2, 2)][0] == f32(db - h * -1.0) and np.array_equal(val[at(2, 2, 2)][1], f32([-1, 0, 0])) and np.array_equal(val[at(2, 2, 2)][2], f32([1, 0.75, 0]))
    assert val[at(4, 2, 2)][3] == 1 and val[at(4, 2, 2)][0] == f32(db - (-h) * -1.0)
    # round 2: (1, 3, 2) is reached from (1, 2, 2) and from (0, 3, 2), both filled in round 1 from a: it takes both, in the order -x, then -y
    d1, d0 = float(val[at(1, 2, 2)][0]), float(val[at(0, 3, 2)][0])
    assert val[at(1, 3, 2)][3] == 2 and val[at(1, 3, 2)][0] == f32(((d0 - (-h) * 1.0) + (d1 - (-h) * 0.0)) / 2)
    # K = 1: (1, 2, 2) becomes the mean of its six neighbours' distances of BEFORE the sweep ((2, 2, 2) among them), a stays
    r1 = fref.fill(v, dim, VS, 2, 1)
    nb = [at(0, 2, 2), at(2, 2, 2), at(1, 1, 2), at(1, 3, 2), at(1, 2, 1), at(1, 2, 3)]
    before = dict(val); before[a] = (f32(VS),)
    s = 0.0
    for q in nb:
        s = s + float(before[q][0])
    assert r1["dist"][list(r1["lin"]).index(at(1, 2, 2))] == f32(s / 6) and np.array_equal(r1["round"], r["round"]) and np.array_equal(r1["lin"], r["lin"])
    assert r1["volume"]["dist"][a] == f32(VS) and r1["volume"]["dist"][b] == f32(5 * VS)
    # an observed voxel with a zero gradient: the constant extension
    c = at(2, 2, 2)
    r = fref.fill(volume(dim, [c], dist={c: f32(0.5 * VS)}, grad={c: f32([0, 0, 0])}), dim, VS, 2, 3)
    assert (r["dist"] == f32(0.5 * VS)).all() and not r["grad"].any() and len(r["lin"]) == 6 + 18
    # everything observed, nothing observed, R = 0
    v = volume(dim, np.arange(125))
    assert len(fref.fill(v, dim, VS, 5, 2)["lin"]) == 0
    v = volume(dim, [])
    assert len(fref.fill(v, dim, VS, 5, 2)["lin"]) == 0
    v = volume(dim, [c])
    r = fref.fill(v, dim, VS, 0, 4)
    assert len(r["lin"]) == 0 and all(r["volume"][k].tobytes() == v[k].tobytes() for k in v)
    # R = 255 on 5^3: everything filled, no round beyond the largest distance in the grid
    r = fref.fill(volume(dim, [at(0, 0, 0)]), dim, VS, 255, 0)
    assert len(r["lin"]) == 124 and r["round"].max() == 12


@functools.lru_cache(maxsize=None)
def sphere(hole_planes, R, K):
    """the 32^3 bumpy sphere with a hole of hole_planes planes, filled (R = 0: as it is): (volume, dim, vs, shape, mesh, topology)"""
    v, dim, vs, shape = fref.analytic_volume(32, hole_planes)
    vol = fref.fill(v, dim, vs, R, K)["volume"] if R else v
    m = mref.mesh(vol, dim, vs)
    return vol, dim, vs, shape, m, mref.topology(m[3], len(m[0]))


def surface_distance(m, shape, vs):
    """|f| / vs of the vertices: their distance to the analytic surface, in voxels"""
    return np.abs(synth._shape_f(m[0].astype(np.float64), *shape)[0]) / vs


def winding_agrees(m):
    p = m[0][m[3]].astype(np.float64)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return bool((np.einsum("ij,ij->i", fn, m[1][m[3]].sum(1)) > 0).all())


@pytest.mark.parametrize("R,K,nv,nf,closed,chi,boundary", [(0, 0, 1732, 3412, False, 1, 50), (1, 0, None, None, False, 1, 34), (2, 0, 1812, 3620, True, 2, 0), (2, 4, 1798, 3592, True, 2, 0)])
def test_filling_closes_the_hole_of_the_bumpy_sphere(R, K, nv, nf, closed, chi, boundary):
    """Measured: vertices' distance to the analytic surface, max / p99 in voxels: unfilled 0.385 / 0.092, R=2 K=0 0.421 / 0.210, R=2 K=4 0.385 / 0.141
    (the 0.385 is the unfilled mesh's own maximum)."""
    vol, dim, vs, shape, m, (is_closed, euler, bnd, over) = sphere(4, R, K)
    assert (is_closed, euler, len(bnd), over) == (closed, chi, boundary, 0)
    if nv is not None:
        assert (len(m[0]), len(m[3])) == (nv, nf)
    d = surface_distance(m, shape, vs)
    print(f"R={R} K={K}: {len(m[0])} vertices, {len(m[3])} faces, boundary edges {len(bnd)}, chi {euler}; |f|/vs max {d.max():.3f} p99 {np.percentile(d, 99):.3f}")
    if R == 2:
        assert winding_agrees(m)
        assert d.max() < 0.75


def test_a_hole_twice_as_wide_needs_more_rounds():
    for R, closed, chi, boundary in ((2, False, 1, 34), (6, True, 2, 0)):
        _, _, _, _, m, (is_closed, euler, bnd, over) = sphere(8, R, 0)
        assert (is_closed, euler, len(bnd), over) == (closed, chi, boundary, 0), R


@pytest.mark.parametrize("hole_planes,R", [(4, 1), (4, 2), (8, 6)])
def test_round_is_the_city_block_distance_to_the_observed_set(hole_planes, R):
    v, dim, vs, _ = fref.analytic_volume(32, hole_planes)
    r = fref.fill(v, dim, vs, R, 0)
    dist = fref.manhattan(v["weight"], dim, R + 1)
    assert np.array_equal(r["lin"], np.nonzero((dist >= 1) & (dist <= R))[0]) and np.array_equal(r["round"], dist[r["lin"]])
    assert (np.bincount(r["round"], minlength=R + 1)[1:] > 0).all()


def test_vertex_filled_rule():
    dim = (5, 5, 5)
    lin = np.array([31, 32, 62], np.int64)
    keys = np.array([4 * 31 + 0, 4 * 30 + 0, 4 * 31 + 3, 4 * 37 + 2, 4 * 6 + 1, 4 * 57 + 1, 4 * 0 + 3], np.int64)      # 31|32, 30|31, 31 alone, 37|62, 6|11, 57|62, 0 alone
    assert fref.vertex_filled(keys, lin, dim).tolist() == [2, 1, 2, 1, 0, 1, 0]


def test_fill_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    res = resources("fill.hip", tmp_path)
    ks = {k: v for k, v in res.items() if "k_fill_" in k or "k_wmesh_filled" in k}
    assert len(ks) == 9 and all(v["scratch"] == 0 for v in ks.values()), ks


@pytest.mark.parametrize("hole_planes,R,K", [(4, 2, 0), (4, 2, 4), (8, 6, 0)])
def test_vertices_between_unfilled_voxels_keep_their_bits(hole_planes, R, K):
    """the filled mesh is placed in the unfilled crop box's frame (_fill_ref.mesh_filled): a vertex without a filled end voxel is a row of the unfilled
    mesh bit for bit, normal and colour too, although the crop box's corner moves from (4, 6, 3) to (4, 5, 3); against the filled box's own frame the
    positions are within 1 float32 ulp"""
    v, dim, vs, _ = fref.analytic_volume(32, hole_planes)
    f = fref.fill(v, dim, vs, R, K)
    assert not np.array_equal(mref.crop_box(v["dist"], dim, vs)[0], mref.crop_box(f["volume"]["dist"], dim, vs)[0])
    xyz, nrm, rgb, faces, keys = fref.mesh_filled(v, f["volume"], dim, vs)
    own = mref.mesh(f["volume"], dim, vs)
    a, b = np.ascontiguousarray(xyz).view(np.int32).astype(np.int64), np.ascontiguousarray(own[0]).view(np.int32).astype(np.int64)
    assert np.abs(a - b).max() == 1 and np.array_equal(faces, own[3]) and np.array_equal(nrm, own[1]) and np.array_equal(rgb, own[2])
    plain = mref.mesh(v, dim, vs)
    old = fref.vertex_filled(keys, f["lin"], dim) == 0
    assert old.sum() == len(plain[0])
    for q in range(3):
        assert plain[q].tobytes() == (xyz, nrm, rgb)[q][old].tobytes(), q      # the same rows in the same order
