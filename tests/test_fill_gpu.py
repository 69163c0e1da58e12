"""Hole filling on the device (include/psgsdf_fill.h, csrc/fill.hip; DESIGN.md "Hole filling"): the filled voxels against the float64 restatement
tests/_fill_ref.py on the bumpy sphere with a hole and on 5^3 / 5x5x9 grids built to catch an in-place update, the mesh of the filled state against
tests/_mesh_ref.py and tests/_mesh_components_ref.py on the restatement's filled volume, no side effects on the optimisation, the error returns,
the refusal on ranks, and `voxelPS --mesh-fill`.

Every operation of the definition is an IEEE double operation, so the device is expected to give the restatement's bits; the tests allow 1 float32 ulp.
Largest distance measured on the MI355X over the cases below: 0 ulp (profiles/fill_mi355x.md)."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import _fill_ref as fref
import _mesh_components_ref as ccref
import _mesh_ref as mref
from _curvature_ref import mesh_keys
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_curvature_gpu import K9, SCENE_EXE, bumpy, state, upload
from test_fill_cpu import VS, fill_comment, read_ply_filled, volume
from test_mesh_indexed_cpu import read_ply_indexed
from test_mesh_indexed_gpu import EXE, assert_matches_restatement, ulps, voxelps_config

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ("dist", "grad", "rgb")
MESH = ("xyz", "normals", "rgb", "faces", "vertex_component", "components")


def upload_volume(v, dim, vs=VS):
    """a context holding the volume v (dist, grad, weight, rgb as tests/_fill_ref.py takes them), no keyframes"""
    n = int(np.prod(dim))
    g = capi.GridDesc(); g.dim[:] = [int(x) for x in dim]; g.voxel_size = vs; g.shift[:] = [0.0, 0.0, 0.0]; g.truncation = 5 * vs
    eng = capi.load_engine(g, K9, capi.default_settings(capi.SH1), 0)
    eng.upload_volume(np.ascontiguousarray(v["dist"], f32), np.ascontiguousarray(v["grad"], f32), np.ascontiguousarray(v["weight"], f32), np.ascontiguousarray(v["rgb"], f32),
                      np.zeros((n, 1), np.uint64), 1)
    return eng


def assert_rows(got, exp, tag):
    """lin and round exactly, every float within 1 ulp of the restatement; returns the largest distance"""
    assert got["lin"].dtype == np.int64 and got["round"].dtype == np.uint8
    assert np.array_equal(got["lin"], exp["lin"]) and np.array_equal(got["round"], exp["round"]), (tag, len(got["lin"]), len(exp["lin"]))
    worst = 0
    for k in FLOATS:
        assert got[k].dtype == np.float32 and got[k].shape == exp[k].shape, (tag, k)
        worst = max(worst, int(ulps(got[k], exp[k]).max()) if got[k].size else 0)
    print(f"{tag}: {len(got['lin'])} filled voxels, rounds {np.bincount(got['round']).tolist()[1:]}, largest distance from the restatement {worst} ulp")
    assert worst <= 1, (tag, worst)
    return worst


def assert_same_table(t, e, vs):
    """the component table against the yardstick's, as tests/test_mesh_components_gpu.py compares them: integers and boxes exactly, the area to within
    one unit of its fixed point per face"""
    assert len(t) == len(e)
    for k in ccref.INT_FIELDS:
        assert np.array_equal(t[k], e[k]), (k, t[k][:8], e[k][:8])
    assert np.array_equal(t["lo"], e["lo"]) and np.array_equal(t["hi"], e["hi"])
    assert (np.abs(t["area"] - e["area"]) <= e["n_faces"] * vs * vs / 2 ** 24).all()
    assert np.array_equal(t["kept"], e["kept"]) and not t["reserved"].any()


def same_bytes(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


@pytest.mark.parametrize("R,K", [(1, 0), (2, 0), (2, 4), (6, 16)])
def test_rows_match_the_restatement_on_the_bumpy_sphere_with_a_hole(built, R, K):
    eng, v, dim, vs = bumpy(True)
    got = eng.fill_voxels(R, K)
    assert_rows(got, fref.fill(v, dim, vs, R, K), f"bumpy sphere with a hole, R={R} K={K}")
    assert len(got["lin"]) > 2000 and (np.diff(got["lin"]) > 0).all()
    assert same_bytes(got, eng.fill_voxels(R, K))      # two calls give the same bits
    after = eng.download_volume()
    assert all(after[k].tobytes() == v[k].tobytes() for k in ("dist", "grad", "weight", "rgb"))


def test_where_the_kernel_can_go_wrong(built):
    dim = (5, 5, 5)
    at = lambda i, j, k: (k * 5 + j) * 5 + i

    def both(v, dim, R, K, tag):
        got = upload_volume(v, dim).fill_voxels(R, K)
        assert_rows(got, fref.fill(v, dim, VS, R, K), tag)
        return got

    # one observed voxel at a grid corner, R = 3, on 5^3 and on 5 x 5 x 9: the round is the city-block distance and no face of the grid is crossed
    for d in (dim, (5, 5, 9)):
        r = both(volume(d, [0]), d, 3, 0, f"corner of {d}")
        i, j, k = r["lin"] % 5, (r["lin"] // 5) % 5, r["lin"] // 25
        assert np.array_equal(r["round"], i + j + k) and len(r["lin"]) == 19
        far = (d[2] * 5 * 5) - 1      # ... nor from the opposite corner
        r = both(volume(d, [far]), d, 3, 0, f"far corner of {d}")
        assert np.array_equal(r["round"], (4 - r["lin"] % 5) + (4 - (r["lin"] // 5) % 5) + (d[2] - 1 - r["lin"] // 25)) and len(r["lin"]) == 19
    # two observed voxels three apart along x with different distances and gradients (tests/test_fill_cpu.py has the numbers by hand): the voxels
    # between them take their round-1 values from one side only, a voxel reached from two sides in one round takes both
    a, b = at(0, 2, 2), at(3, 2, 2)
    for d in (dim, (5, 5, 9)):
        v = volume(d, [a, b], dist={a: f32(VS), b: f32(5 * VS)}, grad={a: f32([2, 0, 0]), b: f32([-3, 0, 0])}, rgb={a: f32([0, 0.25, 1]), b: f32([1, 0.75, 0])})
        r = both(v, d, 2, 0, f"two sources in {d}")
        row = lambda q: list(r["lin"]).index(q)
        h = float(f32(VS))
        assert r["dist"][row(at(1, 2, 2))] == f32(float(f32(VS)) + h) and np.array_equal(r["grad"][row(at(1, 2, 2))], f32([1, 0, 0])) and np.array_equal(r["rgb"][row(at(1, 2, 2))], f32([0, 0.25, 1]))
        assert r["dist"][row(at(2, 2, 2))] == f32(float(f32(5 * VS)) + h) and np.array_equal(r["grad"][row(at(2, 2, 2))], f32([-1, 0, 0])) and np.array_equal(r["rgb"][row(at(2, 2, 2))], f32([1, 0.75, 0]))
        assert r["round"][row(at(1, 3, 2))] == 2 and r["round"][row(at(2, 3, 2))] == 2
        for K in (1, 2, 5):      # an in-place sweep fails these
            both(v, d, 2, K, f"two sources in {d}, K={K}")
    # an observed voxel with a zero gradient (tests/test_curvature_gpu.py upload: no gradients, grey albedo): the constant extension
    c = at(2, 2, 2)
    w = np.zeros(125, f32); w[c] = 1
    r = upload(np.full(125, 0.5 * VS, f32), w, dim).fill_voxels(2, 3)
    assert len(r["lin"]) == 24 and (r["dist"] == f32(0.5 * VS)).all() and not r["grad"].any() and (r["rgb"] == f32(0.5)).all()
    # everything observed; nothing observed (an empty mesh, no error); R = 0
    full = upload_volume(volume(dim, np.arange(125)), dim)
    assert len(full.fill_voxels(5, 2)["lin"]) == 0
    none = upload_volume(volume(dim, []), dim)
    r = none.fill_voxels(5, 2)
    assert len(r["lin"]) == 0 and r["grad"].shape == (0, 3) and r["lin"].dtype == np.int64 and r["round"].dtype == np.uint8
    m = none.extract_mesh_filled(5, 2)
    assert len(m["xyz"]) == 0 and len(m["faces"]) == 0 and len(m["components"]) == 0 and len(m["vertex_filled"]) == 0
    one = upload_volume(volume(dim, [c]), dim)
    assert len(one.fill_voxels(0, 4)["lin"]) == 0
    # R = 255 on 5^3 and 5 x 5 x 9: everything filled, no round beyond the largest distance in the grid
    for d in (dim, (5, 5, 9)):
        r = both(volume(d, [0]), d, 255, 2, f"R=255 in {d}")
        assert len(r["lin"]) == int(np.prod(d)) - 1 and r["round"].max() == sum(d) - 3


@pytest.mark.parametrize("R,K", [(2, 0), (2, 4)])
def test_mesh_of_the_filled_state(built, R, K):
    eng, v, dim, vs = bumpy(True)
    filled = fref.fill(v, dim, vs, R, K)
    vol = filled["volume"]
    got = eng.extract_mesh_filled(R, K)
    assert_matches_restatement((got["xyz"], got["normals"], got["rgb"], got["faces"], 0), vol, dim, vs)
    hx, hn, hc, hf, _ = fref.mesh_filled(v, vol, dim, vs)      # ... and, placed in the unfilled box's frame as the header says, to the bit
    print(f"R={R} K={K}: xyz from the restatement in the filled box's frame {int(ulps(got['xyz'], mref.mesh(vol, dim, vs)[0]).max())} ulp, in the unfilled box's frame {int(ulps(got['xyz'], hx).max())} ulp")
    assert np.array_equal(got["xyz"], hx) and np.array_equal(got["faces"], hf)
    closed, chi, bnd, over = mref.topology(got["faces"], len(got["xyz"]))
    assert closed and chi == 2 and over == 0 and len(bnd) == 0
    exp = ccref.components(got["xyz"], got["faces"], vs)
    assert np.array_equal(got["vertex_component"], exp["vertex_component"])
    assert_same_table(got["components"], exp["components"], vs)
    assert len(got["components"]) == 1 and got["components"]["n_boundary_edges"][0] == 0
    before = eng.extract_mesh_components()
    assert before["components"]["n_boundary_edges"].sum() == 50
    # vertex_filled: the rule on the vertex keys and the list of filled voxels
    keys = mesh_keys(vol, dim, vs)
    assert len(keys) == len(got["xyz"])
    assert np.array_equal(got["vertex_filled"], fref.vertex_filled(keys, eng.fill_voxels(R, K)["lin"], dim))
    counts = np.bincount(got["vertex_filled"], minlength=3)
    print(f"R={R} K={K}: {len(got['xyz'])} vertices, {len(got['faces'])} faces, filled end voxels 0 / 1 / 2: {counts.tolist()}")
    assert (counts > 0).all()
    assert counts[0] == len(eng.extract_mesh_indexed()[0])      # every vertex of the unfilled mesh is still there
    assert same_bytes(got, eng.extract_mesh_filled(R, K))      # two calls give the same bytes
    # with a filter: the kept components' arrays, vertex_filled with them
    cut = eng.extract_mesh_filled(R, K, keep_largest=1)
    assert same_bytes(cut, got)


def xyz_rows(a):
    return set(np.ascontiguousarray(a, f32).view(np.dtype((np.void, 12))).ravel().tolist())


@pytest.mark.parametrize("R,K", [(2, 0), (2, 4)])
def test_vertices_without_a_filled_end_voxel_keep_their_bits(built, R, K):
    """The vertex_filled == 0 rows of xyz are rows of the unfilled mesh, bit for bit -- although filling moves the crop box's lower corner from
    (4, 6, 3) to (4, 5, 3) here (a filled voxel in plane j = 5 comes within sqrt(3) voxels of the surface) and psgsdf_extract_mesh's frame computes a
    position as p voxel - origin with origin = -vs lo in float32: the filled mesh's vertices are placed in the UNFILLED box's frame.  In its own
    box's frame 634 of the 1732 rows would differ by one ulp of the coordinate (1.9e-6 voxels)."""
    eng, v, dim, vs = bumpy(True)
    got = eng.extract_mesh_filled(R, K)
    old, plain = got["xyz"][got["vertex_filled"] == 0], eng.extract_mesh_indexed()[0]
    missing = xyz_rows(old) - xyz_rows(plain)
    from scipy.spatial import cKDTree
    far = cKDTree(plain.astype(np.float64)).query(old.astype(np.float64))[0].max() / vs
    print(f"R={R} K={K}: {len(old)} vertices without a filled end voxel, {len(plain)} in the unfilled mesh, {len(missing)} rows with other bits, the farthest {far:.2e} voxels from its twin; "
          f"crop box {[x.tolist() for x in mref.crop_box(v['dist'], dim, vs)]} -> {[x.tolist() for x in mref.crop_box(fref.fill(v, dim, vs, R, K)['volume']['dist'], dim, vs)]}")
    assert len(old) == len(plain) and far == 0
    assert not missing


@pytest.mark.parametrize("R,K", [(2, 0), (2, 4)])
def test_vertices_keep_their_bits_where_the_crop_box_stays(built, R, K):
    """the same sphere with an unobserved d = 0 in the near corner too (the far one has it): the crop box is the grid without and with the filling, and
    normals and colours are checked with the positions"""
    v, dim, vs, _ = fref.analytic_volume(32, 4)
    v["dist"][0] = 0.0
    assert v["weight"][0] == 0
    eng = upload_volume(v, dim, vs)
    got, plain = eng.extract_mesh_filled(R, K), eng.extract_mesh_indexed()
    closed, chi, bnd, over = mref.topology(got["faces"], len(got["xyz"]))
    assert closed and chi == 2 and over == 0
    same = got["vertex_filled"] == 0
    assert same.sum() == len(plain[0]) and (~same).sum() > 50
    assert xyz_rows(got["xyz"][same]) == xyz_rows(plain[0])
    rows = {plain[0][q].tobytes(): (plain[1][q].tobytes(), plain[2][q].tobytes()) for q in range(len(plain[0]))}      # normals and colours with them
    assert all(rows[got["xyz"][q].tobytes()] == (got["normals"][q].tobytes(), got["rgb"][q].tobytes()) for q in np.nonzero(same)[0])


def test_filter_compacts_vertex_filled(built):
    """two spheres, the small one next to a block of unobserved voxels: keep_largest = 1 drops it, and vertex_filled follows the kept vertices"""
    N, vs = 32, VS
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    X = np.stack([i, j, k], -1).reshape(-1, 3) * vs
    c1, c2 = np.array([10.3, 16.2, 15.7]) * vs, np.array([24.4, 16.1, 16.3]) * vs
    d1, d2 = np.linalg.norm(X - c1, axis=1) - 7 * vs, np.linalg.norm(X - c2, axis=1) - 3.5 * vs
    first = d1 < d2
    dist = np.where(first, d1, d2)
    grad = np.where(first[:, None], (X - c1) / np.maximum(np.linalg.norm(X - c1, axis=1), 1e-9)[:, None], (X - c2) / np.maximum(np.linalg.norm(X - c2, axis=1), 1e-9)[:, None])
    weight = (np.abs(dist) < 2.5 * vs).astype(f32)
    w = weight.reshape(N, N, N); w[14:18, 14:18, :16] = 0; w[15:17, 15:17, 16:] = 0      # a hole in each sphere's surface
    v = dict(dist=dist.astype(f32), grad=grad.T.astype(f32).copy(), weight=weight, rgb=np.full((3, N ** 3), 0.25, f32))
    eng = upload_volume(v, (N, N, N))
    every = eng.extract_mesh_filled(2, 1)
    cut = eng.extract_mesh_filled(2, 1, keep_largest=1)
    assert len(every["components"]) == 2 and every["components"]["kept"].tolist() == [1, 1] and cut["components"]["kept"].sum() == 1
    kept = cut["components"]["kept"][every["vertex_component"]].astype(bool)
    assert 0 < kept.sum() < len(kept) and len(cut["xyz"]) == kept.sum()
    assert np.array_equal(cut["xyz"], every["xyz"][kept]) and np.array_equal(cut["vertex_filled"], every["vertex_filled"][kept])
    assert (np.bincount(every["vertex_filled"][kept], minlength=3) > 0).all() and (every["vertex_filled"][~kept] > 0).any()
    exp = ccref.components(every["xyz"], every["faces"], vs, every["normals"], every["rgb"], keep_largest=1)
    for key in ("xyz", "normals", "rgb", "faces", "vertex_component"):
        assert np.array_equal(cut[key], exp[key]), key
    assert_same_table(cut["components"], exp["components"], vs)


@pytest.mark.parametrize("flt", [{}, {"min_faces": 100}, {"keep_largest": 1}])
def test_no_rounds_is_extract_mesh_components(built, flt):
    eng, v, dim, vs = bumpy(True)
    exp = eng.extract_mesh_components(**flt)
    for K in (0, 4):
        got = eng.extract_mesh_filled(0, K, **flt)
        for k in MESH:
            assert got[k].tobytes() == exp[k].tobytes() and got[k].shape == exp[k].shape, (k, K)
        assert len(got["faces"]) > 1000 and not got["vertex_filled"].any() and len(got["vertex_filled"]) == len(got["xyz"])
    assert len(eng.fill_voxels(0, 4)["lin"]) == 0


def test_no_side_effects(built):
    """two contexts on one scene, two times one iteration each; the first is asked for both results twice in between"""
    sc = synth.make_scene(N=24, F=3, W=64, H=48, model="SH1")
    res = []
    for ask in (True, False):
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo(); eng.normalize_weights()
        recs = eng.iterate(capi.ALL, 1)
        mesh = eng.extract_mesh_indexed()
        if ask:
            before = eng.download_volume()
            a = (eng.fill_voxels(2, 3), eng.extract_mesh_filled(2, 3))
            b = (eng.fill_voxels(2, 3), eng.extract_mesh_filled(2, 3))
            assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])      # two calls give the same bits
            assert len(a[0]["lin"]) > 500 and len(a[1]["faces"]) > 500 and (a[1]["vertex_filled"] > 0).any()
            after = eng.download_volume()      # the state as it was
            i = eng.info()
            assert all(after[k].tobytes() == before[k].tobytes() for k in ("dist", "grad", "weight", "rgb"))
            assert_rows(a[0], fref.fill(before, [int(x) for x in i.dim], float(i.voxel_size), 2, 3), "after one iteration")
            for x, y in zip(mesh, eng.extract_mesh_indexed()):      # a later extraction returns what it returned before
                assert np.array_equal(x, y)
        recs += eng.iterate(capi.ALL, 1)
        res.append(dict(vol=eng.download_volume(), light=eng.download_light(), poses=eng.download_poses(), energy=eng.energy(), mesh=eng.extract_mesh_indexed(), recs=recs))
    a, b = res
    for k in ("dist", "grad", "weight", "rgb"):
        assert a["vol"][k].tobytes() == b["vol"][k].tobytes(), k
    assert a["light"].tobytes() == b["light"].tobytes() and a["poses"].tobytes() == b["poses"].tobytes()
    assert a["energy"] == b["energy"] and a["recs"] == b["recs"]
    for x, y in zip(a["mesh"], b["mesh"]):
        assert np.array_equal(x, y)


def test_errors(built):
    import ctypes as C
    sc = synth.make_scene(N=24, F=3, W=64, H=48, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    for call in (lambda: eng.fill_voxels(2, 1), lambda: eng.fill_voxels(0, 0), lambda: eng.extract_mesh_filled(2, 1)):      # before a volume
        with pytest.raises(capi.PsgsdfError, match="rc=-4"):
            call()
    eng.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)      # a volume is enough: no keyframes, no band
    assert len(eng.fill_voxels(2, 1)["lin"]) > 500 and len(eng.extract_mesh_filled(2, 1)["faces"]) > 500
    for R, K in ((-1, 0), (256, 0), (2, -1), (2, 4097)):
        for call in (eng.fill_voxels, eng.extract_mesh_filled):
            with pytest.raises(capi.PsgsdfError, match="rc=-1"):
                call(R, K)
    for bad in (dict(keep_largest=-1), dict(min_area=float("nan"))):
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):
            eng.extract_mesh_filled(2, 1, **bad)
    assert len(eng.fill_voxels(255, 0)["lin"]) > 500 and len(eng.fill_voxels(1, 4096)["lin"]) > 500      # the ends of the ranges
    P = C.c_void_p
    vox = eng._fn("fill_voxels"); vox.argtypes = [P, C.c_int32, C.c_int32] + [P] * 6
    msh = eng._fn("extract_mesh_filled"); msh.argtypes = [P, C.c_int32, C.c_int32, P] + [P] * 10
    outs = [P(0x10) for _ in range(10)]
    refs = [C.byref(o) for o in outs]
    for k in range(6):
        assert vox(eng.ctx, 2, 1, *[None if i == k else r for i, r in enumerate(refs[:6])]) == -1
    for k in range(10):
        assert msh(eng.ctx, 2, 1, None, *[None if i == k else r for i, r in enumerate(refs)]) == -1
    flt = capi.MeshFilter(0, 0.0, -1)
    for R, K, f in ((-1, 0, None), (256, 0, None), (2, -1, None), (2, 4097, None), (2, 1, C.byref(flt))):
        assert msh(eng.ctx, R, K, f, *refs) == -1
        if f is None:
            assert vox(eng.ctx, R, K, *refs[:6]) == -1
    assert all(o.value == 0x10 for o in outs)      # a call that fails its argument checks leaves the outputs alone
    assert len(eng.extract_mesh_filled(2, 1)["faces"]) > 500      # the context still works


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the context
    goes on working (the collective psgsdf_extract_mesh_indexed afterwards).  tests/_refused_ranks.py's driver with this family."""
    res = refused_ranks(tmp_path, "fill", N=32, F=3)
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e, name in zip(res[1]["errors"], ("fill_voxels", "extract_mesh_filled")):
        assert "rc=-3" in e and "rank 1 of 2" in e and name in e, e
    assert res[0]["faces"] + res[1]["faces"] > 500 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_flags(built, tmp_path):
    outs = {}
    for name, extra in (("plain", []), ("filled", ["--mesh-fill", "2"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4}), "--indexed-mesh"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    base = sorted(f for f in os.listdir(outs["plain"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in base if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes and not any("filled" in f for f in base)
    assert sorted(f for f in os.listdir(outs["filled"]) if f not in skip) == sorted(base + [m + "_mesh_filled.ply" for m in meshes])      # the only new files
    for f in base:      # the flag changes no other file
        assert filecmp.cmp(outs["plain"] + f, outs["filled"] + f, shallow=False), f
    for m in meshes:
        head, verts, faces = read_ply_filled(outs["filled"] + m + "_mesh_filled.ply")
        ihead, iverts, ifaces = read_ply_indexed(outs["filled"] + m + "_mesh_indexed.ply")
        assert [h for h in head if not h.startswith(("comment fill", "property", "element"))] == [h for h in ihead if not h.startswith(("property", "element"))]
        c = fill_comment(head)
        topo = lambda f, n: len(mref.topology(f, n)[2])
        print(f"{m}: {len(iverts)} -> {len(verts)} vertices, {len(ifaces)} -> {len(faces)} faces, {c}")
        assert c["rounds"] == 2 and c["sweeps"] == 4 and c["voxels"] > 1000
        assert c["before"] == topo(ifaces, len(iverts)) and c["after"] == topo(faces, len(verts))
        assert set(np.unique(verts["filled"]).tolist()) <= {0, 1, 2} and (verts["filled"] > 0).any() and len(faces) > 1000
    cfg = outs["filled"] + "config.json"
    for extra, word in ((["--mesh-fill", "2", "--gpus", "2"], "--mesh-fill needs a single process"), (["--mesh-fill", "-1"], "--mesh-fill:"), (["--mesh-fill", "256"], "--mesh-fill:"),
                        (["--mesh-fill", "2", "--mesh-fill-sweeps", "4097"], "--mesh-fill-sweeps:"), (["--mesh-fill-sweeps", "3"], "--mesh-fill-sweeps needs --mesh-fill")):
        r = subprocess.run([EXE, "--config_file", cfg] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)


def test_voxelps_files_equal_the_api(built, tmp_path):
    """the host mirror on a dumped synthetic scene (tests/test_host_mirror_gpu.py: the same library, the same calls, the same bits as the ctypes path)
    with the flag: the columns of the last dump's PLY and the numbers of its comment line are the API's on the optimised state"""
    from test_host_mirror_gpu import dump
    sc = synth.make_scene(N=32, F=4, W=64, H=48, model="SH1")
    max_it, conv, R, K = 3, 1e-9, 3, 2      # (dumps come after every third iteration: the last one is the final state)
    st = capi.default_settings(sc.model_id, max_it=max_it, conv_threshold=conv)
    ind, outd = str(tmp_path / "scene") + "/", str(tmp_path / "out") + "/"
    os.makedirs(outd)
    dump(sc, ind, max_it, conv, 0, st.reg_weight_n, st.reg_weight_l, st.damping)
    r = subprocess.run([SCENE_EXE, ind, outd, "--mesh-fill", str(R), "--mesh-fill-sweeps", str(K)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    eng = capi.load_engine(sc, sc.K, st, 0); eng.load_scene(sc)
    eng.optimize(capi.ALL)
    assert np.array_equal(np.fromfile(outd + "dist_out.f32", np.float32)[eng.download_band()], eng.download_volume()["dist"][eng.download_band()])
    api = eng.extract_mesh_filled(R, K)
    head, verts, faces = read_ply_filled(outd + f"after_iter_{max_it}_mesh_filled.ply")
    assert np.array_equal(faces, api["faces"]) and len(faces) > 1000
    assert np.array_equal(np.stack([verts[k] for k in "xyz"], 1), api["xyz"]) and np.array_equal(np.stack([verts[k] for k in ("nx", "ny", "nz")], 1), api["normals"])
    assert np.array_equal(np.stack([verts[k] for k in ("red", "green", "blue")], 1), api["rgb"]) and verts["filled"].tobytes() == api["vertex_filled"].tobytes()
    c = fill_comment(head)
    assert c == dict(rounds=R, sweeps=K, voxels=len(eng.fill_voxels(R, K)["lin"]), before=int(eng.extract_mesh_components()["components"]["n_boundary_edges"].sum()),
                     after=int(api["components"]["n_boundary_edges"].sum()))
