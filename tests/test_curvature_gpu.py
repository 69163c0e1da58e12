"""Surface curvature on the device (include/psgsdf_curvature.h, csrc/curvature.hip; DESIGN.md "Surface curvature"): the per-voxel rows against the
float64 restatement tests/_curvature_ref.py and against closed-form geometry, the validity rules on a 5^3 stencil, the vertex rule and the baked map
against the per-voxel call, no side effects on the optimisation, the error returns, and `voxelPS --mesh-curvature / --mesh-bake-curvature`.

Every operation of the definition is an IEEE double operation, so the device is expected to give the restatement's bits; the tests allow 1 float32 ulp.
Largest distance measured on the MI355X over the cases below: 0 ulp (profiles/curvature_mi355x.md)."""
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

import _curvature_ref as cref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_curvature_cpu import N, SHAPES, VS, assert_analytic, assert_header_matches_columns, read_ply_curvature, shape_volume
from test_mesh_indexed_cpu import read_ply_indexed
from test_mesh_indexed_gpu import EXE, analytic_engine, ulps, voxelps_config

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelps_scene")
K9 = f32([100, 0, 32, 0, 100, 24, 0, 0, 1])
FLOATS = ("mean", "gauss", "k1", "k2", "dir1")


def upload(dist, weight, dim, vs=VS):
    """a context holding the volume: dist and weight as given, no gradients, grey albedo, no keyframes"""
    n = int(np.prod(dim))
    g = capi.GridDesc(); g.dim[:] = [int(x) for x in dim]; g.voxel_size = vs; g.shift[:] = [0.0, 0.0, 0.0]; g.truncation = 5 * vs
    eng = capi.load_engine(g, K9, capi.default_settings(capi.SH1), 0)
    eng.upload_volume(np.ascontiguousarray(dist, f32), np.zeros((3, n), f32), np.ascontiguousarray(weight, f32), np.full((3, n), 0.5, f32), np.zeros((n, 1), np.uint64), 1)
    return eng


def state(eng):
    i = eng.info()
    return eng.download_volume(), [int(x) for x in i.dim], float(i.voxel_size)


def assert_rows(got, exp, tag):
    """valid exactly, every float within 1 ulp of the restatement rounded to float32; returns the largest distance"""
    assert np.array_equal(got["valid"], exp["valid"]), tag
    worst = 0
    for k in FLOATS:
        assert got[k].dtype == np.float32 and got[k].shape == exp[k].shape, (tag, k)
        u = int(ulps(got[k], exp[k]).max()) if got[k].size else 0
        worst = max(worst, u)
    print(f"{tag}: {len(got['valid'])} voxels, {int(got['valid'].sum())} valid, largest distance from the restatement {worst} ulp")
    assert worst <= 1, (tag, worst)
    return worst


@functools.lru_cache(maxsize=None)
def bumpy(hole):
    """the bumpy sphere of tests/test_mesh_indexed_gpu.py at 32^3 (with hole: a block of unobserved voxels across its surface), its state downloaded"""
    eng, _, vs, _ = analytic_engine(N=32, hole=hole)
    return (eng,) + tuple(state(eng))


@pytest.mark.parametrize("kind", SHAPES)
def test_rows_match_the_restatement_and_the_analytic_bounds(built, kind):
    v, dim, X, lin = shape_volume(kind)
    eng = upload(v["dist"], v["weight"], dim)
    dv, ddim, dvs = state(eng)
    assert np.array_equal(dv["dist"], v["dist"]) and ddim == list(dim) and dvs == float(f32(VS))
    every = np.arange(N ** 3, dtype=np.int64)
    got = eng.curvature_voxels(every)
    assert_rows(got, cref.voxels(v, dim, VS, every), kind)
    assert got["valid"].sum() > 500 and not any(got[k][got["valid"] == 0].any() for k in FLOATS)
    near = eng.curvature_voxels(lin)
    for k in FLOATS + ("valid",):
        assert np.array_equal(near[k], got[k][lin]), k
    assert_analytic(kind, X[lin], near, "device")


def test_rows_match_the_restatement_on_the_bumpy_sphere_with_a_hole(built):
    eng, v, dim, vs = bumpy(True)
    every = np.arange(int(np.prod(dim)), dtype=np.int64)
    got = eng.curvature_voxels(every)
    assert_rows(got, cref.voxels(v, dim, vs, every), "bumpy sphere with a hole")
    near = np.abs(v["dist"]) < vs
    assert got["valid"][near].sum() > 1000 and (got["valid"][near] == 0).sum() > 20      # the hole and its rim
    assert np.median(got["mean"][near & (got["valid"] == 1)]) > 0                        # convex on the whole


def plane5(nz=5, normal=(0.36, -0.48, 0.8)):
    k, j, i = np.meshgrid(np.arange(nz), np.arange(5), np.arange(5), indexing="ij")
    return ((normal[0] * i + normal[1] * j + normal[2] * k) * VS).ravel().astype(f32)


def test_where_the_kernel_can_go_wrong(built):
    c = (2 * 5 + 2) * 5 + 2
    dist = plane5()
    ones = np.ones(125, f32)
    eng = upload(dist, ones, (5, 5, 5))
    v = dict(dist=dist, weight=ones)
    every = np.arange(125, dtype=np.int64)
    got = eng.curvature_voxels(every)
    assert_rows(got, cref.voxels(v, (5, 5, 5), VS, every), "5^3 plane")
    inner = np.zeros((5, 5, 5), bool); inner[1:-1, 1:-1, 1:-1] = True
    assert got["valid"][c] == 1 and np.array_equal(got["valid"].reshape(5, 5, 5) == 1, inner)      # every voxel on a grid face is invalid
    # the indices that are no voxel, duplicates, a descending list, the empty list
    odd = np.array([c, -1, 125, 1 << 40, c, -(1 << 40), 124, 0, c + 1], np.int64)
    r = eng.curvature_voxels(odd)
    assert r["valid"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for k in FLOATS:
        assert np.array_equal(r[k][0], got[k][c]) and np.array_equal(r[k][4], got[k][c]) and np.array_equal(r[k][8], got[k][c + 1]) and not r[k][[1, 2, 3, 5, 6, 7]].any(), k
    down = eng.curvature_voxels(every[::-1].copy())
    for k in FLOATS + ("valid",):
        assert np.array_equal(down[k], got[k][::-1]), k
    none = eng.curvature_voxels(np.zeros(0, np.int64))
    assert all(len(none[k]) == 0 for k in none) and none["dir1"].shape == (0, 3) and none["valid"].dtype == np.uint8 and none["mean"].dtype == np.float32
    # one of the 27 neighbours unobserved, in 27 blocks of 5 planes stacked along z (a block's stencil stays inside the block): the 18 of the stencil
    # invalidate the centre, the 8 cube corners do not matter
    dist27 = plane5(nz=135)
    w27 = np.ones(125 * 27, f32)
    centres, expect = [], []
    for b, (dk, dj, di) in enumerate((dk, dj, di) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)):
        cb = 125 * b + c
        w27[cb + (dk * 5 + dj) * 5 + di] = 0
        centres.append(cb); expect.append(1 if abs(di) + abs(dj) + abs(dk) == 3 else 0)
    assert sum(expect) == 8
    e27 = upload(dist27, w27, (5, 5, 135))
    r27 = e27.curvature_voxels(np.array(centres, np.int64))
    assert r27["valid"].tolist() == expect
    assert_rows(r27, cref.voxels(dict(dist=dist27, weight=w27), (5, 5, 135), VS, centres), "27 blocks")
    # a constant distance: G2 = 0
    flat = upload(np.full(125, 0.01, f32), ones, (5, 5, 5)).curvature_voxels(every)
    assert not flat["valid"].any() and not any(flat[k].any() for k in FLOATS)
    # the normal along -z exactly: the frame's sg = -1 branch
    dz = plane5(normal=(0.0, 0.0, -1.0))
    r = upload(dz, ones, (5, 5, 5)).curvature_voxels([c])
    assert_rows(r, cref.voxels(dict(dist=dz, weight=ones), (5, 5, 5), VS, [c]), "normal -z")
    assert r["valid"][0] == 1 and r["mean"][0] == 0 and np.array_equal(r["dir1"][0], f32([1, 0, 0]))


@pytest.mark.parametrize("hole", [False, True])
def test_vertices(built, hole):
    eng, v, dim, vs = bumpy(hole)
    plain = eng.extract_mesh_indexed()
    got = eng.extract_mesh_curvature()
    assert len(got["faces"]) > 1000
    for name, a in zip(("xyz", "normals", "rgb", "faces"), plain):
        assert got[name].tobytes() == a.tobytes() and got[name].shape == a.shape, name
    keys = cref.mesh_keys(v, dim, vs)
    assert len(keys) == len(got["xyz"])
    exp = cref.vertices(v, dim, keys, eng.curvature_voxels)      # the rule, fed with the device's own per-voxel floats
    assert np.array_equal(got["valid"], exp["valid"])
    worst = max(int(ulps(got[k], exp[k]).max()) for k in cref.SCALARS)
    counts = np.bincount(got["valid"], minlength=3)
    print(f"hole {hole}: {len(keys)} vertices, valid end voxels 0 / 1 / 2: {counts.tolist()}, largest distance from the rule {worst} ulp")
    assert worst <= 1
    assert not any(got[k][got["valid"] == 0].any() for k in cref.SCALARS)
    ref_valid = cref.vertices(v, dim, keys, lambda q: cref.voxels(v, dim, vs, q))["valid"]      # the restatement alone
    assert np.array_equal(ref_valid, got["valid"])
    if hole:
        assert (np.bincount(ref_valid, minlength=3) > 0).all() and (counts > 0).all()
    else:
        assert counts[2] == len(keys)
    again = eng.extract_mesh_curvature()
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_bake(built):
    eng, v, dim, vs = bumpy(False)
    plain = eng.bake_lod(2 * vs, 4)
    got = eng.bake_lod_curvature(2 * vs, 4)
    for k, a in plain.items():
        assert (got[k].tobytes() == a.tobytes() and got[k].shape == a.shape) if isinstance(a, np.ndarray) else got[k] == a, k
    H, W = plain["height"], plain["width"]
    assert got["mean"].shape == (H, W) and got["valid"].shape == (H, W) and got["mean"].dtype == np.float32 and got["valid"].dtype == np.uint8
    hit = plain["voxel"] >= 0
    assert hit.sum() > 1000 and (~hit).sum() > 100
    rows = eng.curvature_voxels(plain["voxel"][hit])
    assert got["mean"][hit].tobytes() == rows["mean"].tobytes() and np.array_equal(got["valid"][hit], rows["valid"])
    assert not got["mean"][~hit].any() and not got["valid"][~hit].any()
    assert got["n_valid"] == int(got["valid"].sum()) and got["n_valid"] > 1000
    assert_rows(rows, cref.voxels(v, dim, vs, plain["voxel"][hit]), "hit texels")
    again = eng.bake_lod_curvature(2 * vs, 4)
    assert again["mean"].tobytes() == got["mean"].tobytes() and again["valid"].tobytes() == got["valid"].tobytes()
    empty = eng.bake_lod_curvature(64 * vs, 4)      # everything in one cluster: an empty level-of-detail mesh
    assert empty["width"] == 0 and empty["mean"].size == 0 and empty["n_valid"] == 0


def test_no_side_effects(built):
    """two contexts on one scene, two times one iteration each; the first is asked for all three results in between"""
    sc = synth.make_scene(N=24, F=3, W=64, H=48, model="SH1")
    res = []
    for ask in (True, False):
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo(); eng.normalize_weights()
        recs = eng.iterate(capi.ALL, 1)
        mesh = eng.extract_mesh_indexed()
        if ask:
            vs = float(eng.info().voxel_size)
            band = eng.download_band().astype(np.int64)
            a = (eng.curvature_voxels(band), eng.extract_mesh_curvature(), eng.bake_lod_curvature(2 * vs, 4))
            b = (eng.curvature_voxels(band), eng.extract_mesh_curvature(), eng.bake_lod_curvature(2 * vs, 4))
            for x, y in zip(a, b):      # two calls give the same bits
                assert all((x[k].tobytes() == y[k].tobytes()) if isinstance(x[k], np.ndarray) else x[k] == y[k] for k in x)
            assert a[0]["valid"].sum() > 200 and len(a[1]["faces"]) > 500 and a[2]["n_valid"] > 500
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
    for call in (lambda: eng.curvature_voxels([5]), lambda: eng.curvature_voxels([]), eng.extract_mesh_curvature, lambda: eng.bake_lod_curvature(0.1, 4)):      # before a volume
        with pytest.raises(capi.PsgsdfError, match="rc=-4"):
            call()
    eng.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)      # a volume is enough: no keyframes, no band
    vs = float(eng.info().voxel_size)
    assert eng.curvature_voxels(np.nonzero(np.abs(sc.dist) < vs)[0])["valid"].sum() > 200 and len(eng.extract_mesh_curvature()["faces"]) > 500
    for bad in (lambda: eng.bake_lod_curvature(2 * vs, 0), lambda: eng.bake_lod_curvature(0.0, 4), lambda: eng.bake_lod_curvature(2 * vs, 4, float("nan")),
                lambda: eng.bake_lod_curvature(2 * vs, 4, keep_largest=-1)):
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):
            bad()
    with pytest.raises(capi.PsgsdfError, match="rc=-3"):
        eng.bake_lod_curvature(2 * vs, 16383)      # what psgsdf_bake_lod refuses as unsupported: an atlas beyond 16384 texels along a side
    P = C.c_void_p
    vox = eng._fn("curvature_voxels"); vox.argtypes = [P, P, C.c_int64] + [P] * 6
    msh = eng._fn("extract_mesh_curvature"); msh.argtypes = [P] * 12
    bake = eng._fn("bake_lod_curvature"); bake.argtypes = [P, P, C.c_double, C.c_int32, C.c_double, P]
    lin = (C.c_int64 * 2)(5, 6)
    outs = [P(0x10) for _ in range(11)]
    refs = [C.byref(o) for o in outs]
    for k in range(6):
        assert vox(eng.ctx, lin, 2, *[None if i == k else r for i, r in enumerate(refs[:6])]) == -1
    assert vox(eng.ctx, None, 2, *refs[:6]) == -1 and vox(eng.ctx, lin, -1, *refs[:6]) == -1
    for k in range(11):
        assert msh(eng.ctx, *[None if i == k else r for i, r in enumerate(refs)]) == -1
    assert bake(eng.ctx, None, 2 * vs, 4, 2 * vs, None) == -1
    assert all(o.value == 0x10 for o in outs)      # a call that fails its argument checks leaves the outputs alone
    assert eng.bake_lod_curvature(2 * vs, 4)["n_valid"] > 500      # the context still works


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the context
    goes on working (the collective psgsdf_extract_mesh_indexed afterwards).  tests/_refused_ranks.py's driver with this family."""
    res = refused_ranks(tmp_path, "curvature", N=32, F=3)
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 4
    for e, name in zip(res[1]["errors"], ("curvature_voxels", "extract_mesh_curvature", "bake_lod_curvature", "bake_lod_curvature")):
        assert "rc=-3" in e and "rank 1 of 2" in e and name in e, e
    assert res[0]["faces"] + res[1]["faces"] > 500 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_flags(built, tmp_path):
    from PIL import Image
    import _bake_ref as bref
    flags = ["--mesh-curvature", "--mesh-bake-curvature", "0.25"]
    outs = {}
    for name, extra in (("bake", []), ("curvature", flags)):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4}), "--indexed-mesh", "--mesh-lod", "2", "--mesh-bake", "4"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    base = sorted(f for f in os.listdir(outs["bake"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in base if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes and not any("curvature" in f for f in base)
    new = [m + s for m in meshes for s in ("_mesh_curvature.ply", "_mesh_lod_curvature.png")]
    assert sorted(f for f in os.listdir(outs["curvature"]) if f not in skip) == sorted(base + new)      # the only new files
    for f in base:      # the flags change no other file
        assert filecmp.cmp(outs["bake"] + f, outs["curvature"] + f, shallow=False), f
    for m in meshes:
        head, verts, faces = read_ply_curvature(outs["curvature"] + m + "_mesh_curvature.ply")
        ihead, iverts, ifaces = read_ply_indexed(outs["curvature"] + m + "_mesh_indexed.ply")
        assert np.array_equal(faces, ifaces), m
        for k in iverts.dtype.names:
            assert verts[k].tobytes() == iverts[k].tobytes(), (m, k)
        assert [h for h in head if not h.startswith(("comment curvature", "property"))] == [h for h in ihead if not h.startswith("property")]
        assert_header_matches_columns(head, verts)
        none = verts["curvature_valid"] == 0
        assert set(np.unique(verts["curvature_valid"]).tolist()) <= {0, 1, 2} and (~none).sum() > 1000
        assert not any(verts[k][none].any() for k in ("quality", "gauss", "k1", "k2")) and (verts["k1"] >= verts["k2"]).all()
        _, _, lfaces = read_ply_indexed(outs["curvature"] + m + "_mesh_lod.ply")
        L = bref.layout(len(lfaces), 4)
        im = Image.open(outs["curvature"] + m + "_mesh_lod_curvature.png")
        px = np.asarray(im)
        assert im.mode == "L" and px.shape == (L["H"], L["W"])
        own = L["face"] >= 0
        print(f"{m}: {len(verts)} vertices, {int((~none).sum())} with a curvature; atlas {L['W']} x {L['H']}, grey {px[own].min()} .. {px[own].max()}, mean {px[own].mean():.1f}")
        assert (px[~own] == 128).all() and px[own].min() < 128 < px[own].max()
    for extra, word in ((flags[:1] + ["--gpus", "2"], "--mesh-curvature needs a single process"), (["--mesh-lod", "2", "--mesh-bake", "4"] + flags[1:] + ["--gpus", "2"], "--mesh-bake-curvature needs a single process"),
                        (["--mesh-lod", "2"] + flags[1:], "--mesh-bake-curvature needs --mesh-bake"), (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-curvature", "-0.5"], "--mesh-bake-curvature:")):
        r = subprocess.run([EXE, "--config_file", outs["curvature"] + "config.json"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)


def test_voxelps_files_equal_the_api(built, tmp_path):
    """the host mirror on a dumped synthetic scene (tests/test_host_mirror_gpu.py: the same library, the same calls, the same bits as the ctypes path)
    with both flags: the columns of the last dump's PLY and the bytes of its PNG are the API's on the optimised state"""
    from PIL import Image
    from test_host_mirror_gpu import dump
    sc = synth.make_scene(N=32, F=4, W=64, H=48, model="SH1")
    max_it, conv, S = 3, 1e-9, 0.25      # (dumps come after every third iteration: the last one is the final state)
    st = capi.default_settings(sc.model_id, max_it=max_it, conv_threshold=conv)
    ind, outd = str(tmp_path / "scene") + "/", str(tmp_path / "out") + "/"
    os.makedirs(outd)
    dump(sc, ind, max_it, conv, 0, st.reg_weight_n, st.reg_weight_l, st.damping)
    r = subprocess.run([SCENE_EXE, ind, outd, "--mesh-curvature", "--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-curvature", str(S)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    eng = capi.load_engine(sc, sc.K, st, 0); eng.load_scene(sc)
    eng.optimize(capi.ALL)
    assert np.array_equal(np.fromfile(outd + "dist_out.f32", np.float32)[eng.download_band()], eng.download_volume()["dist"][eng.download_band()])
    last = f"after_iter_{max_it}"
    api = eng.extract_mesh_curvature()
    head, verts, faces = read_ply_curvature(outd + last + "_mesh_curvature.ply")
    assert np.array_equal(faces, api["faces"]) and len(faces) > 1000
    for col, k in (("quality", "mean"), ("gauss", "gauss"), ("k1", "k1"), ("k2", "k2"), ("curvature_valid", "valid")):
        assert verts[col].tobytes() == api[k].tobytes(), col
    assert np.array_equal(np.stack([verts[k] for k in "xyz"], 1), api["xyz"])
    assert_header_matches_columns(head, verts)
    vs = float(eng.info().voxel_size)
    bake = eng.bake_lod_curvature(2 * vs, 4)
    px = np.asarray(Image.open(outd + last + "_mesh_lod_curvature.png"))
    assert px.shape == bake["mean"].shape and bake["n_valid"] > 1000
    assert np.array_equal(px, cref.png_byte(bake["mean"], bake["valid"], vs, S))
