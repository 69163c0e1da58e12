"""Ambient occlusion on the device (include/psgsdf_occlusion.h, csrc/occlusion.hip; DESIGN.md "Ambient occlusion").  The points call against closed
form: on the floor-and-wall volume of test_occlusion_cpu the device's mask must equal the analytic one on every ray that is not within 1e-3 voxels
of the radius.  The bake's map against the yardstick tests/_occlusion_ref.py started from the device's OWN bake planes and its own direction table:
the ray bits may differ on at most 2e-3 of the rays (the project's cap for this walk, test_bake_gpu: the yardstick walks in float64 without a cut
at the radius, the device in float32 with one); bytes and counts follow from the masks exactly."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _occlusion_ref as oref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_bake_gpu import LOD_KEYS, same_bits, scene_engine
from test_mesh_components_cpu import TORUS, pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config
from test_occlusion_cpu import CASES, NEAR, PROTOTYPE, VS, corner_analytic, corner_samples, corner_volume, plane, plane_samples

pytestmark = pytest.mark.gpu
RAY_SHARE = 2e-3
BAKE_KEYS = LOD_KEYS + ("uv", "width", "height", "albedo", "normal", "displacement", "voxel", "face", "n_texels", "n_hits", "n_hits_off_band", "n_buried", "n_misses")


def bits_of(mask, K):
    return ((np.asarray(mask, np.uint64)[..., None] >> np.arange(K, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def same_ao(a, b):
    """two results of an occlusion call: every array bit for bit, the counts equal"""
    same_bits(a, b, [k for k in a if k != "counts"])
    assert a["counts"] == b["counts"]


def popcount(mask):
    return bits_of(mask, 64).sum(-1)


def assert_planes_consistent(got, K, n_samples, valid):
    """what follows from the masks exactly: no bit at or above K, the bytes, the counts"""
    mask, occ = got["mask"], got["occlusion"]
    assert mask.dtype == np.uint64 and occ.dtype == np.uint8 and mask.shape == occ.shape
    if K < 64:
        assert not (mask >> np.uint64(K)).any()
    c = popcount(mask)
    assert np.array_equal(occ[valid], ((510 * (K - c[valid]) + K) // (2 * K)).astype(np.uint8))
    assert not mask[~valid].any()
    cn = got["counts"]
    assert tuple(cn) == oref.COUNTS
    assert cn["n_samples"] == n_samples and cn["n_valid"] == int(valid.sum()) and cn["n_rays"] == K * cn["n_valid"]
    assert cn["n_occluded"] == int(c.sum()) and 0 <= cn["n_buried"] <= cn["n_occluded"]
    assert got["dirs"].shape == (K, 3) and got["dirs"].dtype == np.float64 and np.abs(got["dirs"] - oref.dirs(K)).max() < 1e-15


@pytest.fixture(scope="module")
def corner(built):
    v, dim = corner_volume()
    return upload(v, dim, VS)


@pytest.mark.parametrize("K", oref.KS)
@pytest.mark.parametrize("bias,radius", CASES)
def test_corner_equals_the_analytic_mask(corner, K, bias, radius):
    eng = corner
    vs = vs_of(eng)
    q, m = corner_samples()
    got = eng.occlusion_points(q, m, K, radius * vs, bias * vs)
    bits, t, near = corner_analytic(q, K, bias * vs, radius * vs, got["dirs"])
    dev = bits_of(got["mask"], K)
    differ = (dev != bits) & ~near
    print(f"corner K {K} bias {bias} radius {radius}: {got['counts']['n_occluded']} of {got['counts']['n_rays']} rays occluded (analytic {int(bits.sum())}, prototype "
          f"{PROTOTYPE[(bias, radius)][oref.KS.index(K)]}), {int(differ.sum())} differ, {int(near.sum())} within {NEAR} vs of the radius, {got['counts']['n_buried']} buried")
    assert not differ.any()
    assert_planes_consistent(got, K, 141, np.ones(141, bool))
    assert got["counts"]["n_buried"] == 0
    if not near.any():
        assert got["counts"]["n_occluded"] == int(bits.sum())


@pytest.mark.parametrize("K", [8, 64])
def test_plane_is_open(built, K):
    v, dim, _ = plane()
    eng = upload(v, dim, VS)
    q, m = plane_samples()
    vs = vs_of(eng)
    got = eng.occlusion_points(q, m, K, 8 * vs, 0.25 * vs)
    assert_planes_consistent(got, K, 300, np.ones(300, bool))
    assert got["counts"]["n_occluded"] == 0 and got["counts"]["n_buried"] == 0 and (got["occlusion"] == 255).all()
    down = eng.occlusion_points(q, -m, K, 8 * vs, 0.25 * vs)      # into the plane: every origin is below the surface
    assert down["counts"]["n_occluded"] == down["counts"]["n_buried"] == 300 * K and not down["occlusion"].any()


def assert_bake_ao_matches_yardstick(eng, s, R, K, tag, radius_vs=8.0, bias_vs=1.0):
    vs = vs_of(eng)
    cell = s * vs
    plain = eng.bake_lod(cell, R)
    got = eng.bake_lod_ao(cell, R, None, K, radius_vs * vs, bias_vs * vs)
    same_bits(plain, got, BAKE_KEYS)                                  # the bake: psgsdf_bake_lod's, bit for bit
    v = eng.download_volume()
    dim = [int(x) for x in eng.info().dim]
    exp = oref.bake_ao(v, dim, vs, got, got, R, K, radius_vs * vs, bias_vs * vs, dirs=got["dirs"])
    own = got["face"] >= 0
    assert got["mask"].shape == got["occlusion"].shape == own.shape
    assert_planes_consistent({**got, "mask": got["mask"][own], "occlusion": got["occlusion"][own]}, K, int(own.sum()), exp["valid"][own])
    assert not got["mask"][~own].any() and not got["occlusion"][~own].any()      # padding
    assert (got["occlusion"][own & ~exp["valid"]] == 255).all()
    dev = bits_of(got["mask"], K)
    differ = dev != exp["bits"]
    share = differ.sum() / max(got["counts"]["n_rays"], 1)
    print(f"{tag} cell {s} vs, R {R}, K {K}: {got['counts']['n_samples']} texels, {got['counts']['n_valid']} valid, {got['counts']['n_rays']} rays, {got['counts']['n_occluded']} occluded "
          f"({got['counts']['n_occluded'] / max(got['counts']['n_rays'], 1):.2%}), {got['counts']['n_buried']} buried; yardstick {exp['n_occluded']} / {exp['n_buried']}; "
          f"{int(differ.sum())} rays differ ({share:.2e}); mean byte {got['occlusion'][own].mean():.1f}")
    assert got["counts"]["n_samples"] == got["n_texels"] and got["counts"]["n_valid"] == exp["n_valid"]
    assert share <= RAY_SHARE, (tag, share)
    # a buried ray is an occluded one whose t is 0: where every ray's bit agrees the walks agree, and so do the buried counts; otherwise they
    # can differ by the rays that differ
    assert abs(got["counts"]["n_buried"] - exp["n_buried"]) <= int(differ.sum())
    return got, exp


@pytest.fixture(scope="module")
def pieces(built):
    v, dim, vs = pieces_volume(torus=True)
    return upload(v, dim, vs)


@pytest.mark.parametrize("s,R,K", [(4, 3, 64), (2, 3, 16)])
def test_five_pieces_and_the_torus(pieces, s, R, K):
    got, exp = assert_bake_ao_matches_yardstick(pieces, s, R, K, "five pieces + torus")
    assert got["counts"]["n_occluded"] > 0 and got["counts"]["n_valid"] == got["counts"]["n_samples"]
    # the torus (axis z): the texels at its inner equator look across the hole, those at its outer equator into the open
    vs = vs_of(pieces)
    ct, Rt, rt = TORUS
    p = exp["q"] - np.array(ct) * 48 * vs
    rho = np.hypot(p[..., 0], p[..., 1])
    ring = (got["face"] >= 0) & (np.abs(np.hypot(rho - Rt * vs, p[..., 2]) - rt * vs) < vs) & (np.abs(p[..., 2]) < 0.8 * vs)
    inner, outer = ring & (rho < Rt * vs), ring & (rho > Rt * vs)
    print(f"torus equators: {int(inner.sum())} inner texels, mean byte {got['occlusion'][inner].mean():.1f}; {int(outer.sum())} outer, {got['occlusion'][outer].mean():.1f}")
    assert inner.sum() >= 8 and outer.sum() >= 8
    assert got["occlusion"][inner].mean() < got["occlusion"][outer].mean()


@pytest.fixture(scope="module")
def scene(built):
    return scene_engine("SH1")[0]


def test_synthetic_scene_normals_come_from_the_band(scene):
    got, exp = assert_bake_ao_matches_yardstick(scene, 2, 4, 16, "SH1")
    assert got["n_hits"] > 1000 and got["n_hits_off_band"] < got["n_hits"] and got["counts"]["n_rays"] == 16 * got["n_texels"]


def test_invalid_samples_and_no_samples(corner):
    eng = corner
    q, m = corner_samples()
    q, m = q[:70].copy(), m[:70].copy()
    q[3, 1] = np.nan; m[10] = 0; m[33, 2] = np.inf; q[64, 0] = -np.inf; m[69] = [np.nan, 0, 1]
    valid = np.ones(70, bool); valid[[3, 10, 33, 64, 69]] = False
    for K in (8, 64):
        got = eng.occlusion_points(q, m, K)
        assert_planes_consistent(got, K, 70, valid)
        assert (got["occlusion"][~valid] == 255).all()
        whole = eng.occlusion_points(*corner_samples(), K)
        assert np.array_equal(got["mask"][valid], whole["mask"][:70][valid])      # a sample does not depend on its neighbours in the wavefront
    none = eng.occlusion_points(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 32)
    assert none["mask"].shape == (0,) and none["occlusion"].shape == (0,) and np.abs(none["dirs"] - oref.dirs(32)).max() < 1e-15
    assert all(none["counts"][k] == 0 for k in oref.COUNTS)


def test_more_rays_than_one_launch_takes(corner):
    """2^26 + 5 points of 64 rays are 2^32 + 320 rays: more than a dispatch's 32-bit count of work-items, so they go out in five launches.  All but a
    few points are invalid (a zero normal costs no walk); the valid ones sit at the start, on both sides of every launch's first sample (2^24 j) and
    at the very end, and must get the masks they get in a small call."""
    eng = corner
    K, per = 64, (1 << 30) // 64
    n = 4 * per + 5
    q0, m0 = corner_samples()
    small = eng.occlusion_points(q0, m0, K)
    at = np.unique(np.concatenate([np.arange(0, 141)] + [np.arange(c * per - 3, c * per + 3) for c in range(1, 5)] + [np.arange(n - 5, n)]))
    q = np.zeros((n, 3), np.float32); m = np.zeros((n, 3), np.float32)
    q[at] = q0[at % 141]; m[at] = m0[at % 141]
    got = eng.occlusion_points(q, m, K)
    cn = got["counts"]
    assert cn["n_samples"] == n and cn["n_valid"] == len(at) and cn["n_rays"] == K * len(at)
    assert np.array_equal(got["mask"][at], small["mask"][at % 141]) and np.array_equal(got["occlusion"][at], small["occlusion"][at % 141])
    assert small["mask"][at % 141].any() and cn["n_occluded"] == int(popcount(small["mask"][at % 141]).sum())
    rest = np.ones(n, bool); rest[at] = False
    assert not got["mask"][rest].any() and (got["occlusion"][rest] == 255).all()


def test_a_shorter_radius_occludes_a_subset_and_the_cut_changes_no_bit(pieces, monkeypatch):
    eng = pieces
    vs = vs_of(eng)
    monkeypatch.setenv("PSGSDF_AO_CUT", "0")      # a context whose rays walk on to the end of the volume (the knob is read at creation)
    v, dim, _ = pieces_volume(torus=True)
    uncut = upload(v, dim, vs)
    monkeypatch.delenv("PSGSDF_AO_CUT")
    assert uncut.get_tuning()["effective"]["ao_cut"] == 0 and eng.get_tuning()["effective"]["ao_cut"] == 1
    xyz, nrm, _, _, _ = eng.extract_mesh_indexed()
    xyz, nrm = xyz[::5], nrm[::5]
    for K in (16, 64):
        r4, r8 = eng.occlusion_points(xyz, nrm, K, 4 * vs, vs), eng.occlusion_points(xyz, nrm, K, 8 * vs, vs)
        assert not (r4["mask"] & ~r8["mask"]).any() and 0 < r4["counts"]["n_occluded"] < r8["counts"]["n_occluded"] and r4["counts"]["n_buried"] == r8["counts"]["n_buried"]
        same_ao(r8, uncut.occlusion_points(xyz, nrm, K, 8 * vs, vs))    # without the cut: the same rays are occluded
        same_ao(r8, eng.occlusion_points(xyz, nrm, K, 8 * vs, vs))      # two calls: the same bits


def test_two_calls_same_bits_and_the_other_calls_undisturbed(scene):
    eng = scene
    vs = vs_of(eng)
    bake0, lod0, idx0, rep0 = eng.bake_lod(2 * vs, 4), eng.extract_mesh_lod(2 * vs), eng.extract_mesh_indexed(), eng.render_report()
    a, b = eng.bake_lod_ao(2 * vs, 4), eng.bake_lod_ao(2 * vs, 4)
    same_ao(a, b)
    pts = eng.occlusion_points(idx0[0], idx0[1], 32)
    same_ao(pts, eng.occlusion_points(idx0[0], idx0[1], 32))
    same_bits(bake0, eng.bake_lod(2 * vs, 4))
    same_bits(lod0, eng.extract_mesh_lod(2 * vs))
    for x, y in zip(idx0, eng.extract_mesh_indexed()):
        assert np.array_equal(x, y)
    assert rep0 == eng.render_report()
    c = eng.bake_lod_ao(2 * vs, 4, keep_largest=1)
    same_bits(eng.bake_lod(2 * vs, 4, keep_largest=1), c, BAKE_KEYS)


def test_a_call_between_two_iterations_changes_nothing(built):
    ends = []
    for ao in (False, True):
        sc = synth.make_scene(N=32, F=3, W=64, H=48, model="SH1")
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo()
        eng.iterate(capi.ALL, 1)
        if ao:
            assert eng.bake_lod_ao(2 * vs_of(eng), 4)["counts"]["n_rays"] > 16000
            xyz, nrm, _, _, _ = eng.extract_mesh_indexed()
            assert eng.occlusion_points(xyz, nrm)["counts"]["n_valid"] == len(xyz)
        eng.iterate(capi.ALL, 1)
        v = eng.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], eng.download_poses(), eng.download_light()))
    for x, y in zip(*ends):
        assert x.tobytes() == y.tobytes()


def test_errors_and_the_empty_mesh(pieces):
    eng = pieces
    vs = vs_of(eng)
    q, m = corner_samples()
    for kw in (dict(n_dirs=12), dict(n_dirs=0), dict(n_dirs=128), dict(radius=0.0), dict(radius=float("nan")), dict(bias=-vs), dict(bias=float("inf"))):
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # PSGSDF_ERR_ARG
            eng.occlusion_points(q, m, **kw)
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):
            eng.bake_lod_ao(2 * vs, 4, **kw)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):          # what psgsdf_bake_lod refuses
        eng.bake_lod_ao(2 * vs, 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.bake_lod_ao(2 * vs, 4, float("nan"))
    with pytest.raises(capi.PsgsdfError, match="rc=-3"):          # PSGSDF_ERR_UNSUPPORTED: the atlas
        eng.bake_lod_ao(2 * vs, 600)
    got = eng.bake_lod_ao(64 * vs, 4, n_dirs=8)                   # everything in one cluster: an empty level-of-detail mesh
    assert got["width"] == 0 and got["mask"].shape == (0, 0) and got["occlusion"].shape == (0, 0) and all(got["counts"][k] == 0 for k in oref.COUNTS)
    assert np.abs(got["dirs"] - oref.dirs(8)).max() < 1e-15
    assert eng.bake_lod_ao(4 * vs, 2)["counts"]["n_rays"] > 0               # the context still works
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    fresh = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):          # PSGSDF_ERR_STATE: no volume yet
        fresh.occlusion_points(q, m)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):
        fresh.bake_lod_ao(0.1, 4)


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "occlusion")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 3
    for e, name in zip(res[1]["errors"], ("occlusion_points", "bake_lod_ao", "bake_lod_ao")):
        assert "rc=-3" in e and "rank 1 of 2" in e and name in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_mesh_bake_ao(built, tmp_path):
    from PIL import Image
    from test_bake_cpu import read_mtl
    import _bake_ref as bref
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    for name, extra in (("bake", ["--mesh-lod", "2", "--mesh-bake", "4"]), ("ao", ["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "16"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    bake = sorted(f for f in os.listdir(outs["bake"]) if f not in skip)
    meshes = [f[:-len("_mesh_lod.ply")] for f in bake if f.endswith("_mesh_lod.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    # without the flag: the files of --mesh-bake as they were, nothing of the new map
    assert sorted(f for f in bake if "_mesh_lod" in f) == sorted(m + s for m in meshes for s in ("_mesh_lod.ply", "_mesh_lod.obj", "_mesh_lod.mtl", "_mesh_lod_albedo.png", "_mesh_lod_normal.png"))
    for m in meshes:
        assert "map_Ka" not in open(outs["bake"] + m + "_mesh_lod.mtl").read()
    assert sorted(f for f in os.listdir(outs["ao"]) if f not in skip) == sorted(bake + [m + "_mesh_lod_ao.png" for m in meshes])      # the only new files
    for f in bake:      # the flag changes no other file but the material, which gains one line
        if f.endswith("_mesh_lod.mtl"):
            assert open(outs["ao"] + f).read() == open(outs["bake"] + f).read() + "map_Ka " + f[:-len(".mtl")] + "_ao.png\n", f
        else:
            assert filecmp.cmp(outs["bake"] + f, outs["ao"] + f, shallow=False), f
    for m in meshes:
        base = outs["ao"] + m + "_mesh_lod"
        _, _, faces = read_ply_indexed(base + ".ply")
        L = bref.layout(len(faces), 4)
        assert read_mtl(base + ".mtl")["map_Ka"] == m + "_mesh_lod_ao.png"
        im = Image.open(base + "_ao.png")
        px = np.asarray(im)
        assert im.mode == "L" and px.shape == (L["H"], L["W"])
        own = L["face"] >= 0
        print(f"{m}: atlas {L['W']} x {L['H']}, {int(own.sum())} texels, occlusion byte {px[own].min()} .. {px[own].max()}, mean {px[own].mean():.1f}")
        assert not px[~own].any() and px[own].max() == 255 and px[own].min() < 255
        assert set(np.unique(px[own]).tolist()) <= {oref.byte(16, c) for c in range(17)}
