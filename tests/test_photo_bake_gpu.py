"""The albedo texture solved from the keyframes on the device (include/psgsdf_photo.h psgsdf_bake_lod_photo, csrc/photo.hip), against
the yardstick tests/_photo_ref.py (float32 mode) on the context's own downloaded state, its own level-of-detail mesh and its own bake.
Per case: the bake is psgsdf_bake_lod's bit for bit; at most 2e-3 of the (texel, keyframe) pairs have another status (test_bake_gpu.VOXEL_SHARE, the
project's cap for float32 against float64 walks); on the texels whose statuses all agree n_obs is equal, |photo - yardstick| <= 4 E and the bytes
are within 1, where E = max |photo_f32 - photo_f64| of the yardstick's two modes on the case's own inputs (never the device's output; the factor 4
allows for v_rcp_f32 in the Cauchy weight and the 1-ulp reciprocal in project); the counts are the sums over the planes; padding is zero.
Then the quality claim on the device, repeatability, no effect on the optimisation or on later calls, the errors, and voxelPS --mesh-bake-photo."""
import ctypes
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

import _bake_ref as bref
import _photo_ref as pref
from psgradientsdf_amd import capi, synth
from test_bake_gpu import VOXEL_SHARE, same_bits
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config
from test_photo_bake_cpu import fine_albedo

pytestmark = pytest.mark.gpu
f32 = np.float32
BAKE_KEYS = ("xyz", "normals", "rgb", "faces", "vertex_map", "n_vertices_in", "n_faces_in", "uv", "width", "height", "albedo", "normal", "displacement", "voxel", "face",
             "n_texels", "n_hits", "n_hits_off_band", "n_buried", "n_misses")
SCENE = dict(N=32, F=3, W=64, H=48)
CASES = {      # scene, upsample2x, the call's parameters
    "SH1": (dict(SCENE, model="SH1"), False, {}),
    "SH2": (dict(SCENE, model="SH2"), False, {}),
    "LED": (dict(SCENE, model="LED"), False, {}),
    "u8": (dict(SCENE, model="SH1", u8=True), False, {}),                       # the RGBA8 instance of the sampler
    "refined": (dict(SCENE, model="SH1"), True, {}),
    "far side": (dict(SCENE, model="SH1"), False, dict(cos_min=-1.0)),          # the far side reaches the ray: occluded and buried in bulk
    "cropped": (dict(SCENE, model="SH1", H=16, arc=90.0), False, {}),           # test_photo_bake_cpu: 11 % of the pairs outside
}


def engine(scene_kw, refine=False, iters=2):
    sc = synth.make_scene(**scene_kw)
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.load_scene(sc)
    eng.init_albedo()
    if iters:
        eng.iterate(capi.ALL, iters)
    if refine:
        eng.upsample2x()
    return eng, sc


def yardstick(eng, sc, got, R, mode, **params):
    """the yardstick on the context's downloaded state, the device's own level-of-detail mesh and bake"""
    info = eng.info()
    vs = vs_of(eng)
    st = capi.default_settings(sc.model_id)
    params.setdefault("bias", vs)
    return pref.photo(eng.download_volume(), [int(x) for x in info.dim], vs, [float(x) for x in info.origin], got, got, R, eng.download_poses(), eng.download_light(),
                      sc.images, (sc.K[0], sc.K[4], sc.K[2], sc.K[5]), sc.model_id, int(st.loss), float(st.lambda_), mode=mode, **params)


@functools.lru_cache(maxsize=None)
def parity(name, s=2, R=4):
    """one case: the device's result, the two yardsticks, and the per-case checks"""
    scene_kw, refine, params = CASES[name]
    eng, sc = engine(scene_kw, refine)
    vs = vs_of(eng)
    got = eng.bake_lod_photo(s * vs, R, status=True, **params)
    same_bits(eng.bake_lod(s * vs, R), got, BAKE_KEYS)                      # the bake: psgsdf_bake_lod's, bit for bit
    a, b = (yardstick(eng, sc, got, R, m, **params) for m in ("f32", "f64"))
    ref_share, E, _ = pref.compare_modes(a, b)
    F = sc.F
    k, st = got["counts"], got["status"]
    assert st.shape == (F,) + got["face"].shape and st.dtype == np.uint8
    smp = a["sample"]
    assert np.array_equal(st != pref.NO_SAMPLE, np.broadcast_to(smp, st.shape))      # the samples: owned texels with a hit, for every frame
    differ = st != a["status"]
    share = differ.sum() / max(int(smp.sum()) * F, 1)
    agree = smp & ~differ.any(0)
    err = float(np.abs(got["photo"][agree].astype(np.float64) - a["photo"][agree].astype(np.float64)).max())
    rgb_err = int(np.abs(got["photo_rgb"][agree].astype(np.int32) - a["photo_rgb"][agree].astype(np.int32)).max())
    print(f"{name}: {got['width']} x {got['height']}, {k['n_samples']} samples x {F} keyframes: used {k['n_used']}, outside {k['n_outside']}, grazing {k['n_grazing']}, "
          f"occluded {k['n_occluded']} ({k['n_buried']} buried), dark {k['n_dark']}, {k['n_texels_solved']} texels solved; another status on {int(differ.sum())} pairs ({share:.2e}; "
          f"the yardstick's two modes: {ref_share:.2e}); |photo - yardstick| max {err:.3e} = {err / E:.2f} E (E = {E:.3e}), bytes within {rgb_err}")
    assert share <= VOXEL_SHARE, (name, share)
    assert np.array_equal(got["n_obs"][agree], a["n_obs"][agree])
    assert err <= 4 * E, (name, err, E)
    assert rgb_err <= 1
    # texels without a sample keep the bake's albedo; padding is zero
    rest = ~smp
    assert np.array_equal(got["photo_rgb"][rest], got["albedo"][rest]) and np.array_equal(got["photo"][rest], (got["albedo"][rest].astype(np.float64) / 255.0).astype(f32))
    pad = got["face"] < 0
    assert not got["photo"][pad].any() and not got["photo_rgb"][pad].any() and not got["n_obs"][pad].any() and (st[:, pad] == pref.NO_SAMPLE).all()
    # the counts are the sums over the planes
    assert k["n_samples"] == int(smp.sum()) and k["n_pairs"] == k["n_samples"] * F == k["n_used"] + k["n_outside"] + k["n_grazing"] + k["n_occluded"] + k["n_dark"]
    for key, code in (("n_used", pref.USED), ("n_outside", pref.OUTSIDE), ("n_grazing", pref.GRAZING), ("n_occluded", pref.OCCLUDED), ("n_dark", pref.DARK)):
        assert k[key] == int((st == code).sum()), key
    assert np.array_equal(got["n_obs"], (st == pref.USED).sum(0)) and k["n_texels_solved"] == int((got["n_obs"] > 0).sum())
    assert 0 <= k["n_buried"] <= k["n_occluded"] and abs(k["n_buried"] - a["counts"]["n_buried"]) <= int(differ.sum())
    return got, a, err / E


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_yardstick(built, name):
    got, _, _ = parity(name)
    k = got["counts"]
    assert k["n_samples"] > 1000 and k["n_texels_solved"] > 0.5 * k["n_samples"]
    if name == "far side":
        assert k["n_occluded"] > 0.2 * k["n_pairs"] and k["n_buried"] > 0 and k["n_grazing"] == 0
    if name == "cropped":
        assert k["n_outside"] >= 0.05 * k["n_pairs"]


def test_every_status_occurs_somewhere(built):
    seen = set()
    for name in CASES:
        seen |= set(np.unique(parity(name)[0]["status"]).tolist())
    assert seen == {pref.USED, pref.OUTSIDE, pref.GRAZING, pref.OCCLUDED, pref.DARK, pref.NO_SAMPLE}, seen
    print("largest |photo - yardstick| / E over the cases:", max(parity(name)[2] for name in CASES))


def test_photo_map_beats_the_voxel_map_on_a_fine_pattern(built, monkeypatch):
    """test_photo_bake_cpu's claim on the device, after init_albedo and two iterations: both maps against the true albedo at the texels' world points,
    each with its own least-squares gain per channel"""
    monkeypatch.setattr(synth, "_albedo", fine_albedo)
    eng, sc = engine(dict(N=32, F=6, W=160, H=120, model="SH1"))
    got = eng.bake_lod_photo(2 * vs_of(eng), 4)
    assert got["status"] is None
    smp, _, _, _, _, _, xw = pref.sample_points(got, got, 4, [float(x) for x in eng.info().origin])
    solved = got["n_obs"].ravel()[smp] > 0
    truth = fine_albedo(xw[solved], sc.shift.astype(np.float64), sc.extent)
    e_photo = pref.gain_rms(got["photo"].reshape(-1, 3)[smp][solved], truth)
    e_voxel = pref.gain_rms(got["albedo"].reshape(-1, 3)[smp][solved].astype(np.float64) / 255.0, truth)
    print(f"12 cycles across the extent, N = 32, 6 keyframes of 160 x 120, two iterations: {int(solved.sum())} solved texels, rms error of the photo map {e_photo:.4f}, "
          f"of the voxel map {e_voxel:.4f}")
    assert int(solved.sum()) > 5000
    assert e_photo < e_voxel


def test_two_calls_same_bits_and_the_other_calls_undisturbed(built):
    eng, sc = engine(dict(SCENE, model="SH1"))
    vs = vs_of(eng)
    bake0, lod0, rep0 = eng.bake_lod(2 * vs, 4), eng.extract_mesh_lod(2 * vs), eng.render_report()
    a, b = eng.bake_lod_photo(2 * vs, 4, status=True), eng.bake_lod_photo(2 * vs, 4, status=True)
    same_bits({k: v for k, v in a.items() if k != "counts"}, {k: v for k, v in b.items() if k != "counts"})
    assert a["counts"] == b["counts"]
    c = eng.bake_lod_photo(2 * vs, 4)      # without the status plane: the bytes go through the scratch buffer, the maps are the same
    assert c["status"] is None and c["counts"] == a["counts"]
    same_bits(a, c, ("photo", "photo_rgb", "n_obs") + BAKE_KEYS)
    same_bits(bake0, eng.bake_lod(2 * vs, 4))
    same_bits(lod0, eng.extract_mesh_lod(2 * vs))
    assert rep0 == eng.render_report()


def test_a_call_between_two_iterations_changes_nothing(built):
    ends = []
    for photo in (False, True):
        sc = synth.make_scene(**dict(SCENE, model="SH1"))
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo()
        eng.iterate(capi.ALL, 1)
        if photo:
            assert eng.bake_lod_photo(2 * vs_of(eng), 4)["counts"]["n_used"] > 1000
        eng.iterate(capi.ALL, 1)
        v = eng.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], eng.download_poses(), eng.download_light()))
    for x, y in zip(*ends):
        assert x.tobytes() == y.tobytes()


def raw_call(eng, cell, res, reach, params, out):
    fn = eng._fn("bake_lod_photo")
    return fn(eng.ctx, None, ctypes.c_double(cell), ctypes.c_int32(res), ctypes.c_double(reach), ctypes.byref(params) if params is not None else None,
              ctypes.byref(out) if out is not None else None)


def test_errors_and_the_empty_mesh(built):
    eng, sc = engine(dict(N=32, F=6, W=64, H=48, model="SH1"), iters=0)
    vs = vs_of(eng)
    ARG, UNSUPPORTED, STATE = -1, -3, -4
    good = lambda: capi.PhotoParams(vs, 0.2, 0.05, 0, 0)
    out = capi.BakePhoto(); out.n_frames = 77
    assert raw_call(eng, 2 * vs, 4, 2 * vs, None, out) == ARG and raw_call(eng, 2 * vs, 4, 2 * vs, good(), None) == ARG      # NULL pointers
    for field, values in (("bias", (0.0, -1.0, float("nan"), float("inf"))), ("cos_min", (1.0, -1.5, float("nan"), float("inf"))), ("shade_min", (0.0, -0.1, float("nan"), float("inf"))),
                          ("want_status", (2, -1)), ("reserved", (1,))):
        for x in values:
            p = good(); setattr(p, field, x)
            assert raw_call(eng, 2 * vs, 4, 2 * vs, p, out) == ARG, (field, x)
    for cell, res, reach in ((2 * vs, 0, 2 * vs), (2 * vs, 4, 0.0), (2 * vs, 4, float("nan")), (2 * vs, 4, float("inf")), (0.0, 4, vs), (float("nan"), 4, vs)):      # what the bake refuses
        assert raw_call(eng, cell, res, reach, good(), out) == ARG, (cell, res, reach)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.bake_lod_photo(2 * vs, 4, keep_largest=-1)
    assert out.n_frames == 77 and not out.photo and out.bake.width == 0      # refused arguments leave the outputs untouched
    with pytest.raises(capi.PsgsdfError, match="rc=-3.*16384"):      # the bake's own limit
        eng.bake_lod_photo(2 * vs, 16384)
    # the widest atlas the bake allows, with a status plane: 6 keyframes x W x H texels are more than 2^30 bytes; refused before the atlas is allocated
    L1 = bref.layout(len(eng.extract_mesh_lod(2 * vs)["faces"]), 1)
    B = 16384 // L1["bpr"]
    assert 6 * (L1["W"] // 2 * B) * (L1["H"] // 2 * B) > 2 ** 30
    with pytest.raises(capi.PsgsdfError, match="rc=-3.*status"):
        eng.bake_lod_photo(2 * vs, B - 1, status=True)
    got = eng.bake_lod_photo(64 * vs, 4, status=True)      # everything in one cluster: an empty level-of-detail mesh
    assert got["width"] == 0 and got["height"] == 0 and len(got["faces"]) == 0 and got["photo"].shape == (0, 0, 3) and got["photo_rgb"].shape == (0, 0, 3)
    assert got["n_obs"].shape == (0, 0) and got["status"].shape == (6, 0, 0) and all(v == 0 for v in got["counts"].values())
    assert eng.bake_lod_photo(2 * vs, 4)["counts"]["n_used"] > 1000      # the context still works
    # before psgsdf_init: no context state at all, and a volume alone (the bake itself is valid there)
    fresh = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):
        fresh.bake_lod_photo(2 * vs, 4)
    v, dim, pvs = pieces_volume()
    uploaded = upload(v, dim, pvs)
    assert uploaded.bake_lod(2 * pvs, 4)["n_hits"] > 1000
    with pytest.raises(capi.PsgsdfError, match="rc=-4.*init first"):
        uploaded.bake_lod_photo(2 * pvs, 4)
    assert (ARG, UNSUPPORTED, STATE) == (-1, -3, -4)


def test_voxelps_mesh_bake_photo(built, tmp_path):
    from PIL import Image
    from test_bake_cpu import read_mtl
    outs = {}
    for name, extra in (("bake", ["--mesh-lod", "2", "--mesh-bake", "4"]), ("photo", ["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-photo"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    base = sorted(f for f in os.listdir(outs["bake"]) if f not in skip)
    meshes = [f[:-len("_mesh_lod.ply")] for f in base if f.endswith("_mesh_lod.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    # the fused volume's dump is taken before the optimiser holds the keyframes: baked as without the flag
    solved = [m for m in meshes if m != "init"]
    assert sorted(f for f in os.listdir(outs["photo"]) if f not in skip) == sorted(base + [m + "_mesh_lod_photo.png" for m in solved])      # the only new files
    for f in base:      # the flag changes no other file but the material, whose map_Kd names the photo map
        if f.endswith("_mesh_lod.mtl") and f != "init_mesh_lod.mtl":
            continue
        assert filecmp.cmp(outs["bake"] + f, outs["photo"] + f, shallow=False), f
    for m in solved:
        was, now = read_mtl(outs["bake"] + m + "_mesh_lod.mtl"), read_mtl(outs["photo"] + m + "_mesh_lod.mtl")
        assert was["map_Kd"] == m + "_mesh_lod_albedo.png" and now["map_Kd"] == m + "_mesh_lod_photo.png"
        assert {k: v for k, v in was.items() if k != "map_Kd"} == {k: v for k, v in now.items() if k != "map_Kd"}
        pho, alb = (np.asarray(Image.open(outs["photo"] + m + "_mesh_lod" + s).convert("RGB")) for s in ("_photo.png", "_albedo.png"))
        ply = open(outs["photo"] + m + "_mesh_lod.ply", "rb").read(2000).decode("latin1")
        L = bref.layout(int(ply.split("element face ")[1].split()[0]), 4)
        own = L["face"] >= 0
        assert pho.shape == alb.shape == (L["H"], L["W"], 3) and not pho[~own].any() and pho[own].max() > 0
        changed = (pho != alb).any(2)
        print(f"{m}: atlas {L['W']} x {L['H']}, {int(own.sum())} texels, the photo map differs from the voxel map on {int(changed.sum())}")
        assert changed.sum() > 0.3 * own.sum()
