"""The albedo texture solved from the keyframes, without a GPU (include/psgsdf_photo.h): the yardstick tests/_photo_ref.py alone, on
synthetic scenes' own volumes, poses and lights, with the bake's planes from tests/_bake_ref.py.
  (a) the count identities;
  (b) the share of (texel, keyframe) pairs whose status differs between the yardstick's float32 and float64 modes is at most 1e-3: the reference alone
      stays inside the cap of the device test (2e-3, the project's cap for float32 against float64 walks);
  (c) E = max |photo_f32 - photo_f64| over the texels whose statuses all agree is printed: the device test takes its tolerance, 4 E, from the same
      two modes on its own inputs;
  (d) the quality claim: with an albedo pattern of 12 cycles across the extent (2.7 voxels a period at N = 32, 160 x 120 keyframes: a pixel covers
      about a third of a voxel) the photo map's rms error against the true albedo is smaller than the voxel map's.
Then the header as C99, the exported symbol and struct sizes, the call's returns without a context, voxelPS's refusals and the kernels' resources."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _bake_ref as bref
import _photo_ref as pref
from psgradientsdf_amd import synth
from test_mesh_components_cpu import EXE, HIPCC, ROOT

f32 = np.float32
STATUS_SHARE = 1e-3
CASES = {      # scene, cell in voxels, R, the call's parameters
    "SH1": (dict(N=32, F=3, W=64, H=48, model="SH1"), 2, 4, {}),
    "SH2": (dict(N=32, F=3, W=64, H=48, model="SH2"), 2, 4, {}),
    "LED": (dict(N=32, F=3, W=64, H=48, model="LED"), 2, 4, {}),
    "far side": (dict(N=32, F=3, W=64, H=48, model="SH1"), 2, 4, dict(cos_min=-1.0)),
    "cropped": (dict(N=32, F=3, W=64, H=16, model="SH1", arc=90.0), 2, 4, {}),      # strips of 16 rows from cameras 30 degrees apart: each sees surface the others crop
}


def scene_inputs(sc):
    """what the yardstick takes of a synthetic scene: the volume, the grid, the keyframes with the poses and lights the optimiser would start from"""
    vs = float(f32(sc.voxel_size))
    dim = [int(x) for x in sc.dim]
    origin = [f32(sc.shift[a]) - f32(0.5 * vs) * f32(dim[a]) for a in range(3)]      # api.hip: the engine's own float arithmetic
    v = dict(dist=sc.dist, grad=sc.grad, weight=sc.weight, rgb=sc.rgb)
    intr = (sc.K[0], sc.K[4], sc.K[2], sc.K[5])
    return dict(v=v, dim=dim, vs=vs, origin=origin, poses=sc.poses, light=sc.light_gt, images=sc.images, intr=intr, model=sc.model_id)


def both_modes(inp, cell_vs, R, loss=1, lam=0.2, **params):
    vs = inp["vs"]
    mesh = bref.lod_mesh(inp["v"], inp["dim"], vs, cell_vs * vs)
    planes = bref.bake(inp["v"], inp["dim"], vs, mesh, R, cell_vs * vs)
    params.setdefault("bias", vs)
    out = [pref.photo(inp["v"], inp["dim"], vs, inp["origin"], mesh, planes, R, inp["poses"], inp["light"], inp["images"], inp["intr"], inp["model"], loss, lam, mode=m, **params)
           for m in ("f32", "f64")]
    return out[0], out[1], planes


@functools.lru_cache(maxsize=None)
def case(name):
    kw, cell_vs, R, params = CASES[name]
    return both_modes(scene_inputs(synth.make_scene(**kw)), cell_vs, R, **params)


@pytest.mark.parametrize("name", list(CASES))
def test_count_identities_and_the_untouched_texels(name):
    for r, planes in ((case(name)[0], case(name)[2]), (case(name)[1], case(name)[2])):
        k, st = r["counts"], r["status"]
        F = st.shape[0]
        smp = r["sample"]
        assert np.array_equal(smp, (planes["face"] >= 0) & (planes["voxel"] >= 0)) and k["n_samples"] == int(smp.sum()) > 1000
        assert k["n_pairs"] == k["n_samples"] * F == k["n_used"] + k["n_outside"] + k["n_grazing"] + k["n_occluded"] + k["n_dark"]
        assert 0 <= k["n_buried"] <= k["n_occluded"]
        assert (st[:, ~smp] == pref.NO_SAMPLE).all() and (st[:, smp] <= pref.DARK).all()
        assert np.array_equal(r["n_obs"], (st == pref.USED).sum(0)) and k["n_texels_solved"] == int((r["n_obs"] > 0).sum()) > 0
        # missed, buried and padding texels keep the bake's albedo; padding stays zero
        rest = ~smp
        assert np.array_equal(r["photo_rgb"][rest], planes["albedo"][rest]) and np.array_equal(r["photo"][rest], (planes["albedo"][rest].astype(np.float64) / 255.0).astype(f32))
        pad = planes["face"] < 0
        assert not r["photo"][pad].any() and not r["photo_rgb"][pad].any() and not r["n_obs"][pad].any()
        assert np.array_equal(r["photo_rgb"][smp], bref.colour_byte(r["photo"][smp]))
        unsolved = smp & (r["n_obs"] == 0)
        assert np.array_equal(r["photo_rgb"][unsolved], planes["albedo"][unsolved])


@pytest.mark.parametrize("name", list(CASES))
def test_float32_and_float64_yardsticks_agree(name):
    a, b, _ = case(name)
    share, E, agree = pref.compare_modes(a, b)
    k = a["counts"]
    print(f"{name}: {k['n_samples']} samples x {a['status'].shape[0]} keyframes: used {k['n_used']}, outside {k['n_outside']}, grazing {k['n_grazing']}, occluded {k['n_occluded']} "
          f"({k['n_buried']} buried), dark {k['n_dark']}; another status in the float64 mode on {share:.2e} of the pairs; E = {E:.3e} over {int(agree.sum())} texels")
    assert share <= STATUS_SHARE, (name, share)
    assert np.array_equal(a["n_obs"][agree], b["n_obs"][agree])
    assert 0 < E < 1e-4, (name, E)      # float32 rounding of values of order 1: a few 1e-7 per step, amplified where the shading is small


def test_the_cases_reach_what_the_device_test_needs_of_them():
    far, crop = case("far side")[0]["counts"], case("cropped")[0]["counts"]
    assert far["n_occluded"] > 0.2 * far["n_pairs"] and far["n_buried"] > 0
    assert crop["n_outside"] >= 0.05 * crop["n_pairs"]
    seen = set()
    for name in CASES:
        seen |= set(np.unique(case(name)[0]["status"]).tolist())
    assert seen == {pref.USED, pref.OUTSIDE, pref.GRAZING, pref.OCCLUDED, pref.DARK, pref.NO_SAMPLE}, seen


def fine_albedo(x, c, L):
    """synth._albedo with 12 cycles across the extent instead of 1.5"""
    q = (x - c) / L
    k = 2 * np.pi * 12.0
    a = np.stack([np.sin(k * q[..., 0] + 0.3) * np.cos(k * q[..., 1]), np.sin(k * q[..., 1] + 1.1) * np.cos(k * q[..., 2]), np.sin(k * q[..., 2] + 2.3) * np.cos(k * q[..., 0])], -1)
    return 0.55 + 0.35 * a


def test_photo_map_beats_the_voxel_map_on_a_fine_pattern(monkeypatch):
    monkeypatch.setattr(synth, "_albedo", fine_albedo)
    sc = synth.make_scene(N=32, F=6, W=160, H=120, model="SH1")
    inp = scene_inputs(sc)
    r, _, planes = both_modes(inp, 2, 4)
    solved = r["n_obs"] > 0
    truth = fine_albedo(r["xw"][solved], sc.shift.astype(np.float64), sc.extent)
    e_photo = pref.gain_rms(r["photo"][solved], truth)
    e_voxel = pref.gain_rms(planes["albedo"][solved].astype(np.float64) / 255.0, truth)
    print(f"12 cycles across the extent, N = 32, 6 keyframes of 160 x 120: {int(solved.sum())} solved texels, rms error of the photo map {e_photo:.4f}, of the voxel map {e_voxel:.4f}")
    assert int(solved.sum()) > 5000
    assert e_photo < e_voxel


def test_yardstick_refuses_bad_parameters():
    for bad in (dict(bias=0.0), dict(bias=float("nan")), dict(bias=float("inf")), dict(cos_min=1.0), dict(cos_min=-1.5), dict(cos_min=float("nan")),
                dict(shade_min=0.0), dict(shade_min=float("inf"))):
        kw = dict(bias=0.01, cos_min=0.2, shade_min=0.05); kw.update(bad)
        with pytest.raises(ValueError):
            pref.check_params(**kw)
    pref.check_params(0.01, -1.0, 0.05)


def test_library_exports_the_call(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_photo.h") == ["psgsdf_bake_lod_photo"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        assert hasattr(ctypes.CDLL(path), "psgsdf_bake_lod_photo"), path
    assert hasattr(capi.Api, "bake_lod_photo")
    assert (ctypes.sizeof(capi.PhotoParams), ctypes.sizeof(capi.PhotoCounts), ctypes.sizeof(capi.BakePhoto)) == (32, 72, ctypes.sizeof(capi.Bake) + 32 + 8 + 72)
    assert (capi.PHOTO_USED, capi.PHOTO_OUTSIDE, capi.PHOTO_GRAZING, capi.PHOTO_OCCLUDED, capi.PHOTO_DARK, capi.PHOTO_NO_SAMPLE) == (0, 1, 2, 3, 4, 255)
    fn = ctypes.CDLL(capi.ENGINE_LIB).psgsdf_bake_lod_photo
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    par, out = capi.PhotoParams(0.01, 0.2, 0.05, 0, 0), capi.BakePhoto()
    out.n_frames = 77
    ARG, STATE = -1, -4
    assert fn(None, None, 0.02, 4, 0.02, ctypes.byref(par), None) == ARG and fn(None, None, 0.02, 4, 0.02, None, ctypes.byref(out)) == ARG
    assert fn(None, None, 0.02, 0, 0.02, ctypes.byref(par), ctypes.byref(out)) == ARG      # the bake's own refusal comes first
    assert fn(None, None, 0.02, 4, 0.02, ctypes.byref(par), ctypes.byref(out)) == STATE    # nothing to solve from
    assert out.n_frames == 77      # refused calls leave the outputs untouched


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_photo.c"
    src.write_text('#include "psgsdf_photo.h"\n'
                   'typedef char params_size[sizeof(psgsdf_photo_params) == 32 ? 1 : -1];\ntypedef char counts_size[sizeof(psgsdf_photo_counts) == 72 ? 1 : -1];\n'
                   'typedef char result_size[sizeof(psgsdf_bake_photo) == sizeof(psgsdf_bake) + 112 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, double cell) {\n    psgsdf_photo_params p; psgsdf_bake_photo b; int rc;\n'
                   '    p.bias = 0.01; p.cos_min = 0.2; p.shade_min = 0.05; p.want_status = 1; p.reserved = 0;\n    rc = psgsdf_bake_lod_photo(c, 0, cell, 4, cell, &p, &b);\n'
                   '    if (rc) return rc;\n    return (int)(b.counts.n_used + b.n_obs[0] + b.photo_rgb[0] + (b.status[0] == PSGSDF_PHOTO_NO_SAMPLE) + PSGSDF_PHOTO_USED + PSGSDF_PHOTO_OUTSIDE\n'
                   '                 + PSGSDF_PHOTO_GRAZING + PSGSDF_PHOTO_OCCLUDED + PSGSDF_PHOTO_DARK + (b.photo[0] > 0.5f) + b.bake.width);\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_photo.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_voxelps_refuses_the_photo_map_without_a_bake_and_on_several_gpus(built, tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    for extra, words in ((["--mesh-lod", "2", "--mesh-bake-photo"], ("--mesh-bake-photo needs --mesh-bake",)),
                         (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-photo", "--gpus", "2"], ("--mesh-bake-photo needs a single process", "--gpus 2"))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


def test_photo_kernels_use_no_scratch_and_no_float_atomics(built, tmp_path):
    from test_kernel_resources import resources
    ks = resources("photo.hip", tmp_path)
    pairs = {k: v for k, v in ks.items() if "k_photo_pairs" in k}
    solve = {k: v for k, v in ks.items() if "k_photo_solve" in k}
    assert len(pairs) == 3 and len(solve) == 9, sorted(ks)      # the models; the models x {float taps, RGBA8 words, decided by the source}
    assert all(v["scratch"] == 0 and v["vgpr"] <= 72 for v in pairs.values()), pairs      # the walk at 7 wavefronts per SIMD
    assert all(v["scratch"] == 0 and v["vgpr"] <= 80 for v in solve.values()), solve
    src = open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "photo.hip")).read()
    assert "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src and src.count("__shared__") == 0      # (dynamic LDS: the frame records)
    for fn in ("project(", "sample<false, IMG>(", "rendered<MODEL>(", "robust_weight(", "render_trace<false, true>(", "bake_sample(", "load_frames("):
        assert fn in src, fn      # one copy of the arithmetic: the energy's, the renderer's and the bake's own functions
