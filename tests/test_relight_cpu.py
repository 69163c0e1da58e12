"""Relighting without a GPU (include/psgsdf_relight.h): the yardstick tests/_relight_ref.py against closed-form geometry -- the floor
meeting a wall of test_occlusion_cpu, seen by a camera, where a shadow ray is occluded iff it reaches the wall's plane within its limit -- for
directional lights with and without a spread, and for point lights in front of and behind the wall; the header as C99, the exported symbol and the
struct sizes, the call's returns without a context, the refusals of `voxelPS --relight` and the new kernel's resources."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _relight_ref as lref
import _render_ref as rref
from test_mesh_components_cpu import EXE, HIPCC, ROOT
from test_occlusion_cpu import VS, VS32, X0, Z0, corner_volume

f32 = np.float32
NEAR = 1e-3                                          # rays whose analytic parameter is this close (in voxels) to their limit are not compared
NEAR_SHARE = 0.01                                    # ... and they may be at most this share of the rays
W, H, FOCAL = 64, 48, 60.0
INTR = (FOCAL, FOCAL, (W - 1) / 2.0, (H - 1) / 2.0)


def P(x, y, z, origin=(0.0, 0.0, 0.0)):
    """a position given in voxels of the corner volume, in the world of a volume whose voxel (0, 0, 0) sits at `origin`"""
    return [float(f32(np.float64(o) + a * VS32)) for a, o in zip((x, y, z), origin)]


def corner_pose(origin=(0.0, 0.0, 0.0)):
    o = np.asarray(origin, np.float64)
    return rref.look_at(o + np.array([X0 + 15, 24, Z0 + 18]) * VS32, o + np.array([X0 + 6, 24, Z0]) * VS32, up=(0.0, 1.0, 0.0)).astype(f32)


def corner_cases(origin=(0.0, 0.0, 0.0)):
    """(name, light, bias, reach in voxels, expected (occluded rays, rays, shadowed pixels or None) of the float64 run of the definition)"""
    sun, front, behind = [-0.6, 0.1, 0.55], P(X0 + 4, 24, Z0 + 4, origin), P(X0 - 4, 20, Z0 + 6, origin)
    return [("sun", dict(kind="directional", vec=sun), 1.0, 12.0, (1056, 2208, 1056)),
            ("sun, short", dict(kind="directional", vec=sun), 0.5, 6.0, (480, 2208, 480)),
            ("high sun", dict(kind="directional", vec=[-0.35, -0.2, 0.8]), 1.0, 12.0, (528, 2208, 528)),
            ("from the open side", dict(kind="directional", vec=[0.5, 0.1, 0.6]), 1.0, 12.0, (0, 3072, 0)),
            ("sun, K 16", dict(kind="directional", vec=sun, spread=0.15, samples=16), 1.0, 12.0, (16752, 35328, None)),
            ("sun, K 64", dict(kind="directional", vec=sun, spread=0.3, samples=64), 1.0, 12.0, (65808, 141312, None)),
            ("lamp in front", dict(kind="point", vec=front), 1.0, 0.0, (0, 3072, 0)),
            ("lamp in front, K 16", dict(kind="point", vec=front, spread=1.5 * VS32, samples=16), 1.0, 0.0, (0, 49152, 0)),
            ("lamp behind the wall", dict(kind="point", vec=behind, spread=1.0 * VS32, samples=8), 1.0, 0.0, (17664, 17664, 2208))]


def corner_analytic(o, w, limit, origin=(0.0, 0.0, 0.0)):
    """a ray o + t w in the corner's free space is occluded iff it runs towards the wall x = X0 vs or the floor z = Z0 vs and reaches the nearer of
    the two planes within its limit.  o [..., 3], w, limit [..., K(, 3)].  Returns (bits, t, near: within NEAR voxels of the limit)."""
    ox = o[..., None, 0] - (origin[0] + X0 * VS32); oz = o[..., None, 2] - (origin[2] + Z0 * VS32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(np.where(w[..., 0] < 0, ox / -w[..., 0], np.inf), np.where(w[..., 2] < 0, oz / -w[..., 2], np.inf))
    with np.errstate(invalid="ignore"):
        return t <= limit, t, np.abs(t - limit) <= NEAR * VS32


@functools.lru_cache(maxsize=None)
def corner_geometry():
    v, dim = corner_volume()
    return lref.geometry(v, dim, VS, np.zeros(3), corner_pose(), INTR, W, H)


def test_corner_view_sees_floor_and_wall():
    geo = corner_geometry()
    hit = geo["voxel"] >= 0
    assert hit.all() and int((geo["normal"][2] == 1).sum()) == 2208 and int((geo["normal"][0] == 1).sum()) == 864


@pytest.mark.parametrize("case", range(9))
def test_corner_yardstick_equals_the_closed_form(case):
    name, light, bias, reach, (n_occ, n_rays, n_shadowed) = corner_cases()[case]
    v, dim = corner_volume()
    geo = corner_geometry()
    floor = geo["normal"][2] == 1
    r = lref.relight(v, dim, VS, np.zeros(3), corner_pose(), INTR, geo, [light], bias * VS32, reach * VS32)[0]
    K = r["K"]
    bits, t, near = corner_analytic(r["o"], r["w"], r["limit"])
    lit = r["lit"]
    differ = (r["bits"] != bits)[lit] & ~near[lit]
    print(f"{name}: {r['n_lit']} lit pixels ({int((lit & floor).sum())} floor), {r['n_occluded']} of {r['n_rays']} rays occluded, {r['n_buried']} buried, "
          f"{int((r['count'] > 0).sum())} pixels shadowed, {int(differ.sum())} rays differ from the closed form, {int(near[lit].sum())} within {NEAR} vs of the limit")
    assert near[lit].sum() <= NEAR_SHARE * max(r["n_rays"], 1)
    assert not differ.any()
    assert (r["n_occluded"], r["n_rays"], r["n_buried"]) == (n_occ, n_rays, 0) and r["n_hits"] == 3072 and r["n_rays"] == K * r["n_lit"]
    if n_shadowed is not None:
        assert int((r["count"] > 0).sum()) == n_shadowed
    if light["vec"][0] < 0 or name == "lamp behind the wall":
        assert np.array_equal(lit, floor)                      # the wall faces away: cos <= 0, unlit, visibility 0 and no rays
        assert not r["visibility"][~floor].any() and not r["rendered"][:, ~floor].any()
    assert np.array_equal(r["visibility"][lit], ((K - r["count"][lit]).astype(f32) / f32(K)))
    # lit and unshadowed: rho (ambient + colour cosv fall) with the closed form's cosine (floor normal (0, 0, 1), wall normal (1, 0, 0))
    free = lit & (r["count"] == 0)
    if free.any():
        vec = np.asarray(light["vec"], f32).astype(np.float64)
        q = r["o"] - bias * VS32 * np.moveaxis(geo["normal"], 0, -1)
        d = np.broadcast_to(vec / np.linalg.norm(vec), q.shape) if light["kind"] == "directional" else (vec - q) / np.linalg.norm(vec - q, axis=-1)[..., None]
        fall = 1.0 if light["kind"] == "directional" else 1.0 / ((vec - q) ** 2).sum(-1)
        exp = 0.5 * np.where(floor, d[..., 2], d[..., 0]) * fall
        assert np.abs(r["rendered"][0][free] / exp[free] - 1).max() < 1e-6
    if light["kind"] == "point" and name.startswith("lamp in front"):
        # the truncation at the light is what is tested: without the |d_i| limit the closed form would shadow some of these pixels
        untruncated, _, _ = corner_analytic(r["o"], r["w"], np.full(r["limit"].shape, np.inf))
        assert untruncated[lit].any() and not bits[lit].any()


def test_yardstick_refuses_bad_parameters_and_sh_needs_no_rays():
    v, dim = corner_volume()
    geo = corner_geometry()
    sh = dict(kind="sh", sh=[0.5, 0.1, -0.2, 0.7], colour=[1, 0.5, 0.25], ambient=[0.1, 0, 0])
    r = lref.relight(v, dim, VS, np.zeros(3), corner_pose(), INTR, geo, [sh], VS32, 0.0)[0]
    assert (r["n_hits"], r["n_lit"], r["n_rays"], r["n_occluded"], r["n_buried"]) == (3072, 3072, 0, 0, 0) and (r["visibility"] == 1).all()
    floor = geo["normal"][2] == 1
    assert np.allclose(r["rendered"][0][floor], 0.5 * (0.1 + 1.2), rtol=1e-6) and np.allclose(r["rendered"][2][~floor], 0.5 * 0.25 * 0.6, rtol=1e-6)
    for bad in (dict(kind="directional", vec=[0, 0, 0]), dict(kind="directional", vec=[0, 0, 1], samples=4), dict(kind="directional", vec=[0, 0, 1], spread=0.1),
                dict(kind="point", vec=[0, np.nan, 1]), dict(kind="point", vec=[0, 0, 1], colour=[-1, 0, 0]), dict(kind="sh", sh=[1, 0, 0]), dict(kind="sh", sh=[1, 0, 0, 0], samples=8),
                dict(kind="spot", vec=[0, 0, 1])):
        with pytest.raises(ValueError):
            lref.relight(v, dim, VS, np.zeros(3), corner_pose(), INTR, geo, [bad], VS32, 0.0)
    for bias, reach in ((0.0, 0.0), (VS32, -1.0), (np.nan, 0.0), (VS32, np.inf)):
        with pytest.raises(ValueError):
            lref.relight(v, dim, VS, np.zeros(3), corner_pose(), INTR, geo, [sh], bias, reach)


def test_library_exports_the_call(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_relight.h") == ["psgsdf_relight"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        assert hasattr(ctypes.CDLL(path), "psgsdf_relight"), path
    assert hasattr(capi.Api, "relight")
    assert (ctypes.sizeof(capi.Light), ctypes.sizeof(capi.RelightParams), ctypes.sizeof(capi.RelightCounts)) == (88, 24, 40)
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    Pt = ctypes.c_void_p
    fn = lib.psgsdf_relight; fn.argtypes = [Pt] * 7
    view, light, par = capi.View(), capi.make_light(dict(kind="directional", vec=[0, 0, 1])), capi.RelightParams(0.01, 0.0, 1, 0)
    out = (ctypes.c_float * 4)()
    ARG = -1
    assert fn(None, ctypes.byref(view), ctypes.byref(light), ctypes.byref(par), out, None, None) == ARG      # a NULL context
    # (the other NULL pointers are refused before the context is looked at: a non-NULL context is not needed to see it)
    for k in range(1, 4):
        args = [None, ctypes.byref(view), ctypes.byref(light), ctypes.byref(par), out, None, None]
        args[k] = None
        assert fn(*args) == ARG
    assert not any(out)


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_relight.c"
    src.write_text('#include "psgsdf_relight.h"\n'
                   'typedef char light_size[sizeof(psgsdf_light) == 88 ? 1 : -1];\ntypedef char params_size[sizeof(psgsdf_relight_params) == 24 ? 1 : -1];\n'
                   'typedef char counts_size[sizeof(psgsdf_relight_counts) == 40 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, const psgsdf_view* v, float* out) {\n    psgsdf_light l = {0}; psgsdf_relight_params p; psgsdf_relight_counts k; int rc;\n'
                   '    l.kind = PSGSDF_LIGHT_DIRECTIONAL; l.vec[2] = 1.0f; l.colour[0] = l.colour[1] = l.colour[2] = 1.0f; l.n_shadow = 16; l.spread = 0.05f;\n'
                   '    p.bias = 0.01; p.reach = 0.0; p.n_lights = 1; p.reserved = 0;\n    rc = psgsdf_relight(c, v, &l, &p, out, 0, &k);\n'
                   '    return rc ? rc : (int)(k.n_occluded + k.n_rays + PSGSDF_LIGHT_SH + PSGSDF_LIGHT_POINT + PSGSDF_RELIGHT_MAX_LIGHTS);\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_relight.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_relight_on_several_gpus_and_bad_files(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    good = tmp_path / "lights.json"
    good.write_text('{"bias_voxels": 1, "reach_voxels": 0, "lights": [{"kind": "directional", "vec": [0, 0, 1], "colour": [1, 1, 1], "ambient": [0, 0, 0], "spread": 0.05, "samples": 16}]}')
    malformed = tmp_path / "malformed.json"
    malformed.write_text('{"lights": [{"kind": "directional", "vec": [0, 0')
    nolights = tmp_path / "nolights.json"
    nolights.write_text('{"bias_voxels": 1}')
    unknown = tmp_path / "unknown.json"
    unknown.write_text('{"lights": [{"kind": "spot", "vec": [0, 0, 1]}]}')
    many = tmp_path / "many.json"
    many.write_text('{"lights": [' + ", ".join(['{"kind": "directional", "vec": [0, 0, 1]}'] * 65) + ']}')
    for extra, words in ((["--relight", str(good), "--gpus", "2"], ("--relight", "--gpus")), (["--relight", str(tmp_path / "missing.json")], ("--relight", "missing.json")),
                         (["--relight", str(malformed)], ("--relight",)), (["--relight", str(nolights)], ("--relight", "lights")),
                         (["--relight", str(unknown)], ("--relight", "kind")), (["--relight", str(many)], ("--relight", "64"))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_relight_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("relight.hip", tmp_path).items() if "k_relight" in k}
    assert len(ks) == 3 and all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in ks.values()), ks      # SH, directional, point: 8 waves per SIMD
    src = open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "relight.hip")).read()
    assert src.count("__shared__") == 0 and "atomicAdd(float" not in src
