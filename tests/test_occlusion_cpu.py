"""Ambient occlusion without a GPU (include/psgsdf_occlusion.h, DESIGN.md "Ambient occlusion"): the yardstick tests/_occlusion_ref.py against closed-form
geometry -- a floor meeting a wall, where a ray is occluded iff it reaches the wall's plane within the radius, and the analytic plane, where none
is -- the direction table, the frame, the byte rule in exact fractions; the header as C99, the exported symbols and struct sizes, the calls' returns
without a context, the refusals of `voxelPS --mesh-bake-ao` and the new kernel's resources."""
import ctypes
import functools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _occlusion_ref as oref
import _render_ref as rref
from test_mesh_components_cpu import EXE, HIPCC, ROOT

f32 = np.float32
VS = 0.01
VS32 = float(f32(VS))
X0, Z0 = 20.3, 17.6                                   # the wall's and the floor's plane, in voxels
CASES = [(1.0, 8.0), (0.5, 4.0), (1.0, 16.0)]         # (bias, radius) in voxels
# occluded rays of the 141 samples for K = 8, 16, 32, 64: counts from a float64 run of the definition
PROTOTYPE = {(1.0, 8.0): (150, 291, 591, 1146), (0.5, 4.0): (66, 129, 261, 507), (1.0, 16.0): (315, 615, 1188, 2355)}
NEAR = 1e-3                                           # rays whose analytic parameter is this close (in voxels) to the radius are not compared


@functools.lru_cache(maxsize=None)
def corner_volume(N=48):
    """a floor z = Z0 vs meeting a wall x = X0 vs (free space: x > X0 vs and z > Z0 vs), positions X = vs x index: dist = min(dx, dz), the gradient
    of whichever is smaller, weight 1 within 3 voxels of the surface.  Returns (v, dim)."""
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    dx = (VS * i.ravel() - X0 * VS); dz = (VS * k.ravel() - Z0 * VS)
    wall = dx < dz
    dist = np.minimum(dx, dz)
    grad = np.zeros((3, N ** 3), f32)
    grad[0, wall] = 1; grad[2, ~wall] = 1
    v = dict(dist=dist.astype(f32), grad=grad, weight=(np.abs(dist) < 3 * VS).astype(f32), rgb=np.full((3, N ** 3), 0.5, f32))
    return v, (N, N, N)


def corner_samples():
    """141 points on the floor, 0.5 .. 12 voxels from the wall in three rows: q [141, 3] float32, m = (0, 0, 1)"""
    a = np.linspace(0.5, 12, 47)
    q = np.array([[X0 * VS + ai * VS, y * VS, Z0 * VS] for y in (15.2, 24.0, 30.7) for ai in a]).astype(f32)
    return q, np.tile(f32([0, 0, 1]), (len(q), 1))


def corner_analytic(q, K, bias, radius, D=None):
    """ray i of sample j is occluded iff it runs towards the wall and reaches its plane within the radius: bits [n, K], the parameter t [n, K] (inf:
    never), and which rays are nearer than NEAR voxels to the radius.  m = (0, 0, 1): t1 = (1, 0, 0), t2 = (0, 1, 0), so w = D_i; o = q + bias m.
    D: the table to use instead of the yardstick's (the device's own)."""
    D = oref.dirs(K) if D is None else np.asarray(D, np.float64)
    t1, t2 = oref.frame(np.array([[0.0, 0.0, 1.0]]))
    assert np.array_equal(t1, [[1, 0, -0.0]]) and np.array_equal(t2, [[0, 1, -0.0]])
    ox = q[:, 0].astype(np.float64)[:, None] - X0 * VS32
    wx = D[None, :, 0]
    with np.errstate(divide="ignore"):
        t = np.where(wx < 0, ox / -wx, np.inf)
    return t <= radius, t, np.abs(t - radius) <= NEAR * VS32


def test_direction_table():
    for K in oref.KS:
        D = oref.dirs(K)
        assert D.shape == (K, 3) and D.dtype == np.float64
        assert np.abs(np.linalg.norm(D, axis=1) - 1).max() < 1e-15 and (D[:, 2] > 0).all()
        assert np.array_equal(D[:, 2], np.sqrt(1 - (np.arange(K) + 0.5) / K))
    assert abs(oref.dirs(64)[:, 2].mean() - 2 / 3) < 0.02      # cosine-weighted: E[z] = 2 / 3
    # the first rows by hand: phi_0 = 0, phi_1 = 2 pi g
    D = oref.dirs(8)
    assert np.allclose(D[0], [0.25, 0, np.sqrt(15 / 16)], rtol=0, atol=1e-16)
    assert np.allclose(D[1], [np.sqrt(3 / 16) * np.cos(2 * np.pi * oref.GOLDEN), np.sqrt(3 / 16) * np.sin(2 * np.pi * oref.GOLDEN), np.sqrt(13 / 16)], rtol=0, atol=1e-15)


def test_frame_is_orthonormal():
    rng = np.random.default_rng(5)
    r = rng.normal(size=(2000, 3)); r /= np.linalg.norm(r, axis=1)[:, None]
    m = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0], [1, 0, 0.0], [1, 0, -0.0], [0, -1, 0.0], [0.6, 0, -0.8]], r])
    t1, t2 = oref.frame(m)
    for a, b, e in ((t1, t1, 1), (t2, t2, 1), (t1, t2, 0), (t1, m, 0), (t2, m, 0)):
        assert np.abs((a * b).sum(1) - e).max() < 1e-15
    assert np.abs(np.cross(t1, t2) - m).max() < 1e-15      # right-handed: t1 x t2 = m
    # copysign, not sign: a normal in the plane z = -0.0 takes the lower branch and its denominator is -1, never 0
    p, n = oref.frame([[1, 0, 0.0]]), oref.frame([[1, 0, -0.0]])
    assert np.array_equal(p[0], [[0, 0, -1]]) and np.array_equal(n[0], [[0, -0.0, 1]]) and np.isfinite(p + n).all()


def test_byte_rule_in_exact_fractions():
    for K in oref.KS:
        for c in range(K + 1):
            exact = Fraction(255 * (K - c), K) + Fraction(1, 2)
            assert oref.byte(K, c) == exact.numerator // exact.denominator, (K, c)
        assert oref.byte(K, 0) == 255 and oref.byte(K, K) == 0
    for bad in ((12, 1.0, 1.0), (16, 0.0, 1.0), (16, 1.0, float("nan")), (16, float("inf"), 1.0), (128, 1.0, 1.0)):
        with pytest.raises(ValueError):
            oref.check_params(*bad)


@pytest.mark.parametrize("K", oref.KS)
@pytest.mark.parametrize("bias,radius", CASES)
def test_corner_yardstick_equals_the_analytic_bits(K, bias, radius):
    v, dim = corner_volume()
    q, m = corner_samples()
    assert len(q) == 141
    r = oref.occlusion(v, dim, VS, q, m, K, radius * VS32, bias * VS32)
    bits, t, near = corner_analytic(q, K, bias * VS32, radius * VS32)
    differ = r["bits"] != bits
    t_err = float(np.abs(r["t"][bits & r["bits"]] - t[bits & r["bits"]]).max()) / VS32
    print(f"corner K {K} bias {bias} radius {radius}: {int(bits.sum())} of {bits.size} rays occluded (prototype {PROTOTYPE[(bias, radius)][oref.KS.index(K)]}), "
          f"{int(differ.sum())} differ, {int(near.sum())} within {NEAR} vs of the radius, hit parameter within {t_err:.2e} vs")
    assert not near.any()                                   # a condition of the comparison: no ray sits on the radius
    assert not differ.any()
    assert t_err < 1e-4                                     # the model is exact on both planes: float32 rounding of uo, uw at |u| <= 48
    assert int(bits.sum()) == PROTOTYPE[(bias, radius)][oref.KS.index(K)]
    assert r["n_valid"] == 141 and r["n_rays"] == 141 * K and r["n_occluded"] == int(bits.sum()) and r["n_buried"] == 0
    c = bits.sum(1)
    assert np.array_equal(r["occlusion"], [oref.byte(K, x) for x in c])
    assert np.array_equal(r["mask"], [sum(1 << i for i in range(K) if b[i]) for b in bits])
    # nearer the wall, never fewer occluded rays (the same directions at every sample)
    assert (np.diff(c.reshape(3, 47), axis=1) <= 0).all() and c.reshape(3, 47)[:, 0].min() > 0


@functools.lru_cache(maxsize=None)
def plane():
    dim, _, dist, grad, weight, n = rref.plane_volume()
    v = dict(dist=dist, grad=grad, weight=weight, rgb=np.full((3, len(dist)), 0.5, f32))
    return v, tuple(int(x) for x in dim), n


def plane_samples(n_pts=300):
    """points on the plane n.x = offset inside the grid's middle, in the mesh's units (the volume's origin is -0.5 vs dim: mesh = world - origin)"""
    _, dim, n = plane()
    rng = np.random.default_rng(11)
    e1 = np.cross(n, [0, 0, 1.0]); e1 /= np.linalg.norm(e1); e2 = np.cross(n, e1)
    ab = rng.uniform(-8 * VS, 8 * VS, size=(n_pts, 2))
    world = 0.004 * n + ab[:, :1] * e1 + ab[:, 1:] * e2
    return (world + 0.5 * VS * np.asarray(dim)).astype(f32), np.tile(n.astype(f32), (n_pts, 1))


@pytest.mark.parametrize("K", [8, 64])
def test_plane_is_open(K):
    v, dim, _ = plane()
    q, m = plane_samples()
    r = oref.occlusion(v, dim, VS, q, m, K, 8 * VS32, 0.25 * VS32)
    assert r["n_valid"] == 300 and r["n_rays"] == 300 * K and r["n_occluded"] == 0 and r["n_buried"] == 0
    assert (r["occlusion"] == 255).all() and not r["mask"].any()
    # ... and the same rays turned into the plane all end in it: the samples are where the surface is
    r = oref.occlusion(v, dim, VS, q, -m, K, 8 * VS32, 0.25 * VS32)
    assert r["n_occluded"] == r["n_buried"] == 300 * K and not r["occlusion"].any()


def test_invalid_samples_take_no_part():
    v, dim = corner_volume()
    q, m = corner_samples()
    q, m = q[:4].copy(), m[:4].copy()
    q[1, 0] = np.nan; m[2] = 0; m[3, 1] = np.inf
    r = oref.occlusion(v, dim, VS, q, m, 16, 8 * VS32, VS32)
    assert r["valid"].tolist() == [True, False, False, False] and r["n_samples"] == 4 and r["n_valid"] == 1 and r["n_rays"] == 16
    assert (r["occlusion"][1:] == 255).all() and not r["mask"][1:].any() and r["n_occluded"] == int(r["bits"][0].sum()) > 0


def test_library_exports_the_calls(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_occlusion.h") == ["psgsdf_bake_lod_ao", "psgsdf_occlusion_points"]
    assert g._declared_symbols("psgsdf_bake.h") == ["psgsdf_bake_lod"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "psgsdf_occlusion_points") and hasattr(lib, "psgsdf_bake_lod_ao"), path
    assert hasattr(capi.Api, "occlusion_points") and hasattr(capi.Api, "bake_lod_ao")
    assert (ctypes.sizeof(capi.AoParams), ctypes.sizeof(capi.AoCounts), ctypes.sizeof(capi.Bake), ctypes.sizeof(capi.BakeAo)) == (24, 40, 168, 240)
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    P = ctypes.c_void_p
    pts = lib.psgsdf_occlusion_points; pts.argtypes = [P, P, P, ctypes.c_int64, P, P, P, P, P]
    ao = lib.psgsdf_bake_lod_ao; ao.argtypes = [P, P, ctypes.c_double, ctypes.c_int32, ctypes.c_double, P, P]
    good = capi.AoParams(16, 0, 0.08, 0.01)
    mask, occ, dirs, cnt, out = P(), P(), P(), capi.AoCounts(), capi.BakeAo()
    x = (ctypes.c_float * 3)(0, 0, 0)
    refs = [ctypes.byref(mask), ctypes.byref(occ), ctypes.byref(dirs), ctypes.byref(cnt)]
    ARG, STATE = -1, -4
    for k in range(4):                                   # a NULL output pointer
        assert pts(None, x, x, 1, ctypes.byref(good), *[None if i == k else r for i, r in enumerate(refs)]) == ARG
    assert pts(None, None, x, 1, ctypes.byref(good), *refs) == ARG and pts(None, x, None, 1, ctypes.byref(good), *refs) == ARG
    assert pts(None, x, x, 1, None, *refs) == ARG and pts(None, x, x, -1, ctypes.byref(good), *refs) == ARG
    assert ao(None, None, 1.0, 4, 1.0, ctypes.byref(good), None) == ARG and ao(None, None, 1.0, 4, 1.0, None, ctypes.byref(out)) == ARG
    assert ao(None, None, 1.0, 0, 1.0, ctypes.byref(good), ctypes.byref(out)) == ARG      # what psgsdf_bake_lod refuses
    for bad in (capi.AoParams(12, 0, 0.08, 0.01), capi.AoParams(0, 0, 0.08, 0.01), capi.AoParams(128, 0, 0.08, 0.01), capi.AoParams(16, 1, 0.08, 0.01),
                capi.AoParams(16, 0, 0.0, 0.01), capi.AoParams(16, 0, 0.08, -1.0), capi.AoParams(16, 0, float("nan"), 0.01), capi.AoParams(16, 0, 0.08, float("inf"))):
        assert pts(None, x, x, 1, ctypes.byref(bad), *refs) == ARG, (bad.n_dirs, bad.reserved, bad.radius, bad.bias)
        assert ao(None, None, 1.0, 4, 1.0, ctypes.byref(bad), ctypes.byref(out)) == ARG
    for K in oref.KS:                                    # everything in order but the context: PSGSDF_ERR_STATE, nothing touched
        ok = capi.AoParams(K, 0, 0.08, 0.01)
        assert pts(None, x, x, 1, ctypes.byref(ok), *refs) == STATE and pts(None, None, None, 0, ctypes.byref(ok), *refs) == STATE
        assert ao(None, None, 1.0, 4, 1.0, ctypes.byref(ok), ctypes.byref(out)) == STATE


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_ao.c"
    src.write_text('#include "psgsdf_occlusion.h"\n'
                   'typedef char params_size[sizeof(psgsdf_ao_params) == 24 ? 1 : -1];\ntypedef char counts_size[sizeof(psgsdf_ao_counts) == 40 ? 1 : -1];\n'
                   'typedef char bake_size[sizeof(psgsdf_bake) == 168 ? 1 : -1];\ntypedef char bake_ao_size[sizeof(psgsdf_bake_ao) == 240 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, const float* x, const float* n) {\n    psgsdf_ao_params p; psgsdf_ao_counts k; psgsdf_bake_ao b; const uint64_t* m; const uint8_t* o; const double* d; int rc;\n'
                   '    p.n_dirs = 16; p.reserved = 0; p.radius = 0.08; p.bias = 0.01;\n    rc = psgsdf_occlusion_points(c, x, n, 1, &p, &m, &o, &d, &k);\n'
                   '    if (!rc) rc = psgsdf_bake_lod_ao(c, 0, 0.02, 8, 0.02, &p, &b);\n    return rc ? rc : (int)(k.n_occluded + b.counts.n_rays + b.bake.width + b.n_dirs);\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_ao.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_ao_without_bake_on_several_gpus_and_a_bad_count(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    for extra, words in ((["--mesh-lod", "2", "--mesh-bake-ao", "16"], ("--mesh-bake-ao", "--mesh-bake")), (["--mesh-bake-ao", "16"], ("--mesh-bake-ao", "--mesh-bake")),
                         (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "16", "--gpus", "2"], ("--mesh-bake-ao", "--gpus")),
                         (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "12"], ("--mesh-bake-ao", "8, 16, 32 or 64")),
                         (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "0"], ("--mesh-bake-ao",)), (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "16.5"], ("--mesh-bake-ao",)),
                         (["--mesh-lod", "2", "--mesh-bake", "4", "--mesh-bake-ao", "x"], ("--mesh-bake-ao",))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_occlusion_kernels_use_no_scratch_and_the_other_walkers_keep_their_registers(tmp_path):
    from test_bake_cpu import test_bake_kernel_uses_no_scratch_and_the_renderer_keeps_its_registers as pins
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("occlusion.hip", tmp_path).items() if "k_occlusion" in k}
    assert len(ks) == 2 and all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in ks.values()), ks      # points and bake provider: 8 waves per SIMD
    assert open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "occlusion.hip")).read().count("__shared__") == 0
    pins(tmp_path)      # render_trace's cut is a template parameter: k_render, k_render_report and k_bake are the kernels they were
