"""View rendering (include/psgsdf_render.h), what runs without a GPU: the ABI is exported, NULL arguments are refused before any device call,
the render kernels compile for gfx950 without scratch, and the numpy restatement of the traversal (tests/_render_ref.py, the definition the
GPU tests compare the kernel with) hits an analytic plane at its analytic depth."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "psgradientsdf_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def render_symbols():
    hdr = open(os.path.join(ROOT, "include", "psgsdf_render.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(psgsdf_[a-z0-9_]+)\s*\(", hdr)))


def test_both_libraries_export_the_render_abi(built):
    from psgradientsdf_amd import capi
    names = render_symbols()
    assert names == ["psgsdf_render", "psgsdf_render_report", "psgsdf_render_size"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        lib = C.CDLL(path)
        assert all(hasattr(lib, n) for n in names), path


def test_null_context_or_view_is_an_argument_error(built):
    from psgradientsdf_amd import capi
    lib = capi.engine_lib()
    view = capi.View()
    st = capi.RenderStats()
    lib.psgsdf_render.restype = C.c_int
    lib.psgsdf_render_report.restype = C.c_int
    assert lib.psgsdf_render(None, C.byref(view), C.c_uint32(capi.R_DEPTH), None, C.byref(st)) == -1
    assert lib.psgsdf_render(None, None, C.c_uint32(0), None, None) == -1
    assert lib.psgsdf_render_report(None, C.byref(st)) == -1
    w, h = C.c_int32(), C.c_int32()
    lib.psgsdf_render_size.restype = C.c_int
    assert lib.psgsdf_render_size(None, C.byref(view), C.byref(w), C.byref(h)) == -1
    assert C.sizeof(capi.View) == 4 + 64 + 16 + 12 and C.sizeof(capi.RenderStats) == 24 + 56


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_render_kernels_compile_without_scratch(tmp_path):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-c", "render.hip", "-o", str(tmp_path / "r.o"),
                          "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for ln in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1); res[name] = {}
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            res[name]["scratch"] = int(m.group(1))
    kernels = {k: v for k, v in res.items() if "k_render" in k}
    assert sum("k_render_report" in k for k in kernels) == 6 and sum("k_renderIL" in k for k in kernels) == 6      # 3 models x {float, 8-bit keyframes}
    assert any("k_render_bricks" in k for k in kernels) and any("k_render_fold" in k for k in kernels)
    assert all(v["scratch"] == 0 for v in kernels.values()), kernels


def test_restatement_hits_an_analytic_plane():
    vs, N, off = 0.01, 48, 0.004
    dim, origin, dist, grad, weight, n = ref.plane_volume(N=N, vs=vs, offset=off)
    W, H, fx, fy = 96, 72, 80.0, 80.0
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    pose = ref.look_at(0.62 * n + np.array([0.03, -0.02, 0.0]), np.zeros(3))
    depth, vox = ref.trace(dist, grad, weight, dim, vs, origin, pose, fx, fy, cx, cy, W, H)
    z = ref.plane_depth(n, off, pose, fx, fy, cx, cy, W, H)
    hit = depth > 0
    assert hit.mean() > 0.5
    assert np.abs(depth[hit] - z[hit]).max() / z[hit].min() < 1e-5
    # the voxel of every hit is the nearest voxel of the hit point, and it is observed
    P = pose
    ys, xs = np.nonzero(hit)
    p = P[:3, 3] + depth[hit][:, None] * (np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(len(xs))], 1) @ P[:3, :3].T)
    u = (p - origin) / vs + 0.5
    lin = vox[hit]
    cell = np.stack([lin % N, (lin // N) % N, lin // (N * N)], 1)
    assert np.all(u >= cell - 1e-6) and np.all(u <= cell + 1 + 1e-6)
    assert np.all(weight[lin] > 0)
    # a miss everywhere when the camera looks away from the volume
    away = ref.look_at(0.62 * n, 1.5 * n)
    d2, v2 = ref.trace(dist, grad, weight, dim, vs, origin, away, fx, fy, cx, cy, W, H)
    assert not (d2 > 0).any() and (v2 == -1).all()


def test_voxelps_png_writer_round_trips_through_pil(built, tmp_path):
    from PIL import Image
    exe = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
    out = str(tmp_path / "p.png")
    r = subprocess.run([exe, "--selftest-png-write", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    a = np.asarray(Image.open(out))
    y, x = np.mgrid[0:23, 0:37]
    want = np.stack([(7 * x) % 256, (11 * y) % 256, (x * y) % 256], -1).astype(np.uint8)
    assert a.dtype == np.uint8 and np.array_equal(a, want)
