"""The photometric fit per band row and vertex without a GPU (include/psgsdf_fit.h, DESIGN.md "Photometric fit per voxel and vertex"): the numpy
restatement tests/_fit_ref.py on a hand-written band whose answer is spelled out, the library's two symbols, the header as C, and the binary PLY
writer of `voxelPS --mesh-fit`."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fit_ref as fref
from test_mesh_indexed_cpu import read_ply_indexed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
N, VS = 8, 0.1
LIN = lambda i, j, k: (k * N + j) * N + i


def hand_state(loss=0, lam=0.2):
    """An 8^3 grid at 0.1 with the plane z = 0.32: d = 0.1 (k - 3) - 0.02, stored gradient (0, 0, 1).  Band rows (3,3,3), (4,3,3), (3,4,3) and (5,5,3);
    the last one is seen by no frame.  Forward differences find d unchanged along x and y (or no band neighbour: backward, the same), and no band row
    above: backward along z, (d - d_below) / vs = 1: the normal is (0, 0, 1).  Surface points (0.1 i, 0.1 j, 0.32).  One camera at (0.35, 0.35, -1)
    looking along +z, f = 100, centre (8, 8) of a 16 x 16 image: depth 1.32, pixels at columns and rows 4.2 and 11.8, more than 3 pixels inside.
    A constant image 0.5, albedo 1, SH1 light (0.3, 0, 0, 0.6): rendered 0.3 + 0.6 * 1 = 0.9, residual -0.4 in every channel."""
    k = np.arange(N ** 3) // (N * N)
    dist = (VS * (k - 3) - 0.02).astype(np.float32)
    grad = np.zeros((3, N ** 3), np.float32); grad[2] = 1
    band = np.array(sorted([LIN(3, 3, 3), LIN(4, 3, 3), LIN(3, 4, 3), LIN(5, 5, 3)]))
    vis = np.zeros((N ** 3, 1), np.uint64); vis[band[:3]] = 1
    pose = np.eye(4); pose[:3, 3] = [0.35, 0.35, -1.0]
    return dict(band=band, dist=dist, grad=grad, rgb=np.ones((3, N ** 3), np.float32), vis=vis, dim=(N, N, N), vs=VS, origin=np.zeros(3), poses=pose.reshape(1, 16),
                light=np.array([[0.3, 0.0, 0.0, 0.6]]), images=np.full((1, 16, 16, 3), 0.5), K=(100.0, 100.0, 8.0, 8.0), model=0, loss=loss, lam=lam)


def test_hand_written_band():
    got = fref.band_fit(hand_state())
    assert got["margin_px"] > 3 and abs(got["min_depth"] - 1.32) < 1e-6
    assert list(got["n_obs"]) == [1, 1, 1, 0]
    assert np.allclose(got["sum_r2"], [[0.16] * 3] * 3 + [[0.0] * 3], rtol=1e-6, atol=0)
    assert np.allclose(got["loss"], [0.48, 0.48, 0.48, 0.0], rtol=1e-6, atol=0)                       # L2: 3 x 0.4^2
    lam = float(np.float32(0.2))
    for loss, per_channel in ((1, np.log(1 + (0.4 / lam) ** 2)), (2, lam * (0.4 - 0.5 * lam)), (3, 1.0), (4, lam * lam)):      # |r| = 2 lambda: beyond every threshold
        assert np.allclose(fref.band_fit(hand_state(loss))["loss"], [3 * per_channel] * 3 + [0.0], rtol=1e-6, atol=0), loss
    assert list(fref.popcount_below(hand_state()["vis"][hand_state()["band"]], 1)) == [1, 1, 1, 0]
    # the light's direction term: tilt it and the rendered colour follows the normal (0, 0, 1) only
    st = hand_state(); st["light"] = np.array([[0.3, 0.5, -0.5, 0.2]])
    assert np.allclose(fref.band_fit(st)["sum_r2"][:3], 0.0, atol=1e-12)                               # 0.3 + 0.2 = 0.5: the image's colour


def test_vertex_attributes_of_the_hand_written_band():
    st = hand_state()
    rows = fref.band_fit(st)
    keys = np.array([4 * LIN(3, 3, 3) + 0, 4 * LIN(3, 3, 3) + 1, 4 * LIN(3, 3, 3) + 2, 4 * LIN(4, 3, 3) + 0, 4 * LIN(3, 4, 3) + 3, 4 * LIN(5, 5, 3) + 3, 4 * LIN(6, 6, 3) + 3, 4 * LIN(4, 5, 3) + 0])
    n, rms, loss = fref.vertex_fit(rows["n_obs"], rows["loss"], rows["sum_r2"], st["band"], keys, st["dim"])
    # x-edge between two observed rows; y-edge likewise; z-edge up to a voxel outside the band; x-edge out of the band; an observed corner; the unseen
    # row as a corner; a corner outside the band; an edge from outside the band to the unseen row
    assert list(n) == [2, 2, 1, 1, 1, 0, 0, 0]
    assert rms.dtype == np.float32 and loss.dtype == np.float32
    assert np.array_equal(rms, np.float32([np.sqrt(rows["sum_r2"][0].sum() / 3)] * 5 + [0, 0, 0])) and abs(float(rms[0]) - 0.4) < 1e-7
    assert np.array_equal(loss, np.float32([rows["loss"][0]] * 5 + [0, 0, 0])) and abs(float(loss[0]) - 0.48) < 1e-7


def test_library_exports_the_two_calls(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_fit.h") == ["psgsdf_band_fit", "psgsdf_extract_mesh_fit"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "psgsdf_band_fit") and hasattr(lib, "psgsdf_extract_mesh_fit"), path
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.psgsdf_band_fit(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(p), ctypes.byref(n)) == -4      # PSGSDF_ERR_STATE: no context, nothing touched
    assert lib.psgsdf_band_fit(None, None, None, None, None) == -1                                                    # PSGSDF_ERR_ARG


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_fit.c"
    src.write_text('#include "psgsdf_fit.h"\nint use(psgsdf_ctx* c) { const int32_t* n; const double* l; const float* r; int64_t s; return psgsdf_band_fit(c, &n, &l, &r, &s); }\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_fit.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def read_ply_fit(path):
    """(header lines, vertex records, faces) of `voxelPS --mesh-fit`'s file: the welded mesh's records with quality, loss, n_obs behind the colours"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("quality", "<f4"), ("loss", "<f4"), ("n_obs", "<i4")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize and vt.itemsize == 39
    props = [h for h in head if h.startswith("property")]
    assert props[:9] == ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                         "property uchar red", "property uchar green", "property uchar blue"]
    assert props[9:] == ["property float quality", "property float loss", "property int n_obs", "property list uchar int vertex_indices"]
    verts = np.frombuffer(raw, vt, nv, end)
    fc = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (fc["n"] == 3).all()
    return head, verts, fc["v"].copy()


def header_fit_numbers(head):
    """(overall rms, observations) of the header's `comment fit` line"""
    w = next(h for h in head if h.startswith("comment fit rms ")).split()
    assert w[4] == "observations" and len(w) == 6
    return float(w[3]), int(w[5])


def assert_header_matches_columns(head, verts):
    rms, n = header_fit_numbers(head)
    no = verts["n_obs"].astype(np.int64)
    assert n == int(no.sum())
    exp = np.sqrt((no * verts["quality"].astype(np.float64) ** 2).sum() / n) if n else 0.0
    assert abs(rms - exp) <= 1e-12 * max(exp, 1e-300), (rms, exp)


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_selftest_ply_fit_parses_back(tmp_path):
    out, plain = str(tmp_path / "octa_fit.ply"), str(tmp_path / "octa.ply")
    for flag, path in (("--selftest-ply-fit", out), ("--selftest-ply-indexed", plain)):
        r = subprocess.run([EXE, flag, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
    head, verts, faces = read_ply_fit(out)
    phead, pverts, pfaces = read_ply_indexed(plain)
    assert np.array_equal(faces, pfaces)
    for k in pverts.dtype.names:
        assert np.array_equal(verts[k], pverts[k]), k
    assert np.array_equal(verts["quality"], np.float32([0.125, 0.03125, 0.0, 0.25, 0.0625, 0.5]))
    assert np.array_equal(verts["loss"], np.float32([0.75, 0.01, 0.0, 1.5, 0.02, 2.25])) and list(verts["n_obs"]) == [3, 8, 0, 1, 16, 2]
    assert_header_matches_columns(head, verts)
    assert header_fit_numbers(head)[1] == 30
    assert [h for h in head if not h.startswith(("comment fit", "property"))] == [h for h in phead if not h.startswith("property")]
