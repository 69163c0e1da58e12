"""Baked detail maps without a GPU (include/psgsdf_bake.h psgsdf_bake_lod, DESIGN.md "Baked detail maps"): the yardstick tests/_bake_ref.py on an atlas
whose layout is spelled out here by hand (so that a wrong yardstick cannot hide), on the analytic plane and on the five-piece volume of
test_mesh_components_cpu; the header as C99, the exported symbol, the OBJ writer's self-test, the refusals of `voxelPS --mesh-bake` and the new
kernel's resources."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _bake_ref as bref
import _render_ref as rref
from test_mesh_components_cpu import EXE, HIPCC, ROOT, pieces_volume

f32 = np.float32
VS = 0.01
VS32 = float(f32(VS))


def test_layout_spelled_out_for_three_faces_at_res_two():
    L = bref.layout(3, 2)
    assert (L["B"], L["nblk"], L["bpr"], L["W"], L["H"]) == (3, 2, 2, 6, 3)
    # block 0 (columns 0-2): face 0 above the anti-diagonal and on it, face 1 below; block 1 (columns 3-5): face 2, and the missing face 3 is padding
    assert L["face"].tolist() == [[0, 0, 0, 2, 2, 2],
                                  [0, 0, 1, 2, 2, -1],
                                  [0, 1, 1, 2, -1, -1]]
    assert [int((L["face"] == f).sum()) for f in (0, 1, 2, -1)] == [6, 3, 6, 3]
    # (a, b) of every owned texel: the even face counts from its corner (0, 0), the odd one from the opposite corner (R, R)
    ab = {(int(L["face"][y, x]), x, y): (int(L["a"][y, x]), int(L["b"][y, x])) for y in range(3) for x in range(6) if L["face"][y, x] >= 0}
    assert ab == {(0, 0, 0): (0, 0), (0, 1, 0): (1, 0), (0, 2, 0): (2, 0), (0, 0, 1): (0, 1), (0, 1, 1): (1, 1), (0, 0, 2): (0, 2),
                  (1, 2, 1): (0, 1), (1, 1, 2): (1, 0), (1, 2, 2): (0, 0),
                  (2, 3, 0): (0, 0), (2, 4, 0): (1, 0), (2, 5, 0): (2, 0), (2, 3, 1): (0, 1), (2, 4, 1): (1, 1), (2, 3, 2): (0, 2)}
    # the weights: ninths, strictly inside, summing to one
    for (a, b), exp in {(0, 0): (7 / 9, 1 / 9, 1 / 9), (1, 0): (4 / 9, 4 / 9, 1 / 9), (2, 0): (1 / 9, 7 / 9, 1 / 9), (0, 1): (4 / 9, 1 / 9, 4 / 9),
                        (1, 1): (1 / 9, 4 / 9, 4 / 9), (0, 2): (1 / 9, 1 / 9, 7 / 9)}.items():
        w = bref.weights(np.float64(a), np.float64(b), 2)
        assert np.allclose(w, exp, rtol=0, atol=1e-15) and min(w) > 0 and abs(sum(w) - 1) < 1e-15
    # the corners, in texels (u W, v H): the even face from its texel centres' continuation, the odd one rotated by half a turn
    uv = bref.uv(3, 2)
    assert uv.dtype == f32 and uv.shape == (3, 3, 2)
    tex = uv.astype(np.float64) * np.array([6.0, 3.0])
    exp = np.array([[[1 / 6, 1 / 6], [3 + 1 / 6, 1 / 6], [1 / 6, 3 + 1 / 6]],
                    [[2 + 5 / 6, 2 + 5 / 6], [-1 / 6, 2 + 5 / 6], [2 + 5 / 6, -1 / 6]],
                    [[3 + 1 / 6, 1 / 6], [6 + 1 / 6, 1 / 6], [3 + 1 / 6, 3 + 1 / 6]]])
    assert np.abs(tex - exp).max() < 1e-6
    # ... which is the affine map that sends (a, b) to the texel centre: w1 = (3a + 1) / 9 of the way from corner 0 to corner 1, and so on
    for (f, x, y), (a, b) in ab.items():
        w0, w1, w2 = bref.weights(np.float64(a), np.float64(b), 2)
        assert np.abs(w0 * exp[f, 0] + w1 * exp[f, 1] + w2 * exp[f, 2] - (x + 0.5, y + 0.5)).max() < 1e-12, (f, x, y)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            bref.layout(3, bad)
    with pytest.raises(ValueError):
        bref.layout(7204, 2000)      # 61 blocks a row of 2001 texels
    E = bref.layout(0, 4)
    assert (E["W"], E["H"]) == (0, 0) and bref.uv(0, 4).shape == (0, 3, 2)


@functools.lru_cache(maxsize=None)
def plane():
    dim, _, dist, grad, weight, _ = rref.plane_volume()
    v = dict(dist=dist, grad=grad, weight=weight, rgb=np.full((3, len(dist)), 0.5, f32))
    return v, tuple(int(x) for x in dim)


@functools.lru_cache(maxsize=None)
def pieces():
    v, dim, vs = pieces_volume()
    assert vs == VS
    return v, dim


@functools.lru_cache(maxsize=None)
def pieces_mesh(s):
    v, dim = pieces()
    return bref.lod_mesh(v, dim, VS, s * VS32)


@pytest.mark.parametrize("s,faces", [(2, 1462), (4, 383)])
def test_plane_every_texel_hits_at_zero_displacement(s, faces):
    v, dim = plane()
    m = bref.lod_mesh(v, dim, VS, s * VS32)
    assert len(m["faces"]) == faces      # (383 is odd: the last block's second face is padding)
    b = bref.bake(v, dim, VS, m, 8, s * VS32)
    own = b["face"] >= 0
    err = float(np.abs(b["displacement"]).max()) / VS32
    print(f"plane, cell {s} vs: {b['width']} x {b['height']}, {b['n_texels']} texels, max |displacement| {err:.2e} vs")
    assert b["n_texels"] == int(own.sum()) == 45 * ((faces + 1) // 2) + 36 * (faces // 2)      # of a block of 9 x 9: 45 texels the even face, 36 the odd one
    assert b["n_hits"] == b["n_texels"] and b["n_buried"] == 0 and b["n_misses"] == 0
    assert (b["voxel"][own] >= 0).all() and (b["voxel"][~own] == -1).all()
    # the clusters' positions are means of points on the plane, rounded to float32 at |x| ~ 0.25: 3e-8 of 0.01, and a margin
    assert err <= 1e-4
    assert (b["albedo"][own] == 128).all() and (b["albedo"][~own] == 0).all() and (b["normal"][~own] == 0).all() and (b["displacement"][~own] == 0).all()
    n = np.asarray(v["grad"])[:, 0].astype(np.float64)
    assert np.abs(b["normal"][own].astype(np.float64) - n / np.linalg.norm(n)).max() < 1e-6


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_five_pieces_every_texel_hits_within_reach(s, R):
    v, dim = pieces()
    m = pieces_mesh(s)
    reach = s * VS32
    b = bref.bake(v, dim, VS, m, R, reach)
    F = len(m["faces"])
    assert F == {2: 1560, 4: 424}[s]
    own = b["face"] >= 0
    # an even face owns (R + 1)(R + 2) / 2 texels, an odd one R (R + 1) / 2
    assert b["n_texels"] == int(own.sum()) == (F + 1) // 2 * (R + 1) * (R + 2) // 2 + F // 2 * R * (R + 1) // 2
    assert b["n_hits"] == b["n_texels"] and b["n_buried"] == 0 and b["n_misses"] == 0
    d = b["displacement"][own]
    print(f"five pieces, cell {s} vs, R {R}: {b['n_texels']} texels, displacement {float(d.min()) / VS32:.3f} .. {float(d.max()) / VS32:.3f} vs")
    assert d.min() >= -reach and d.max() <= reach
    assert np.abs(np.linalg.norm(b["normal"][own].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(np.bincount(b["face"][own], minlength=F)[0::2], np.full((F + 1) // 2, (R + 1) * (R + 2) // 2))


def test_five_pieces_short_reach_buries_and_misses():
    v, dim = pieces()
    m = pieces_mesh(4)
    R, reach = 3, 0.25 * VS32
    b = bref.bake(v, dim, VS, m, R, reach)
    assert (b["n_texels"], b["n_buried"], b["n_misses"], b["n_hits"]) == (3392, 2099, 24, 1269)
    own = b["face"] >= 0
    lost = own & (b["voxel"] < 0)
    assert int(lost.sum()) == 2099 + 24 and (b["displacement"][lost] == 0).all()
    # the fallback values: the coarse mesh's own interpolated normal and colour
    f, a, bb = b["face"][lost], bref.layout(len(m["faces"]), R)["a"][lost], bref.layout(len(m["faces"]), R)["b"][lost]
    w0, w1, w2 = bref.weights(a.astype(np.float64), bb.astype(np.float64), R)
    fv = m["faces"].astype(np.int64)[f]
    n = w0[:, None] * m["normals"][fv[:, 0]].astype(np.float64) + w1[:, None] * m["normals"][fv[:, 1]] + w2[:, None] * m["normals"][fv[:, 2]]
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert np.abs(b["normal"][lost] - n).max() < 1e-6
    c = w0[:, None] * m["rgb"][fv[:, 0]].astype(np.float64) + w1[:, None] * m["rgb"][fv[:, 1]] + w2[:, None] * m["rgb"][fv[:, 2]]
    assert np.abs(b["albedo"][lost].astype(np.float64) - c).max() <= 0.5 + 1e-9
    hit = own & ~lost
    assert (np.abs(b["displacement"][hit]) <= reach).all() and (b["t"][hit] > 0).all()


def test_library_exports_the_call(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_bake.h") == ["psgsdf_bake_lod"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        assert hasattr(ctypes.CDLL(path), "psgsdf_bake_lod"), path
    assert hasattr(capi.Api, "bake_lod")
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    out = capi.Bake()
    lib.psgsdf_bake_lod.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]
    assert lib.psgsdf_bake_lod(None, None, 1.0, 4, 1.0, None) == -1                      # PSGSDF_ERR_ARG
    assert lib.psgsdf_bake_lod(None, None, 1.0, 0, 1.0, ctypes.byref(out)) == -1
    assert lib.psgsdf_bake_lod(None, None, 1.0, 4, float("nan"), ctypes.byref(out)) == -1
    assert lib.psgsdf_bake_lod(None, None, 1.0, 4, 1.0, ctypes.byref(out)) == -4         # PSGSDF_ERR_STATE: no context, nothing touched
    assert ctypes.sizeof(capi.Bake) == 168      # sizeof(psgsdf_bake)


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_bake.c"
    src.write_text('#include "psgsdf_bake.h"\nint use(psgsdf_ctx* c) { psgsdf_bake b; int rc = psgsdf_bake_lod(c, 0, 0.02, 8, 0.02, &b); return rc ? rc : (int)(b.n_hits + b.width); }\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_bake.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def read_obj(path):
    """v [V, 3], vn [V, 3], vt [T, 2], f [F, 3, 3] (1-based position / texture / normal numbers), the mtllib and usemtl names"""
    v, vn, vt, f, lib, mtl = [], [], [], [], None, None
    for ln in open(path).read().splitlines():
        w = ln.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "vt":
            vt.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([[int(x) for x in c.split("/")] for c in w[1:]])
        elif w[0] == "mtllib":
            lib = w[1]
        elif w[0] == "usemtl":
            mtl = w[1]
        else:
            raise AssertionError(ln)
    return np.array(v, f32).reshape(-1, 3), np.array(vn, f32).reshape(-1, 3), np.array(vt, f32).reshape(-1, 2), np.array(f, np.int64).reshape(-1, 3, 3), lib, mtl


def read_mtl(path):
    return dict(ln.split(None, 1) for ln in open(path).read().splitlines() if ln.strip())


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_selftest_obj_bake_parses_back(tmp_path):
    from PIL import Image
    out = str(tmp_path / "octa.obj")
    r = subprocess.run([EXE, "--selftest-obj-bake", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    v, vn, vt, f, lib, mtl = read_obj(out)
    assert np.array_equal(v, f32([[1.5, 0, 0], [-1.5, 0, 0], [0, 2.25, 0], [0, -2.25, 0], [0, 0, 0.75], [0, 0, -0.75]]))
    assert np.array_equal(vn, f32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]))
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    assert np.array_equal(f[:, :, 0], faces + 1) and np.array_equal(f[:, :, 2], faces + 1)
    assert np.array_equal(f[:, :, 1], np.arange(24).reshape(8, 3) + 1)                 # one texture coordinate per corner
    fk = np.arange(8)[:, None], np.arange(3)[None, :]
    assert np.array_equal(vt.reshape(8, 3, 2)[:, :, 0], ((3 * fk[0] + fk[1]) / 32.0).astype(f32))
    assert np.array_equal(vt.reshape(8, 3, 2)[:, :, 1], (1.0 - (fk[0] + fk[1]) / 16.0).astype(f32))      # v flipped: OBJ's v points up
    m = read_mtl(str(tmp_path / "octa.mtl"))
    assert lib == "octa.mtl" and mtl == "baked" and m["newmtl"] == "baked" and m["map_Kd"] == "octa_albedo.png" and m["norm"] == "octa_normal.png"
    px = np.asarray(Image.open(str(tmp_path / "octa_normal.png")).convert("RGB"))
    assert px.shape == (1, 3, 3) and px[0].tolist() == [[255, 128, 0], [128, 128, 128], [191, 64, 159]]      # floor(127.5 (n + 1) + 0.5)


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_bake_without_lod_on_several_gpus_and_a_bad_res(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    for extra, words in ((["--mesh-bake", "4"], ("--mesh-bake", "--mesh-lod")), (["--mesh-lod", "2", "--mesh-bake", "4", "--gpus", "2"], ("--mesh-bake", "--gpus")),
                         (["--mesh-lod", "2", "--mesh-bake", "0"], ("--mesh-bake",)), (["--mesh-lod", "2", "--mesh-bake", "1.5"], ("--mesh-bake",)),
                         (["--mesh-lod", "2", "--mesh-bake", "x"], ("--mesh-bake",))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_bake_kernel_uses_no_scratch_and_the_renderer_keeps_its_registers(tmp_path):
    from test_kernel_resources import resources
    res = resources("bake.hip", tmp_path)
    ks = {k: v for k, v in res.items() if "k_bake" in k}
    assert len(ks) == 1 and all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in ks.values()), ks      # 8 waves per SIMD
    # the walk moved into render_trace.h: the renderer's kernels are the ones they were (44 registers for the SH models, 46 / 47 for LED)
    ren = {k: v["vgpr"] for k, v in resources("render.hip", tmp_path).items() if "k_renderIL" in k or "k_render_reportIL" in k}
    assert len(ren) == 12 and all(v == (44 if "ILi2E" not in k.split("k_render")[1][:12] else (46 if "ELi1EEE" in k else 47)) for k, v in ren.items()), ren
