"""Surface curvature without a GPU (include/psgsdf_curvature.h, DESIGN.md "Surface curvature"): the yardstick tests/_curvature_ref.py against closed-form
geometry -- sphere, cylinder, tilted plane, torus -- and against the adjugate formulation of the same invariants; the header as C99, the exported
symbols and struct sizes, the calls' returns without a context, the PLY writer of `voxelPS --mesh-curvature`, the byte rule of
`--mesh-bake-curvature`, the flags' refusals and the kernels' resources.  The analytic volumes and bounds are shared with tests/test_curvature_gpu.py."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _curvature_ref as cref
from test_mesh_components_cpu import EXE, HIPCC, ROOT
from test_mesh_indexed_cpu import read_ply_indexed

f32 = np.float32
N, VS = 32, 0.016
VS32 = float(f32(VS))
CENTRE = np.array([0.47, 0.52, 0.45]) * N * VS
PLANE_N = np.array([0.36, -0.48, 0.8])                 # a unit normal tilted against every axis
SHAPES = ("sphere", "cylinder", "plane", "torus")
# the figures the formulation was checked at (float32 distances, voxels with |d| < vs); every bound below is asserted at 3 x its figure: the margin
# covers other centres and radii, and a different libm
MARGIN = 3.0
FIG = dict(sphere_mean_rel=3.3e-3, sphere_gauss=9e-5, cyl_k1_rel=4.9e-3, cyl_zero=1e-16, cyl_dir=1e-15, plane_mean=1e-7, torus_mean=4.3e-3)


@functools.lru_cache(maxsize=None)
def shape_volume(kind):
    """(v, dim, X, lin): an N^3 volume of the shape's exact distance in float32, weight 1 within 3 voxels of the surface; X [n, 3] the voxel centres
    (vs x index); lin the voxels with |d| < vs off the grid's faces"""
    idx = np.stack(np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)      # x fastest
    X = idx * VS
    p = X - CENTRE
    rho = np.hypot(p[:, 0], p[:, 1])
    if kind == "sphere":
        d = np.linalg.norm(p, axis=1) - 9.6 * VS
    elif kind == "cylinder":
        d = rho - 8 * VS
    elif kind == "plane":
        d = p @ PLANE_N
    elif kind == "torus":
        d = np.hypot(rho - 9 * VS, p[:, 2]) - 4 * VS
    else:
        raise ValueError(kind)
    v = dict(dist=d.astype(f32), weight=(np.abs(d) < 3 * VS).astype(f32))
    for a in v.values():
        a.setflags(write=False)
    inside = ((idx >= 1) & (idx <= N - 2)).all(1)      # (the cylinder and the plane run into the grid's faces, whose voxels are invalid by definition)
    return v, (N, N, N), X, np.nonzero((np.abs(d) < VS) & inside)[0]


def analytic_figures(kind, X, r):
    """the shape's figures of a result r (voxels()'s dict, or the device's) at the voxel centres X, all of them valid; each is dimensionless.  Returns a
    dict name -> (measured, bound): measured <= bound must hold"""
    p = X - CENTRE
    rho = np.hypot(p[:, 0], p[:, 1])
    c = {k: np.asarray(r[k], np.float64) for k in ("mean", "gauss", "k1", "k2", "dir1")}
    assert (np.asarray(r["valid"]) == 1).all() and len(X) > 500, kind
    if kind == "sphere":
        rr = np.linalg.norm(p, axis=1)
        return dict(mean_rel=(np.abs(c["mean"] * rr - 1).max(), MARGIN * FIG["sphere_mean_rel"]), gauss=(np.abs(c["gauss"] - 1 / rr ** 2).max() * VS32 ** 2, MARGIN * FIG["sphere_gauss"]))
    if kind == "cylinder":
        return dict(k1_rel=(np.abs(c["k1"] * rho - 1).max(), MARGIN * FIG["cyl_k1_rel"]), k2=(np.abs(c["k2"]).max() * VS32, MARGIN * FIG["cyl_zero"]),
                    gauss=(np.abs(c["gauss"]).max() * VS32 ** 2, MARGIN * FIG["cyl_zero"]), dir_z=(np.abs(c["dir1"][:, 2]).max(), MARGIN * FIG["cyl_dir"]))
    if kind == "plane":
        return dict(mean=(np.abs(c["mean"]).max() * VS32, MARGIN * FIG["plane_mean"]))
    if kind == "torus":
        rt = np.hypot(rho - 9 * VS, p[:, 2])                       # distance to the centre circle
        exact = 0.5 * (1 / rt + (rho - 9 * VS) / (rt * rho))       # the tube's curvature and the parallel's
        inner, outer = rho < 7 * VS, rho > 11 * VS                 # more than 2 voxels inside / outside the centre circle
        assert inner.sum() > 50 and outer.sum() > 50
        sign_ok = (c["gauss"][inner] < 0).all() and (c["gauss"][outer] > 0).all()
        return dict(mean=(np.abs(c["mean"] - exact).max() * VS32, MARGIN * FIG["torus_mean"]), gauss_sign=(0.0 if sign_ok else 1.0, 0.5))
    raise ValueError(kind)


def assert_analytic(kind, X, r, tag):
    for name, (got, bound) in analytic_figures(kind, X, r).items():
        print(f"{tag} {kind} {name}: {got:.3e} (bound {bound:.3e})")
        assert got <= bound, (kind, name, got, bound)


@pytest.mark.parametrize("kind", SHAPES)
def test_restatement_meets_the_analytic_bounds(kind):
    v, dim, X, lin = shape_volume(kind)
    r = cref.voxels(v, dim, VS, lin)
    assert_analytic(kind, X[lin], r, "restatement float32")
    assert_analytic(kind, X[lin], dict(r["f64"], valid=r["valid"]), "restatement float64")
    # frame and results: unit direction, orthogonal to the gradient's; k1 >= k2; mean and gauss are their symmetric functions
    d = r["f64"]
    assert np.abs(np.linalg.norm(d["dir1"], axis=1) - 1).max() < 1e-14 and (d["k1"] >= d["k2"]).all()
    assert np.abs(d["k1"] + d["k2"] - 2 * d["mean"]).max() * VS32 < 1e-15 and np.abs(d["k1"] * d["k2"] - d["gauss"]).max() * VS32 ** 2 < 1e-14


@pytest.mark.parametrize("kind", SHAPES)
def test_frame_formulation_equals_the_adjugate_formulation(kind):
    v, dim, X, lin = shape_volume(kind)
    r = cref.voxels(v, dim, VS, lin)["f64"]
    mean, gauss = cref.adjugate(v, dim, VS, lin)
    dm, dg = np.abs(r["mean"] - mean).max() * VS32, np.abs(r["gauss"] - gauss).max() * VS32 ** 2
    print(f"{kind}: frame vs adjugate, mean {dm:.2e} / vs, gauss {dg:.2e} / vs^2")
    assert dm < MARGIN * 1e-16 and dg < MARGIN * 1e-16      # the figure the identity was checked at: 1e-16 / vs


def test_validity_rules_of_the_restatement():
    n = 5
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    dist = ((0.36 * i - 0.48 * j + 0.8 * k) * VS).ravel().astype(f32)
    v = dict(dist=dist, weight=np.ones(n ** 3, f32))
    c = (2 * n + 2) * n + 2
    r = cref.voxels(v, (n, n, n), VS, [c, -1, n ** 3, 1 << 40, c, 0])
    assert r["valid"].tolist() == [1, 0, 0, 0, 1, 0] and not r["mean"][[1, 2, 3, 5]].any() and not r["dir1"][[1, 2, 3, 5]].any()
    every = cref.voxels(v, (n, n, n), VS, np.arange(n ** 3))["valid"].reshape(n, n, n)
    assert every[1:-1, 1:-1, 1:-1].all() and every.sum() == 27
    used = 0
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                w = np.ones(n ** 3, f32); w[c + (dk * n + dj) * n + di] = 0
                got = int(cref.voxels(dict(dist=dist, weight=w), (n, n, n), VS, [c])["valid"][0])
                assert got == (1 if abs(di) + abs(dj) + abs(dk) == 3 else 0)      # the 8 cube corners do not matter
                used += 1 - got
    assert used == 19
    assert cref.voxels(dict(dist=np.full(n ** 3, 0.01, f32), weight=np.ones(n ** 3, f32)), (n, n, n), VS, [c])["valid"][0] == 0      # G2 = 0
    down = cref.voxels(dict(dist=(-VS * k).ravel().astype(f32), weight=np.ones(n ** 3, f32)), (n, n, n), VS, [c])      # the normal is -z exactly: sg = -1
    assert down["valid"][0] == 1 and down["mean"][0] == 0 and np.array_equal(down["dir1"][0], f32([1, 0, 0]))


def test_vertex_rule_of_the_restatement():
    n = 6
    lin = lambda i, j, k: (k * n + j) * n + i
    dist = np.zeros(n ** 3, f32); dist[lin(2, 2, 2)] = -0.25; dist[lin(3, 2, 2)] = 0.75; dist[lin(2, 3, 2)] = 0.25
    table = {lin(2, 2, 2): (1, 1.0), lin(3, 2, 2): (1, 3.0), lin(2, 3, 2): (0, 0.0), lin(2, 2, 3): (0, 0.0)}
    def per_voxel(q):
        out = dict(valid=np.array([table.get(int(x), (0, 0.0))[0] for x in q], np.uint8))
        for s, name in enumerate(cref.SCALARS):
            out[name] = np.array([table.get(int(x), (0, 0.0))[1] * (s + 1) for x in q], f32)
        return out
    keys = np.array([4 * lin(2, 2, 2) + 0, 4 * lin(2, 2, 2) + 1, 4 * lin(2, 2, 2) + 3, 4 * lin(2, 3, 2) + 3, 4 * lin(2, 2, 2) + 2, 4 * lin(2, 3, 2) + 0])
    got = cref.vertices(dict(dist=dist), (n, n, n), keys, per_voxel)
    # an x-edge between two valid ends, a quarter of the way; a y-edge to an invalid end; a valid corner; an invalid corner; a z-edge to an invalid end;
    # an edge between two invalid ends
    assert got["valid"].tolist() == [2, 1, 2, 0, 1, 0]
    assert np.array_equal(got["mean"], f32([1.5, 1, 1, 0, 1, 0])) and np.array_equal(got["k2"], f32([6, 4, 4, 0, 4, 0]))


def test_png_byte_rule():
    S = 0.25
    mean = f32([0, S / VS32, -S / VS32, 0.5 * S / VS32, 3.4e38, -3.4e38, 1e-30, 7.0, np.inf, -np.inf])
    valid = np.ones(len(mean), np.uint8); valid[7] = 0
    got = cref.png_byte(mean, valid, VS, S)
    assert got.tolist()[:3] == [128, 255, 0] and got.tolist()[4:] == [255, 0, 128, 128, 255, 0]
    assert got[3] in (191, 192)      # 255 * 0.75 + 0.5 = 191.75, up to the rounding of S / vs to float32
    assert (cref.png_byte(np.zeros(4, f32), np.zeros(4, np.uint8), VS, S) == 128).all()
    ramp = cref.png_byte(np.linspace(-2 * S, 2 * S, 1001).astype(f32) / f32(VS32), np.ones(1001, np.uint8), VS, S)
    assert (np.diff(ramp.astype(int)) >= 0).all() and ramp[0] == 0 and ramp[-1] == 255 and ramp[500] == 128      # convex is bright


def test_library_exports_the_calls(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    names = ["psgsdf_bake_lod_curvature", "psgsdf_curvature_voxels", "psgsdf_extract_mesh_curvature"]
    assert g._declared_symbols("psgsdf_curvature.h") == names
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, s) for s in names), path
    assert all(hasattr(capi.Api, s) for s in ("curvature_voxels", "extract_mesh_curvature", "bake_lod_curvature"))
    assert (ctypes.sizeof(capi.Bake), ctypes.sizeof(capi.BakeCurvature)) == (168, 192)
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    P = ctypes.c_void_p
    vox = lib.psgsdf_curvature_voxels; vox.argtypes = [P, P, ctypes.c_int64] + [P] * 6
    msh = lib.psgsdf_extract_mesh_curvature; msh.argtypes = [P] * 12
    bake = lib.psgsdf_bake_lod_curvature; bake.argtypes = [P, P, ctypes.c_double, ctypes.c_int32, ctypes.c_double, P]
    ARG, STATE = -1, -4
    lin = (ctypes.c_int64 * 2)(5, 6)
    outs = [P(0x10) for _ in range(11)]
    refs = [ctypes.byref(o) for o in outs]
    for k in range(6):                                   # a NULL output pointer
        assert vox(None, lin, 2, *[None if i == k else r for i, r in enumerate(refs[:6])]) == ARG
    assert vox(None, None, 2, *refs[:6]) == ARG and vox(None, lin, -1, *refs[:6]) == ARG
    for k in range(11):
        assert msh(None, *[None if i == k else r for i, r in enumerate(refs)]) == ARG
    out = capi.BakeCurvature(); out.n_valid = 77
    assert bake(None, None, 1.0, 4, 1.0, None) == ARG
    for cell, res, reach in ((0.0, 4, 1.0), (1.0, 0, 1.0), (1.0, 4, float("nan")), (float("inf"), 4, 1.0)):      # what psgsdf_bake_lod refuses
        assert bake(None, None, cell, res, reach, ctypes.byref(out)) == ARG
    # everything in order but the context: PSGSDF_ERR_STATE, nothing touched
    assert vox(None, lin, 2, *refs[:6]) == STATE and vox(None, None, 0, *refs[:6]) == STATE and msh(None, *refs) == STATE
    assert bake(None, None, 1.0, 4, 1.0, ctypes.byref(out)) == STATE
    assert all(o.value == 0x10 for o in outs) and out.n_valid == 77


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_curvature.c"
    src.write_text('#include "psgsdf_curvature.h"\n'
                   'typedef char bake_size[sizeof(psgsdf_bake) == 168 ? 1 : -1];\ntypedef char curv_size[sizeof(psgsdf_bake_curvature) == 192 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, const int64_t* lin) {\n    const uint8_t* v; const float* m; const float* g; const float* k1; const float* k2; const float* d;\n'
                   '    const float* x; const float* n; const uint8_t* rgb; const int32_t* f; int64_t nv, nf; psgsdf_bake_curvature b; int rc;\n'
                   '    rc = psgsdf_curvature_voxels(c, lin, 3, &v, &m, &g, &k1, &k2, &d);\n'
                   '    if (!rc) rc = psgsdf_extract_mesh_curvature(c, &x, &n, &rgb, &nv, &f, &nf, &v, &m, &g, &k1, &k2);\n'
                   '    if (!rc) rc = psgsdf_bake_lod_curvature(c, 0, 0.02, 8, 0.02, &b);\n    return rc ? rc : (int)(b.n_valid + b.bake.width + nv + nf);\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_curvature.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def read_ply_curvature(path):
    """(header lines, vertex records, faces) of `voxelPS --mesh-curvature`'s file: the welded mesh's records with quality, gauss, k1, k2, curvature_valid
    behind the colours"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("quality", "<f4"), ("gauss", "<f4"), ("k1", "<f4"), ("k2", "<f4"), ("curvature_valid", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize and vt.itemsize == 44
    props = [h for h in head if h.startswith("property")]
    assert props[:9] == ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                         "property uchar red", "property uchar green", "property uchar blue"]
    assert props[9:] == ["property float quality", "property float gauss", "property float k1", "property float k2", "property uchar curvature_valid",
                         "property list uchar int vertex_indices"]
    verts = np.frombuffer(raw, vt, nv, end)
    fc = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (fc["n"] == 3).all()
    return head, verts, fc["v"].copy()


def assert_header_matches_columns(head, verts):
    w = next(h for h in head if h.startswith("comment curvature mean ")).split()
    assert w[4] == "valid" and len(w) == 6
    ok = verts["curvature_valid"] > 0
    exp = float(np.cumsum(verts["quality"][ok].astype(np.float64))[-1] / ok.sum()) if ok.any() else 0.0      # (a running sum in vertex order, as the writer adds)
    assert int(w[5]) == int(ok.sum()) and float(w[3]) == exp, (w, exp)
    assert w[3] == "%.17g" % exp


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_selftest_ply_curvature_parses_back(tmp_path):
    out, plain = str(tmp_path / "octa_curvature.ply"), str(tmp_path / "octa.ply")
    for flag, path in (("--selftest-ply-curvature", out), ("--selftest-ply-indexed", plain)):
        r = subprocess.run([EXE, flag, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
    head, verts, faces = read_ply_curvature(out)
    phead, pverts, pfaces = read_ply_indexed(plain)
    assert np.array_equal(faces, pfaces)
    for k in pverts.dtype.names:
        assert np.array_equal(verts[k], pverts[k]), k
    assert np.array_equal(verts["quality"], f32([0.5, -0.25, 0.0, 8.0, 0.125, -3.0])) and np.array_equal(verts["gauss"], f32([0.25, 0.0625, 0.0, -4.0, 0.01, 9.0]))
    assert np.array_equal(verts["k1"], f32([0.75, -0.125, 0.0, 16.0, 0.25, -3.0])) and np.array_equal(verts["k2"], f32([0.25, -0.375, 0.0, -0.25, 0.04, -3.0]))
    assert list(verts["curvature_valid"]) == [2, 1, 0, 2, 1, 2]
    assert_header_matches_columns(head, verts)
    assert next(h for h in head if h.startswith("comment curvature")) == "comment curvature mean 1.075 valid 5"
    assert [h for h in head if not h.startswith(("comment curvature", "property"))] == [h for h in phead if not h.startswith("property")]


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_the_flags_while_parsing(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    bake = ["--mesh-lod", "2", "--mesh-bake", "4"]
    for extra, words in ((["--mesh-lod", "2", "--mesh-bake-curvature", "0.1"], ("--mesh-bake-curvature", "--mesh-bake")), (["--mesh-bake-curvature", "0.1"], ("--mesh-bake-curvature", "--mesh-bake")),
                         (bake + ["--mesh-bake-curvature", "0.1", "--gpus", "2"], ("--mesh-bake-curvature", "--gpus")), (["--mesh-curvature", "--gpus", "2"], ("--mesh-curvature", "--gpus")),
                         (bake + ["--mesh-bake-curvature", "0"], ("--mesh-bake-curvature", "> 0")), (bake + ["--mesh-bake-curvature", "-1"], ("--mesh-bake-curvature",)),
                         (bake + ["--mesh-bake-curvature", "nan"], ("--mesh-bake-curvature",)), (bake + ["--mesh-bake-curvature", "inf"], ("--mesh-bake-curvature",)),
                         (bake + ["--mesh-bake-curvature", "0.1x"], ("--mesh-bake-curvature",)), (bake + ["--mesh-bake-curvature", "x"], ("--mesh-bake-curvature",))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_curvature_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("curvature.hip", tmp_path).items() if "k_" in k}
    print(ks)
    assert len(ks) == 3 and sorted(n for n in ("k_curv_voxels", "k_wmesh_curv", "k_bake_curv") if any(n in k for k in ks)) == ["k_bake_curv", "k_curv_voxels", "k_wmesh_curv"], ks
    assert all(v["scratch"] == 0 for v in ks.values()), ks
    src = open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "curvature.hip")).read()
    assert src.count("__shared__") == 0 and src.count("atomic") == 1      # (the one in the file's comment: "No atomics")
