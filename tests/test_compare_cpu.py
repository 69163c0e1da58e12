"""Comparison with a reference without a GPU (include/psgsdf_compare.h, DESIGN.md "Comparison with a reference"): the yardstick
tests/_compare_ref.py -- its pair function against an independent formulation, its fixed-point rules in exact fractions, the welded mesh of the
five pieces against clouds on the analytic spheres -- and the interface off the device: the header as C99, the exported symbol and struct sizes,
the call's returns without a context, the refusals of `voxelPS --compare-ply` and the new kernels' resources."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _compare_ref as cref
import _mesh_ref as mref
from test_mesh_components_cpu import EXE, HIPCC, ROOT, SPHERES, pieces_volume

f32, f64 = np.float32, np.float64


def independent(p, a, b, c):
    """D2 another way: the foot of the perpendicular if it lies in the triangle (barycentric signs), else the nearest of the three segments"""
    def segment(p, u, v):
        e = v - u
        t = np.clip(np.dot(p - u, e) / np.dot(e, e), 0.0, 1.0)
        w = p - (u + t * e)
        return np.dot(w, w)
    n = np.cross(b - a, c - a)
    foot = p - n * (np.dot(p - a, n) / np.dot(n, n))
    s = [np.dot(np.cross(v - u, foot - u), n) for u, v in ((a, b), (b, c), (c, a))]
    if all(x >= 0 for x in s):
        return np.dot(p - a, n) ** 2 / np.dot(n, n)
    return min(segment(p, a, b), segment(p, b, c), segment(p, c, a))


def test_pair_function_against_an_independent_formulation():
    rng = np.random.default_rng(16)
    worst, seen = 0.0, set()
    for _ in range(50):
        a, b, c = rng.normal(size=(3, 3))
        n = np.cross(b - a, c - a); nn = n / np.linalg.norm(n)
        # 40 random points around it, and one hand-placed point in each of the seven regions (lifted off the plane)
        away = lambda u, v, w: u - ((v - u) / np.linalg.norm(v - u) + (w - u) / np.linalg.norm(w - u))      # from corner u against its angle's bisector
        hand = [away(a, b, c), away(b, a, c), 0.5 * (a + b) + 0.3 * np.cross(b - a, nn), away(c, a, b), 0.5 * (a + c) + 0.3 * np.cross(nn, c - a),
                0.5 * (b + c) + 0.3 * np.cross(c - b, nn), (a + b + c) / 3]
        P = np.concatenate([(a + b + c) / 3 + 2 * rng.normal(size=(40, 3)), np.array(hand) + 0.7 * nn])
        D2, q, region = cref.pair(P, a, b, c)
        assert region[40:].tolist() == list(range(7)), region[40:]
        seen |= set(region.tolist())
        for j in range(len(P)):
            want = independent(P[j], a, b, c)
            worst = max(worst, abs(D2[j] - want) / want)
    print(f"pair function: 50 triangles x 47 points, regions seen {sorted(seen)}, worst relative difference {worst:.2e}")
    assert seen == set(range(7))
    assert worst <= 1e-12      # double rounding of two different operation orders, not a measurement


def test_point_targets_and_collinear_triangles():
    rng = np.random.default_rng(17)
    p, a = rng.normal(size=(2, 200, 3))
    D2, q, region = cref.pair(p, a, a, a)
    w = p - a
    assert np.array_equal(D2, (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) and np.array_equal(q, a) and not region.any()      # |p - a|^2 exactly
    # a repeated corner (a = b) met from c's side: the edge parameter is 0 / 0, D2 is not finite
    a, c, p = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.5, 0.25, 0])
    D2, _, region = cref.pair(p, a, a, c)
    assert not np.isfinite(D2) and region == 2
    # ... and such a pair takes no part: the nearest target is the other one, whatever its index
    xyz = f32([[0, 0, 0], [1, 0, 0], [0, 5, 0], [1, 5, 0], [0, 6, 0]])
    for faces in ([[0, 0, 1], [2, 3, 4]], [[2, 3, 4], [0, 0, 1]]):
        r = cref.nearest(f32([p]), xyz, np.array(faces), 64.0)
        assert r["nearest"][0] == faces.index([2, 3, 4]) and r["d"][0] == 4.75 and r["side"][0] == 0
    # ties go to the smaller index; a vertex region returns the vertex itself, so two faces sharing it give the same bits
    xyz = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 2, 0]])
    r = cref.nearest(f32([[-0.1, -0.1, 0.3], [np.nan, 0, 0], [0, 0, 9]]), xyz, np.array([[0, 1, 2], [0, 3, 4]]), 1.0)
    assert r["nearest"].tolist() == [0, -1, -1] and r["side"].tolist() == [1, 0, 0]
    assert np.isnan(r["dist"][1]) and np.isinf(r["dist"][2]) and r["valid"].tolist() == [True, False, True] and r["matched"].tolist() == [True, False, False]


def test_fixed_point_rules_in_exact_fractions():
    vs = float(f32(0.01))
    for mult in (8, 64, 0.5):
        max_dist = mult * vs
        for k in range(17):
            d = max_dist * k / 16                      # exact: 24 bits times at most 5, and a power of two
            assert Fraction(16) * Fraction(d) / Fraction(max_dist) == k
            assert int(cref.hist_bin(np.array([d]), max_dist)[0]) == min(15, k), (mult, k)      # d = max_dist itself: bin 15
        assert int(cref.hist_bin(np.array([np.nextafter(max_dist, 0)]), max_dist)[0]) == 15
    # sum_d2 at the bound: every one of 2^31 - 1 queries at d = max_dist = 64 vs adds 2^32
    d = 64 * vs
    u = d / vs
    assert Fraction(u) == 64 and int(np.rint(u * u * cref.UNIT)) == 2 ** 32 == Fraction(u) ** 2 * 2 ** 20
    assert (2 ** 31 - 1) * 2 ** 32 < 2 ** 63 and (2 ** 31 - 1) * int(np.rint(u * cref.UNIT)) < 2 ** 63
    # rounding to nearest, ties to even, as llrint does
    assert np.rint(np.array([0.5, 1.5, 2.5, -0.5])).tolist() == [0.0, 2.0, 2.0, -0.0]
    r = dict(d=np.array([0.25 * vs, 0.5 * vs, np.inf, np.nan]), valid=np.array([1, 1, 1, 0], bool), matched=np.array([1, 1, 0, 0], bool), side=np.array([1, -1, 0, 0], np.int8))
    s = cref.side_stats(r, vs, 8 * vs, 0.3 * vs)
    assert (s["n"], s["n_valid"], s["n_matched"], s["n_within_tau"]) == (4, 3, 2, 1)
    assert (s["sum_d"], s["sum_d2"], s["sum_signed"]) == (3 * 2 ** 18, 2 ** 16 + 2 ** 18, -2 ** 18)
    assert s["hist"].tolist() == [1, 1] + [0] * 14 and s["max"] == 0.5 * vs
    assert s["mean"] == vs * 0.375 and s["rms"] == vs * np.sqrt(0.15625) and s["mean_signed"] == vs * -0.125
    assert cref.scores(dict(n_within_tau=1, n_valid=2), dict(n_within_tau=0, n_valid=0)) == (0.5, 0.0, 0.0)
    for bad in ((65 * vs, vs), (0.0, 0.0), (vs, 2 * vs), (float("nan"), vs), (vs, float("inf"))):
        with pytest.raises(ValueError):
            cref.check_params(vs, *bad)


def test_five_pieces_against_clouds_on_the_analytic_spheres():
    """A vertex of the welded mesh is the zero of the LINEAR interpolant of the distance along a grid edge of length vs.  Along a straight line
    the distance to a sphere's surface, |x - c| - R, is convex with second derivative sin^2 / |x - c| <= 1 / R where it is zero, so the interpolant
    lies above it by at most vs^2 / (8 R): a vertex sits inside the analytic sphere, by at most eps = vs^2 / (8 R) plus the float32 rounding of
    its coordinates (2^-24 of the largest one, per axis).  That is the bound checked on the vertices, with R from SPHERES.
    The clouds on the analytic spheres go through the yardstick against the mesh's faces.  A flat triangle with its corners within eps of the
    sphere and edges no longer than L has a circumradius of at most L / sqrt(3), so the sphere bulges over it by at most the sagitta
    R - sqrt(R^2 - L^2 / 3): every cloud point is within eps + that of the mesh, L being the longest edge found next to that sphere (marching
    cubes: below sqrt(3) vs), and on the outer side of it."""
    v, dim, vs = pieces_volume()
    xyz, nrm, rgb, faces, _ = mref.mesh(v, dim, vs)
    assert (len(xyz), len(faces)) == (3612, 7204)
    vs = float(f32(vs)); L = dim[0] * vs
    rounding = 3 ** 0.5 * 2.0 ** -24 * float(np.abs(xyz).max())
    X = xyz.astype(f64)
    for cs, R in SPHERES:
        c = np.array(cs) * L
        radial = np.linalg.norm(X - c, axis=1) - R * vs
        near = np.abs(radial) < 0.6 * vs                       # this sphere's vertices: the pieces are many voxels apart
        eps = vs * vs / (8 * R * vs) + rounding
        fc = faces[near[faces].all(1)]
        edge = max(float(np.linalg.norm(X[fc[:, i]] - X[fc[:, (i + 1) % 3]], axis=1).max()) for i in range(3))
        sagitta = R * vs - np.sqrt((R * vs) ** 2 - edge * edge / 3)
        cloud = cref.fibonacci(400, c, R * vs)
        r = cref.nearest(cloud, xyz, faces, 8 * vs)
        print(f"sphere R = {R} vs: {int(near.sum())} vertices, radial error {radial[near].min() / vs:.4f} .. {radial[near].max() / vs:.2e} vs, bound vs^2 / (8 R) + rounding = "
              f"{eps / vs:.4f} vs; longest edge {edge / vs:.3f} vs, cloud -> mesh max {r['d'].max() / vs:.4f} vs, mean {r['d'].mean() / vs:.4f} vs, bound {(eps + sagitta) / vs:.4f} vs")
        assert near.sum() > 20 and len(fc) > 40 and edge < 3 ** 0.5 * vs
        assert -eps <= radial[near].min() and radial[near].max() <= rounding
        assert r["matched"].all() and near[faces[r["nearest"]]].all()
        assert r["d"].max() <= eps + sagitta
        assert (r["side"] == 1).all()


def test_library_exports_the_call(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_compare.h") == ["psgsdf_compare_reference"]
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        assert hasattr(ctypes.CDLL(path), "psgsdf_compare_reference"), path
    assert hasattr(capi.Api, "compare_reference")
    assert (ctypes.sizeof(capi.CompareParams), ctypes.sizeof(capi.CompareSide), ctypes.sizeof(capi.Compare)) == (32, 216, 552)
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    P = ctypes.c_void_p
    f = lib.psgsdf_compare_reference; f.argtypes = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, P, P]
    good = capi.CompareParams(0.08, 0.01, 0.0, (ctypes.c_int32 * 2)(0, 0))
    out = capi.Compare()
    x = (ctypes.c_float * 9)(*range(9)); tri = (ctypes.c_int32 * 3)(0, 1, 2)
    ARG, STATE = -1, -4
    pg, po = ctypes.byref(good), ctypes.byref(out)
    assert f(None, None, x, 3, tri, 1, None, po) == ARG and f(None, None, x, 3, tri, 1, pg, None) == ARG and f(None, None, None, 3, tri, 1, pg, po) == ARG
    assert f(None, None, x, -1, None, 0, pg, po) == ARG and f(None, None, x, 3, tri, -1, pg, po) == ARG and f(None, None, x, 3, None, 1, pg, po) == ARG
    for bad_tri in ((0, 1, 3), (-1, 1, 2)):                      # a face index outside [0, n_ref)
        assert f(None, None, x, 3, (ctypes.c_int32 * 3)(*bad_tri), 1, pg, po) == ARG
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.01, 0.0, 0, 0), (-1.0, 0.01, 0.0, 0, 0), (nan, 0.01, 0.0, 0, 0), (inf, 0.01, 0.0, 0, 0), (0.08, 0.0, 0.0, 0, 0), (0.08, nan, 0.0, 0, 0), (0.08, 0.09, 0.0, 0, 0),
                (0.08, 0.01, -1.0, 0, 0), (0.08, 0.01, nan, 0, 0), (0.08, 0.01, inf, 0, 0), (0.08, 0.01, 0.0, 1, 0), (0.08, 0.01, 0.0, 0, 1)):
        p = capi.CompareParams(bad[0], bad[1], bad[2], (ctypes.c_int32 * 2)(bad[3], bad[4]))
        assert f(None, None, x, 3, tri, 1, ctypes.byref(p), po) == ARG, bad
    for flt in (capi.MeshFilter(0, nan, 0), capi.MeshFilter(0, 0.0, -1)):      # what psgsdf_extract_mesh_components refuses
        assert f(None, ctypes.byref(flt), x, 3, tri, 1, pg, po) == ARG
    # everything in order but the context: PSGSDF_ERR_STATE, nothing touched
    assert f(None, None, x, 3, tri, 1, pg, po) == STATE and f(None, None, x, 3, None, 0, pg, po) == STATE and f(None, None, None, 0, None, 0, pg, po) == STATE
    assert bytes(out) == bytes(ctypes.sizeof(capi.Compare))


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_compare.c"
    src.write_text('#include "psgsdf_compare.h"\n'
                   'typedef char params_size[sizeof(psgsdf_compare_params) == 32 ? 1 : -1];\ntypedef char side_size[sizeof(psgsdf_compare_side) == 216 ? 1 : -1];\n'
                   'typedef char compare_size[sizeof(psgsdf_compare) == 552 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, const float* x, const int32_t* f) {\n    psgsdf_compare_params p; psgsdf_compare r; int rc;\n'
                   '    p.max_dist = 0.08; p.tau = 0.01; p.grid_cell = 0.0; p.reserved[0] = p.reserved[1] = 0;\n    rc = psgsdf_compare_reference(c, 0, x, 3, f, 1, &p, &r);\n'
                   '    return rc ? rc : (int)(r.to_reference.n_matched + r.to_reconstruction.hist[15] + r.n_faces + r.vertex_side[0]) + (r.fscore > 0.5);\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_compare.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_compare_on_several_gpus_an_unreadable_file_and_bad_numbers(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    ply = tmp_path / "ref.ply"
    ply.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                   "0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    bad = tmp_path / "bad.ply"
    bad.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nend_header\n0 0\n1 0\n0 1\n")
    for extra, words in ((["--compare-ply", str(ply), "--gpus", "2"], ("--compare-ply", "--gpus")), (["--compare-ply", str(tmp_path / "missing.ply")], ("--compare-ply", "missing.ply")),
                         (["--compare-ply", str(bad)], ("--compare-ply", "bad.ply")), (["--compare-ply", str(ply), "--compare-tau", "x"], ("--compare-tau",)),
                         (["--compare-ply", str(ply), "--compare-tau", "0"], ("--compare-tau",)), (["--compare-ply", str(ply), "--compare-max", "65"], ("--compare-max",)),
                         (["--compare-ply", str(ply), "--compare-max", "nan"], ("--compare-max",)), (["--compare-ply", str(ply), "--compare-tau", "9"], ("--compare-tau",)),
                         (["--compare-tau", "1"], ("--compare-tau", "--compare-ply"))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


def read_compare_ply(path):
    """a <name>_mesh_compare.ply: (header lines, structured vertex array, faces [f, 3])"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[2]); nf = int(next(h for h in head if h.startswith("element face")).split()[2])
    vt = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("rgb", "u1", (3,)), ("distance", "<f4"), ("side", "i1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert vt.itemsize == 32 and ft.itemsize == 13 and len(raw) == end + 32 * nv + 13 * nf
    v = np.frombuffer(raw, vt, nv, end); f = np.frombuffer(raw, ft, nf, end + 32 * nv)
    assert (f["n"] == 3).all()
    return head, v, f["v"]


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_compare_ply_writer_and_reader(tmp_path):
    out = tmp_path / "octa.ply"
    r = subprocess.run([EXE, "--selftest-ply-compare", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr      # (0: the reader returned the positions and faces that were written)
    head, v, f = read_compare_ply(out)
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "comment grid origin -0.25 0.5 1 voxel size 0.00400000019"] and head[3] == "comment compare selftest"
    assert head[-5:-3] == ["property float distance", "property char side"]
    assert np.array_equal(v["xyz"], f32([[1.5, 0, 0], [-1.5, 0, 0], [0, 2.25, 0], [0, -2.25, 0], [0, 0, 0.75], [0, 0, -0.75]]))
    assert np.array_equal(v["distance"], f32([0.125, 0.03125, 0, np.inf, 0.0625, 0.5])) and v["side"].tolist() == [1, -1, 0, 0, -1, 1]
    assert f.tolist() == [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_compare_kernels_use_no_scratch_and_no_lds(tmp_path):
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("compare.hip", tmp_path).items() if "k_cmp_" in k}
    assert len(ks) == 5 and all(v["scratch"] == 0 for v in ks.values()), ks      # total, count, fill, query, stats
    assert open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "compare.hip")).read().count("__shared__") == 0
