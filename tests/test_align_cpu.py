"""Alignment of a reference (include/psgsdf_align.h, DESIGN.md "Alignment of a reference") without a GPU: the yardstick tests/_align_ref.py itself --
its rows against finite differences, its pruned search against the exhaustive one, the convergence cases and the pivot margins on both sides of
the degeneracy threshold -- and what surrounds the device code: struct sizes, exports and argument checks, voxelPS's flags, kernel resources."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _align_ref as aref
import _compare_ref as cref
import _mesh_ref as mref
from test_mesh_components_cpu import EXE, HIPCC, ROOT, SPHERES, pieces_volume
from test_occlusion_cpu import plane, plane_samples

f32, f64 = np.float32, np.float64
N = 48
AXIS = (0.3, -0.5, 0.8)


@functools.lru_cache(maxsize=None)
def pieces_mesh():
    v, dim, vs = pieces_volume(torus=True)
    xyz, nrm, rgb, faces, _ = mref.mesh(v, dim, vs)
    assert (len(xyz), len(faces)) == (4280, 8540)
    return xyz, nrm, faces, float(f32(vs))


def motion(xyz, vs, degrees, shift):
    """`degrees` about AXIS through the vertex mean, then `shift` voxels along (1, -2, 2) / 3"""
    return aref.rigid(AXIS, degrees, shift * vs * np.array([1.0, -2.0, 2.0]) / 3.0, np.asarray(xyz, f64).mean(0))


def displacement(xyz, vs, T, M):
    """how far T o M^-1 moves the mesh's vertices, in voxels (M took the reference away, T should bring it back)"""
    X = np.asarray(xyz, f64)
    return float(np.linalg.norm(aref.apply((T @ aref.rigid_inverse(M))[:3], X) - X, axis=1).max()) / vs


def sphere_cloud(vs):
    """600 Fibonacci points on the four analytic spheres"""
    return np.concatenate([cref.fibonacci(150, np.array(cs) * N * vs, R * vs) for cs, R in SPHERES])


def test_exp_is_orthonormal_and_delta_inverts():
    rng = np.random.default_rng(5)
    for om in [np.zeros(3), [1e-12, 0, 0], [3e-9, -4e-9, 1e-9], [1e-8, 0, 0], [1e-5, 2e-5, -1e-5], [0.01, 0.02, 0.03], [0.3, -0.5, 0.8], [2.0, 1.0, -2.0]] + list(rng.normal(size=(20, 3))):
        E = aref.exp_so3(om)
        assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-15, om
        assert np.abs(E @ np.asarray(om, f64) - np.asarray(om, f64)).max() <= 1e-15 * max(1.0, np.linalg.norm(om))      # the axis stays
    # the series and the closed form meet at the switch
    a = np.array([1e-8, 0, 0]) * (1 - 1e-9); b = np.array([1e-8, 0, 0]) * (1 + 1e-9)
    assert np.abs(aref.exp_so3(a) - aref.exp_so3(b)).max() <= 1e-16
    # compose is Delta o T, and the inverse of a rigid transform undoes it
    T = aref.rigid(AXIS, 8.0, [0.01, -0.02, 0.03], [0.2, 0.2, 0.2])
    c = np.array([0.25, 0.2, 0.3]); om = np.array([0.01, -0.02, 0.005]); v = np.array([1e-3, 2e-3, -1e-3])
    D = np.eye(4); D[:3] = aref.delta(om, v, c)
    assert np.abs(aref.compose(T[:3], om, v, c) - (D @ T)[:3]).max() <= 1e-15
    assert np.abs(T @ aref.rigid_inverse(T) - np.eye(4)).max() <= 1e-15
    p = f32([[0.1, 0.2, 0.3], [np.nan, 0, 0], [0, np.inf, 0]])
    m = aref.move(T[:3], p)
    assert m.dtype == f32 and np.isfinite(m[0]).all() and not np.isfinite(m[1]).any() and not np.isfinite(m[2]).all()


@pytest.mark.parametrize("direction", [1, 2])
def test_rows_are_the_derivative_of_the_residual(direction):
    """for frozen correspondences, each J row is the central finite difference of rho under Delta, to 1e-6 relative"""
    xyz, nrm, faces, vs = pieces_mesh()
    M = motion(xyz, vs, 3.0, 1.5)
    cloud = aref.move(aref.rigid_inverse(M)[:3], sphere_cloud(vs))
    T = np.eye(4)[:3]; c = aref.bbox_centre(xyz)
    r = aref.rows(direction, T, xyz, nrm, faces, cloud, None, 8 * vs, c, vs, search=aref.pruned_nearest)
    J, rho, m, j = r["J"], r["rho"], r["query"], r["target"]
    assert len(rho) > 500 and J.shape == (len(rho), 6)
    # the frozen pair: direction 1: the moved point x against its closest point q and the face's normal; direction 2: x = T q against the vertex
    if direction == 1:
        a, b, cc, _ = cref.corners(xyz, faces)
        x = r["moved"][m].astype(f64)
        _, q, _ = cref.pair(x, a[j], b[j], cc[j])
        n = aref.cross(b[j] - a[j], cc[j] - a[j]); anchor = q
    else:
        q = cloud[j].astype(f64)
        x = aref.apply(T, q)
        n = nrm[m].astype(f64); anchor = xyz[m].astype(f64)
    n = n / np.sqrt(aref.dot(n, n))[:, None]
    assert np.abs(aref.dot(n, x - anchor) / vs - rho).max() <= 1e-12

    def residual(xi):
        D = aref.delta(xi[:3], xi[3:] * vs, c)
        return aref.dot(n, aref.apply(D, x) - anchor) / vs

    h = 1e-5
    scale = np.abs(J).max(1)
    worst = 0.0
    for k in range(6):
        e = np.zeros(6); e[k] = h
        fd = (residual(e) - residual(-e)) / (2 * h)
        worst = max(worst, float((np.abs(fd - J[:, k]) / scale).max()))
    print(f"direction {direction}: {len(rho)} rows, |finite difference - J| <= {worst:.2e} of the row's largest entry")
    assert worst <= 1e-6


def test_pruned_search_returns_the_exhaustive_matches():
    xyz, nrm, faces, vs = pieces_mesh()
    M = motion(xyz, vs, 3.0, 1.5)
    cloud = aref.move(aref.rigid_inverse(M)[:3], sphere_cloud(vs))
    cloud[5] = np.nan; cloud[9] = f32([200, 200, 200]) * f32(vs)
    for q, t_xyz, t_faces in ((cloud, xyz, faces), (xyz[::7], cloud, None)):
        for radius in (8 * vs, 1.0 * vs):
            a, b = cref.nearest(q, t_xyz, t_faces, radius), aref.pruned_nearest(q, t_xyz, t_faces, radius)
            assert 0 < b["matched"].sum() < len(q)
            for k in ("nearest", "matched", "valid"):
                assert np.array_equal(a[k], b[k]), k
            assert a["dist"].tobytes() == b["dist"].tobytes()


@functools.lru_cache(maxsize=None)
def run_cloud(degrees, shift, directions):
    xyz, nrm, faces, vs = pieces_mesh()
    M = motion(xyz, vs, degrees, shift)
    cloud = aref.move(aref.rigid_inverse(M)[:3], sphere_cloud(vs))
    r = aref.align(xyz, nrm, faces, cloud, None, vs, directions=directions, search=aref.pruned_nearest)
    return r, displacement(xyz, vs, r["transform"], M)


def test_own_copy_is_recovered_exactly():
    """the mesh's own copy, moved 3 degrees / 1.5 voxels, direction 1: quadratic convergence to rms 0"""
    xyz, nrm, faces, vs = pieces_mesh()
    M = motion(xyz, vs, 3.0, 1.5)
    ref = aref.move(aref.rigid_inverse(M)[:3], xyz)
    r = aref.align(xyz, nrm, faces, ref, faces, vs, directions=1, search=aref.pruned_nearest)
    rms = [it["rms"] / vs for it in r["iters"]]
    d = displacement(xyz, vs, r["transform"], M)
    print(f"own copy: status {r['status']} after {r['n_iters']} steps, rms {['%.3g' % x for x in rms]} -> {r['final']['rms'] / vs:.3g} vs, displacement {d:.2e} vs")
    assert r["status"] == aref.CONVERGED and r["n_iters"] <= 5
    assert 0.5 < rms[0] < 1.5 and rms[1] < 0.2 * rms[0] and rms[2] < 0.01 * rms[1]
    assert r["final"]["rms"] / vs <= 1e-5 and d <= 1e-5      # (the reference's float32 rounding, ~3e-6 vs, is all that is left)
    assert min(it["min_pivot"] for it in r["iters"]) >= 100 * aref.PIVOT_MIN


@pytest.mark.parametrize("degrees,shift,directions", [(3.0, 1.5, 1), (8.0, 3.0, 1), (3.0, 1.5, 2), (3.0, 1.5, 3), (8.0, 3.0, 3)])
def test_sphere_clouds_converge(degrees, shift, directions):
    """600 points on the analytic spheres against the mesh, whose vertices lie up to vs^2 / (8 R) inside them (test_compare_cpu): the residual
    displacement is of that size, not zero.  The same answer from both motions."""
    xyz, nrm, faces, vs = pieces_mesh()
    r, d = run_cloud(degrees, shift, directions)
    small, _ = run_cloud(3.0, 1.5, directions)
    last = r["iters"][-1]["step"]
    print(f"cloud {degrees} deg / {shift} vs, directions {directions}: status {r['status']} after {r['n_iters']} steps, displacement {d:.4f} vs, final rms {r['final']['rms'] / vs:.4f} vs, "
          f"pairs {r['final']['n_pairs']}, smallest pivot {min(it['min_pivot'] for it in r['iters']):.3f}, last step {np.linalg.norm(last[:3]):.1e} rad {np.linalg.norm(last[3:]) / vs:.1e} vs")
    assert r["status"] == aref.CONVERGED and r["n_iters"] <= 9
    assert d <= 0.03                                                         # vs^2 / (8 R) is 0.031 vs for the smallest sphere (R = 4)
    # both runs stopped after a step below eps_trans = 1e-3 vs and eps_rot = 1e-5 rad (2.5e-4 vs at the 25 voxels the farthest vertex is from the centre)
    # while converging at least linearly with a ratio below a half, so each is within 1.25e-3 vs of the fixed point and the two within 2.5e-3 vs
    X = xyz.astype(f64)
    A, B = r["transform"] @ aref.rigid_inverse(motion(xyz, vs, degrees, shift)), small["transform"] @ aref.rigid_inverse(motion(xyz, vs, 3.0, 1.5))
    assert np.linalg.norm(aref.apply(A[:3], X) - aref.apply(B[:3], X), axis=1).max() <= 2.5e-3 * vs
    assert min(it["min_pivot"] for it in r["iters"]) >= 100 * aref.PIVOT_MIN      # every pieces case: at least 100x above the threshold
    assert r["final"]["n_pairs"][0] == (600 if directions & 1 else 0) and (r["final"]["n_pairs"][1] > 700) == bool(directions & 2)


def test_plane_is_degenerate():
    """a plane leaves three motions free: the smallest pivot is at least 100x below the threshold, and no step is taken"""
    v, dim, n = plane()
    vs = float(f32(0.01))
    xyz, nrm, rgb, faces, _ = mref.mesh(v, dim, 0.01)
    q, m = plane_samples()
    cloud = (q.astype(f64) + 0.37 * vs * m.astype(f64)).astype(f32)
    for directions in (1, 3):
        r = aref.align(xyz, nrm, faces, cloud, None, vs, directions=directions, search=aref.pruned_nearest)
        mp = r["iters"][0]["min_pivot"]
        print(f"plane, directions {directions}: status {r['status']}, pairs {r['final']['n_pairs']}, smallest pivot {mp:.3e}")
        assert r["status"] == aref.DEGENERATE and r["n_iters"] == 0 and len(r["iters"]) == 1
        assert mp <= aref.PIVOT_MIN / 100
        assert np.array_equal(r["transform"], np.eye(4)) and r["final"]["n_pairs"][0] == 300
    # fewer than 6 rows
    r = aref.align(xyz, nrm, faces, cloud[:3], None, vs, directions=1)
    assert r["status"] == aref.TOO_FEW and r["n_iters"] == 0 and np.array_equal(r["transform"], np.eye(4))


def _c_sizes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "psgsdf_align.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(psgsdf_align_params), sizeof(psgsdf_align_iter), sizeof(psgsdf_align), offsetof(psgsdf_align, iters),\n'
                   '           offsetof(psgsdf_align, system0), offsetof(psgsdf_align, aligned_xyz), offsetof(psgsdf_align_params, directions));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]


def test_struct_sizes_agree_between_c_and_python(tmp_path):
    from psgradientsdf_amd import capi
    got = _c_sizes(tmp_path)
    want = [ctypes.sizeof(capi.AlignParams), ctypes.sizeof(capi.AlignIter), ctypes.sizeof(capi.Align), capi.Align.iters.offset, capi.Align.system0.offset, capi.Align.aligned_xyz.offset,
            capi.AlignParams.directions.offset]
    assert got == want == [192, 88, 6168, 160, 5792, 6104, 176], (got, want)


def test_library_exports_the_call_and_checks_its_arguments(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    assert g._declared_symbols("psgsdf_align.h") == ["psgsdf_align_reference"]
    assert hasattr(capi.Api, "align_reference")
    P = ctypes.c_void_p
    ARG, STATE = -1, -4
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        assert hasattr(ctypes.CDLL(path), "psgsdf_align_reference"), path
    f = ctypes.CDLL(capi.ENGINE_LIB).psgsdf_align_reference; f.argtypes = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, P, P]

    def params(init=None, max_dist=0.08, min_dist=0.01, shrink=1.0, eps_rot=1e-5, eps_trans=1e-5, grid_cell=0.0, directions=3, max_iters=30, reserved=(0, 0)):
        T = np.eye(4) if init is None else np.asarray(init, f64)
        return capi.AlignParams((ctypes.c_double * 16)(*T.ravel()), max_dist, min_dist, shrink, eps_rot, eps_trans, grid_cell, directions, max_iters, (ctypes.c_int32 * 2)(*reserved))

    out = capi.Align(); ctypes.memset(ctypes.byref(out), 0xAB, ctypes.sizeof(out))
    po = ctypes.byref(out)
    x = (ctypes.c_float * 9)(*range(9)); tri = (ctypes.c_int32 * 3)(0, 1, 2)
    good = params(); pg = ctypes.byref(good)
    assert f(None, None, x, 3, tri, 1, None, po) == ARG and f(None, None, x, 3, tri, 1, pg, None) == ARG and f(None, None, None, 3, tri, 1, pg, po) == ARG
    assert f(None, None, x, -1, None, 0, pg, po) == ARG and f(None, None, x, 3, tri, -1, pg, po) == ARG and f(None, None, x, 3, None, 1, pg, po) == ARG
    for bad_tri in ((0, 1, 3), (-1, 1, 2)):
        assert f(None, None, x, 3, (ctypes.c_int32 * 3)(*bad_tri), 1, pg, po) == ARG
    nan, inf = float("nan"), float("inf")
    scaled = np.eye(4); scaled[:3, :3] *= 1.001
    sheared = np.eye(4); sheared[0, 1] = 1e-4
    bottom = np.eye(4); bottom[3, 0] = 1e-9
    nant = np.eye(4); nant[1, 3] = nan
    for bad in (dict(init=scaled), dict(init=sheared), dict(init=bottom), dict(init=nant), dict(init=np.zeros((4, 4))), dict(max_dist=0.0), dict(max_dist=nan), dict(max_dist=inf), dict(min_dist=0.0),
                dict(min_dist=0.09), dict(min_dist=nan), dict(shrink=0.0), dict(shrink=1.5), dict(shrink=nan), dict(eps_rot=-1.0), dict(eps_rot=nan), dict(eps_rot=inf), dict(eps_trans=-1e-9),
                dict(eps_trans=nan), dict(grid_cell=-1.0), dict(grid_cell=inf), dict(directions=0), dict(directions=4), dict(max_iters=-1), dict(max_iters=65), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        p = params(**bad)
        assert f(None, None, x, 3, tri, 1, ctypes.byref(p), po) == ARG, bad
    for flt in (capi.MeshFilter(0, nan, 0), capi.MeshFilter(0, 0.0, -1)):
        assert f(None, ctypes.byref(flt), x, 3, tri, 1, pg, po) == ARG
    # a rotation that is rigid to 1e-6 passes the argument checks: PSGSDF_ERR_STATE without a context; nothing was touched by any of these
    rot = params(init=aref.rigid(AXIS, 8.0, [0.01, 0.02, 0.03], [0.2, 0.2, 0.2]))
    assert f(None, None, x, 3, tri, 1, ctypes.byref(rot), po) == STATE and f(None, None, x, 3, tri, 1, pg, po) == STATE and f(None, None, None, 0, None, 0, pg, po) == STATE
    assert bytes(out) == b"\xab" * ctypes.sizeof(out)


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_align_without_a_reference_and_on_several_gpus(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    ply = tmp_path / "ref.ply"
    ply.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                   "0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    for extra, words in ((["--compare-align"], ("--compare-align", "--compare-ply")), (["--compare-align", "--compare-ply", str(ply), "--gpus", "2"], ("--compare-align", "--gpus")),
                         (["--compare-ply", str(ply), "--compare-align-iters", "5"], ("--compare-align-iters", "--compare-align")),
                         (["--compare-ply", str(ply), "--compare-align", "--compare-align-iters", "65"], ("--compare-align-iters",)),
                         (["--compare-ply", str(ply), "--compare-align", "--compare-align-iters", "x"], ("--compare-align-iters",))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_align_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("align.hip", tmp_path).items() if "k_aln_" in k}
    print({k: v for k, v in ks.items()})
    assert len(ks) == 4 and all(v["scratch"] == 0 for v in ks.values()), ks      # move, rows<1>, rows<2>, fold
    rows = [v for k, v in ks.items() if "k_aln_rows" in k]
    assert len(rows) == 2 and all(v["vgpr"] <= 128 and v["waves"] >= 4 for v in rows), rows      # 29 double accumulators and the pair function: four waves per SIMD
