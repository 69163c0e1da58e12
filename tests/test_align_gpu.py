"""Alignment of a reference on the device (include/psgsdf_align.h, csrc/align.hip; DESIGN.md "Alignment of a reference"): the evaluation at the
initial transform against the yardstick tests/_align_ref.py on the context's OWN welded mesh (pairs exactly, moved points bit for bit, the sums to
the bound of two summation orders), the loop on the mesh's own moved copy and on the analytic spheres' cloud, and the call's contract (same bytes
whatever the grid and the launch size, shrink, degenerate and too-few inputs, non-finite points, errors, filter, ranks, `voxelPS --compare-align`)."""
import ctypes
import filecmp
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _align_ref as aref
import _compare_ref as cref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi
from test_align_cpu import AXIS, displacement, motion, sphere_cloud
from test_bake_gpu import scene_engine
from test_compare_gpu import cloud600, icospheres, pieces, plane_cloud, plane_engine      # noqa: F401 (fixtures)
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def bits(x):
    return np.asarray(x).tobytes()


def iter_bits(it):
    return bits(f64([it["radius"], it["rms"], it["min_pivot"]])) + bits(np.int64(it["n_pairs"])) + bits(it["step"])


def same_result(a, b):
    """two results of the call, byte for byte"""
    assert a["status"] == b["status"] and a["n_iters"] == b["n_iters"] and len(a["iters"]) == len(b["iters"])
    for k in ("transform", "centre", "system0", "aligned_xyz", "xyz", "normals", "rgb", "faces"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), k
    for x, y in zip(a["iters"] + [a["final"]], b["iters"] + [b["final"]]):
        assert iter_bits(x) == iter_bits(y)


def reference(kind, vs):
    return icospheres(vs) if kind == "icospheres" else (cloud600(vs), None)


@functools.lru_cache(maxsize=None)
def yardstick0(kind, directions, with_init):
    """computed once and shared: the exhaustive evaluation at the initial transform of the moved icospheres or cloud against the device's own mesh"""
    xyz, nrm, faces, vs = yardstick0.mesh
    M = motion(xyz, vs, 3.0, 1.5)
    pts, ref_faces = reference(kind, vs)
    ref = aref.move(M[:3], pts)
    init = aref.rigid((0.5, 0.1, -0.7), 1.0, [0.3 * vs, -0.2 * vs, 0.4 * vs], xyz.astype(f64).mean(0)) if with_init else None
    return ref, ref_faces, init, aref.align(xyz, nrm, faces, ref, ref_faces, vs, init=init, directions=directions, max_iters=0)


@pytest.mark.parametrize("kind,directions,with_init", [("icospheres", 1, False), ("icospheres", 2, False), ("cloud", 1, False), ("cloud", 2, False), ("cloud", 3, True)])
def test_iteration_zero_equals_the_yardstick(pieces, kind, directions, with_init):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    yardstick0.mesh = (xyz, nrm, faces, vs)
    ref, ref_faces, init, exp = yardstick0(kind, directions, with_init)
    got = eng.align_reference(ref, ref_faces, init=init, directions=directions, max_iters=0)
    n = exp["n0"]
    assert got["status"] == exp["status"] == aref.MAX_ITERS and got["n_iters"] == 0 and got["iters"] == []
    assert got["final"]["n_pairs"] == exp["final"]["n_pairs"] and sum(got["final"]["n_pairs"]) == n > 500
    assert got["aligned_xyz"].dtype == f32 and bits(got["aligned_xyz"]) == bits(exp["aligned_xyz"])
    assert bits(got["centre"]) == bits(exp["centre"]) and bits(got["transform"]) == bits(exp["transform"])
    bound = (n - 1) * 2.0 ** -52 * exp["system0_abs"]      # two summation orders of the same n terms
    err = np.abs(got["system0"] - exp["system0"])
    print(f"{kind} directions {directions}{' with init' if with_init else ''}: pairs {got['final']['n_pairs']}, |system0 - yardstick| / bound <= {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"rms {got['final']['rms'] / vs:.4f} vs")
    assert (err <= bound).all(), (err, bound)
    assert abs(got["final"]["rms"] - exp["final"]["rms"]) <= 1e-12 * vs and got["final"]["radius"] == 8 * vs
    assert bits(got["xyz"]) == bits(xyz) and bits(got["normals"]) == bits(nrm) and bits(got["faces"]) == bits(faces)


@pytest.mark.parametrize("directions", [1, 2, 3])
def test_own_mesh_moved_is_brought_back(pieces, directions):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    M = motion(xyz, vs, 3.0, 1.5)
    ref = aref.move(aref.rigid_inverse(M)[:3], xyz)
    got = eng.align_reference(ref, faces, directions=directions)
    d = displacement(xyz, vs, got["transform"], M)
    after = eng.compare_reference(got["aligned_xyz"], faces, 8 * vs, 0.01 * vs)
    before = eng.compare_reference(ref, faces, 8 * vs, 0.01 * vs)
    print(f"own mesh, directions {directions}: status {got['status']} after {got['n_iters']} steps, rms {['%.3g' % (it['rms'] / vs) for it in got['iters']]} -> {got['final']['rms'] / vs:.3g} vs, "
          f"displacement {d:.2e} vs; compare rms {after['to_reference']['rms'] / vs:.2e} / {after['to_reconstruction']['rms'] / vs:.2e} vs (unaligned {before['to_reference']['rms'] / vs:.3f})")
    assert got["status"] == capi.ALIGN_CONVERGED and got["n_iters"] <= 10
    assert d <= 1e-3
    for s in ("to_reference", "to_reconstruction"):
        assert after[s]["rms"] <= 1e-3 * vs and before[s]["rms"] > 0.1 * vs
    assert after["precision"] == after["recall"] == 1.0


@pytest.mark.parametrize("directions", [1, 3])
def test_sphere_cloud_moved_eight_degrees(pieces, directions):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    M = motion(xyz, vs, 8.0, 3.0)
    ref = aref.move(aref.rigid_inverse(M)[:3], sphere_cloud(vs))
    exp = aref.align(xyz, nrm, faces, ref, None, vs, directions=directions, search=aref.pruned_nearest)
    d_exp = displacement(xyz, vs, exp["transform"], M)
    got = eng.align_reference(ref, None, directions=directions)
    d = displacement(xyz, vs, got["transform"], M)
    print(f"sphere cloud 8 deg / 3 vs, directions {directions}: device status {got['status']} after {got['n_iters']} steps, displacement {d:.4f} vs; yardstick {exp['status']} after {exp['n_iters']}, {d_exp:.4f} vs")
    assert got["status"] == capi.ALIGN_CONVERGED and exp["status"] == aref.CONVERGED
    assert d <= 2 * d_exp + 2 * 1e-3
    assert min(it["min_pivot"] for it in got["iters"]) >= 100 * aref.PIVOT_MIN


def test_same_bytes_whatever_the_grid_and_the_launch_size(pieces, monkeypatch):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    M = motion(xyz, vs, 3.0, 1.5)
    cases = [(aref.move(aref.rigid_inverse(M)[:3], cloud600(vs)), None), (aref.move(aref.rigid_inverse(M)[:3], icospheres(vs)[0]), icospheres(vs)[1])]
    base = [eng.align_reference(r, f, max_iters=6) for r, f in cases]
    for (r, f), b in zip(cases, base):
        assert b["n_iters"] >= 3
        same_result(b, eng.align_reference(r, f, max_iters=6))
        for cell in (0.5, 3.7, 16.0):
            same_result(b, eng.align_reference(r, f, max_iters=6, grid_cell=cell * vs))
    monkeypatch.setenv("PSGSDF_COMPARE_CHUNK", "64")      # (read when a context is created)
    v, dim, _ = pieces_volume(torus=True)
    small = upload(v, dim, vs)
    monkeypatch.delenv("PSGSDF_COMPARE_CHUNK")
    assert small.get_tuning()["effective"]["compare_chunk"] == 64
    for (r, f), b in zip(cases, base):
        same_result(b, small.align_reference(r, f, max_iters=6))
    t = small.get_tuning()["last_align"]
    assert t["iterations"] == base[1]["n_iters"] and t["evaluations"] == t["iterations"] + 1 and t["queries"] == [t["evaluations"] * 648, t["evaluations"] * len(xyz)] and min(t["pairs"]) > 0
    small.close()


def test_shrink(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    M = motion(xyz, vs, 3.0, 1.5)
    ref = aref.move(aref.rigid_inverse(M)[:3], cloud600(vs))
    same_result(eng.align_reference(ref), eng.align_reference(ref, shrink=1.0, max_dist=8 * vs, min_dist=vs, eps_trans=1e-3 * vs))
    got = eng.align_reference(ref, shrink=0.5, min_dist=vs, eps_rot=0.0, eps_trans=0.0, max_iters=6)
    assert got["status"] == capi.ALIGN_MAX_ITERS and got["n_iters"] == 6
    assert [it["radius"] for it in got["iters"]] == [max(vs, 8 * vs * 0.5 ** k) for k in range(6)] and got["final"]["radius"] == vs
    assert got["iters"][0]["n_pairs"][1] >= got["iters"][5]["n_pairs"][1] > 0      # no more vertices find a partner within the smaller radius


def test_plane_is_degenerate_and_three_points_are_too_few(plane_engine, pieces):
    eng, n = plane_engine
    vs = vs_of(eng)
    init = aref.rigid((0, 0, 1), 0.0, [0, 0, 0], [0, 0, 0])
    got = eng.align_reference(plane_cloud(0.37, vs), None, init=init)
    print(f"plane: status {got['status']}, pairs {got['final']['n_pairs']}, pivot {got['iters'][0]['min_pivot']:.3e}")
    assert got["status"] == capi.ALIGN_DEGENERATE and got["n_iters"] == 0 and bits(got["transform"]) == bits(init)
    assert len(got["iters"]) == 1 and got["iters"][0]["min_pivot"] <= aref.PIVOT_MIN / 100 and not got["iters"][0]["step"].any()
    assert got["final"]["n_pairs"][0] == 300 and abs(got["final"]["rms"] / vs - 0.37) <= 1e-3
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    pts = cloud600(vs)[:3]
    got = eng.align_reference(pts, None, directions=1)
    assert got["status"] == capi.ALIGN_TOO_FEW and got["n_iters"] == 0 and bits(got["transform"]) == bits(np.eye(4)) and got["final"]["n_pairs"] == [3, 0]
    assert bits(got["aligned_xyz"]) == bits(pts)


def test_non_finite_points_are_skipped(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    M = motion(xyz, vs, 3.0, 1.5)
    clean = aref.move(aref.rigid_inverse(M)[:3], sphere_cloud(vs))
    dirty = np.insert(clean, [3, 9], f32([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1]]), 0)
    a, b = eng.align_reference(clean, None, directions=1), eng.align_reference(dirty, None, directions=1)
    assert b["status"] == a["status"] == capi.ALIGN_CONVERGED
    assert not np.isfinite(b["aligned_xyz"][[3, 10]]).all(1).any() and np.isfinite(np.delete(b["aligned_xyz"], [3, 10], 0)).all()
    assert a["iters"][0]["n_pairs"] == b["iters"][0]["n_pairs"] and b["final"]["n_pairs"] == a["final"]["n_pairs"] == [600, 0]
    # the same rows of iteration 0 in another order of summation (the lanes shift by two queries): the same sums to the bound of two orders
    assert np.abs(a["system0"] - b["system0"]).max() <= 600 * 2.0 ** -52 * max(1.0, np.abs(a["system0"]).max())


def test_errors_leave_out_untouched_and_empty_inputs_are_too_few(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    f = eng._fn("align_reference")
    P = ctypes.c_void_p
    f.argtypes = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, P, P]
    pts = np.ascontiguousarray(cloud600(vs)[:40])
    tri = np.repeat(np.arange(len(pts), dtype=np.int32)[:, None], 3, 1)

    def params(init=None, max_dist=8 * vs, min_dist=vs, shrink=1.0, directions=3, max_iters=30):
        T = np.eye(4) if init is None else np.asarray(init, f64)
        return capi.AlignParams((ctypes.c_double * 16)(*T.ravel()), max_dist, min_dist, shrink, 1e-5, 1e-3 * vs, 0.0, directions, max_iters, (ctypes.c_int32 * 2)(0, 0))

    scaled = np.eye(4); scaled[:3, :3] *= 1.01
    bad_tri = tri.copy(); bad_tri[5, 2] = len(pts)
    flt = capi.MeshFilter(0, 0.0, -1)
    for p, t, fl in ((params(init=scaled), tri, None), (params(max_dist=65 * vs), tri, None), (params(min_dist=9 * vs), tri, None), (params(shrink=0.0), tri, None), (params(directions=0), tri, None),
                     (params(max_iters=65), tri, None), (params(), bad_tri, None), (params(), tri, flt)):
        out = capi.Align(); ctypes.memset(ctypes.byref(out), 0xAB, ctypes.sizeof(out))
        assert f(eng.ctx, ctypes.byref(fl) if fl is not None else None, pts.ctypes.data, len(pts), t.ctypes.data, len(t), ctypes.byref(p), ctypes.byref(out)) == -1
        assert bytes(out) == b"\xab" * ctypes.sizeof(out)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.align_reference(pts, None, keep_largest=-1)
    # no reference
    init = aref.rigid(AXIS, 2.0, [vs, 0, 0], [0.2, 0.2, 0.2])
    got = eng.align_reference(np.zeros((0, 3), f32), init=init)
    assert got["status"] == capi.ALIGN_TOO_FEW and got["n_iters"] == 0 and bits(got["transform"]) == bits(init) and len(got["aligned_xyz"]) == 0 and len(got["xyz"]) == len(xyz)
    # no surface
    v, dim, _ = pieces_volume(torus=True)
    empty = upload(dict(v, weight=np.zeros_like(v["weight"])), dim, vs)
    got = empty.align_reference(pts, None, init=init)
    assert got["status"] == capi.ALIGN_TOO_FEW and bits(got["transform"]) == bits(init) and len(got["xyz"]) == 0 and got["final"]["n_pairs"] == [0, 0] and not got["centre"].any()
    assert bits(got["aligned_xyz"]) == bits(aref.move(init[:3], pts))
    empty.close()


def test_filter_aligns_the_kept_mesh(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    comp = eng.extract_mesh_components(keep_largest=1)
    M = motion(xyz, vs, 3.0, 1.5)
    ref = aref.move(aref.rigid_inverse(M)[:3], comp["xyz"])
    kept = eng.align_reference(ref, comp["faces"], keep_largest=1)
    for k in ("xyz", "normals", "rgb", "faces"):
        assert kept[k].dtype == comp[k].dtype and bits(kept[k]) == bits(comp[k]), k
    assert 0 < len(kept["xyz"]) < len(xyz) and kept["final"]["n_pairs"][1] == len(comp["xyz"]) >= kept["final"]["n_pairs"][0] > 0.99 * len(comp["xyz"])
    assert kept["status"] == capi.ALIGN_CONVERGED and displacement(comp["xyz"], vs, kept["transform"], M) <= 1e-3
    full = eng.align_reference(ref, comp["faces"], directions=1)
    assert full["final"]["n_pairs"][0] == kept["final"]["n_pairs"][0] and len(full["xyz"]) == len(xyz)


def test_leaves_everything_else_alone(pieces):
    eng, mesh0 = pieces
    vs = vs_of(eng)
    ref_xyz, ref_faces = icospheres(vs)
    before = eng.compare_reference(ref_xyz, ref_faces)
    eng.align_reference(ref_xyz, ref_faces, max_iters=3)
    after = eng.compare_reference(ref_xyz, ref_faces)
    from test_compare_gpu import same_result as same_compare
    same_compare(before, after)
    for x, y in zip(mesh0, eng.extract_mesh_indexed()):
        assert bits(x) == bits(y)
    ends = []
    for align in (False, True):
        e, sc = scene_engine("SH1")
        if align:
            xyz, _, _, faces, _ = e.extract_mesh_indexed()
            got = e.align_reference(xyz, faces, max_iters=2)
            assert sum(got["final"]["n_pairs"]) > 1.9 * len(xyz) and len(xyz) > 1000 and got["final"]["rms"] == 0.0
        e.iterate(capi.ALL, 1)
        v = e.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], e.download_poses(), e.download_light()))
        e.close()
    for x, y in zip(*ends):
        assert bits(x) == bits(y)


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "align")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 3
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e and "align_reference" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def write_ply(path, xyz, faces):
    rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))])); rec["n"] = 3; rec["v"] = faces
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n").encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes()); f.write(rec.tobytes())


def test_voxelps_compare_align(built, tmp_path):
    from test_mesh_indexed_cpu import read_ply_indexed
    vs = float(f32(0.004))
    plain = str(tmp_path / "plain") + "/"; os.makedirs(plain)
    r = subprocess.run([EXE, "--config_file", voxelps_config(plain, **{"max iter": 4}), "--indexed-mesh"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    skip = ("config.json", "saved_config.json")
    before = sorted(f for f in os.listdir(plain) if f not in skip)
    last = "after_iter_3"
    _, verts, faces = read_ply_indexed(plain + last + "_mesh_indexed.ply")
    xyz = np.stack([verts[a] for a in "xyz"], 1)
    M = motion(xyz, vs, 2.0, 1.0)
    ref = str(tmp_path / "moved.ply")
    write_ply(ref, aref.move(aref.rigid_inverse(M)[:3], xyz), faces)
    rms = {}
    for tag, flags in (("aligned", ["--compare-align"]), ("unaligned", [])):
        out = str(tmp_path / tag) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4}), "--indexed-mesh", "--compare-ply", ref] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files = sorted(f for f in os.listdir(out) if f not in skip)
        assert ([f for f in files if f.endswith("_align.txt")] != []) == bool(flags) and last + "_compare.txt" in files
        for f in before:      # every file of the plain run is byte-identical
            assert filecmp.cmp(plain + f, out + f, shallow=False), (tag, f)
        for ln in open(out + last + "_compare.txt").read().splitlines():
            w = ln.split()
            if w[0] in ("to_reference", "to_reconstruction") and w[1] == "mean_voxels":
                rms[tag, w[0]] = float(w[w.index("rms_voxels") + 1])
        if flags:
            txt = open(out + last + "_align.txt").read().splitlines()
            assert txt[0].split()[:2] == ["status", "converged"], txt[0]
            assert len([ln for ln in txt if ln.startswith("iter ")]) == int(txt[0].split()[3]) <= 10
            T = np.array([[float(x) for x in ln.split()] for ln in txt[txt.index("transform") + 1:txt.index("transform") + 5]])
            bound = 1e-3 * vs + 3 * 2.0 ** -24 * float(np.abs(xyz).max())      # eps_trans and the PLY's float32 coordinates
            d = displacement(xyz, vs, T, M) * vs
            print(f"voxelPS --compare-align on its own {last} moved 2 deg / 1 vs: {txt[0]}, displacement {d:.3e} m (bound {bound:.3e})")
            assert np.array_equal(T[3], [0, 0, 0, 1]) and d <= bound
    print(f"rms in voxels: {rms}")
    for s in ("to_reference", "to_reconstruction"):
        assert rms["aligned", s] < 1e-3 and rms["unaligned", s] > 0.1
