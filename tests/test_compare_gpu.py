"""Comparison with a reference on the device (include/psgsdf_compare.h, csrc/compare.hip; DESIGN.md "Comparison with a reference"): the device's
nearest distances, indices, sides, integers and doubles against the exhaustive yardstick tests/_compare_ref.py applied to the context's OWN welded
mesh, bit for bit; against closed form on the analytic plane; and the call's contract (grid and launch size never decide, filter, errors, empty
inputs, ranks, `voxelPS --compare-ply`)."""
import ctypes
import filecmp
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _compare_ref as cref
import _render_ref as rref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi
from test_bake_gpu import scene_engine
from test_mesh_components_cpu import SPHERES, pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config
from test_occlusion_cpu import plane, plane_samples

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
N = 48
INTS = ("n", "n_valid", "n_matched", "n_within_tau", "sum_d", "sum_d2", "sum_signed")
DOUBLES = ("max", "mean", "rms", "mean_signed")
ARRAYS = ("xyz", "normals", "rgb", "faces", "vertex_dist", "vertex_nearest", "vertex_side", "ref_dist", "ref_nearest", "ref_side")


def bits(x):
    return np.asarray(x).tobytes()


def same_result(a, b):
    """two results of the call: every array, integer and double bit for bit"""
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), k
    for s in ("to_reference", "to_reconstruction"):
        for k in INTS:
            assert a[s][k] == b[s][k], (s, k)
        assert np.array_equal(a[s]["hist"], b[s]["hist"]), s
        for k in DOUBLES:
            assert bits(f64(a[s][k])) == bits(f64(b[s][k])), (s, k)
    for k in ("precision", "recall", "fscore"):
        assert bits(f64(a[k])) == bits(f64(b[k])), k


def assert_equals_yardstick(got, exp, tag):
    """the device's dict against _compare_ref.compare's, bit for bit"""
    for side, pre, name in ((exp["vertex"], "vertex_", "to_reference"), (exp["ref"], "ref_", "to_reconstruction")):
        d, n, s = got[pre + "dist"], got[pre + "nearest"], got[pre + "side"]
        assert d.dtype == f32 and n.dtype == np.int32 and s.dtype == np.int8
        differ = int((d.view(np.uint32) != side["dist"].view(np.uint32)).sum())
        print(f"{tag} {name}: {len(d)} queries, {int(side['matched'].sum())} matched, dist differs in {differ}, nearest in {int((n != side['nearest']).sum())}, side in {int((s != side['side']).sum())}")
        assert differ == 0 and np.array_equal(n, side["nearest"]) and np.array_equal(s, side["side"]), (tag, name)
        st = exp[name]
        for k in INTS:
            assert got[name][k] == st[k], (tag, name, k, got[name][k], st[k])
        assert np.array_equal(got[name]["hist"], st["hist"]), (tag, name, got[name]["hist"], st["hist"])
        for k in DOUBLES:
            assert bits(f64(got[name][k])) == bits(f64(st[k])), (tag, name, k, got[name][k], st[k])
    for k in ("precision", "recall", "fscore"):
        assert bits(f64(got[k])) == bits(f64(exp[k])), (tag, k, got[k], exp[k])


@pytest.fixture(scope="module")
def pieces(built):
    v, dim, vs = pieces_volume(torus=True)
    eng = upload(v, dim, vs)
    return eng, eng.extract_mesh_indexed()


def icospheres(vs, lift=0.3):
    """four icospheres of 320 faces around the plain spheres, their radii `lift` voxels larger"""
    parts = [cref.icosphere(np.array(cs) * N * vs, (R + lift) * vs) for cs, R in SPHERES]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] + 162 * k for k, p in enumerate(parts)]).astype(np.int32)


def cloud600(vs):
    """600 Fibonacci points on those four spheres; one exactly on walls of every grid tried (x = 32 vs, y = z = 16 vs: whole multiples of every
    cell edge used below except 3.7 vs, and powers of two times the float32 voxel size, so exact), one far outside the grid's box"""
    pts = np.concatenate([cref.fibonacci(150, np.array(cs) * N * vs, (R + 0.3) * vs) for cs, R in SPHERES])
    pts[7] = f32([32, 16, 16]) * f32(vs)
    pts[11] = f32([200, 200, 200]) * f32(vs)
    return pts


@functools.lru_cache(maxsize=None)
def yardstick(kind):
    """computed once and shared: the exhaustive comparison of the device's own mesh with the icospheres or the cloud (max_dist 8 vs, tau 0.5 vs)"""
    xyz, faces, vs = yardstick.mesh
    ref_xyz, ref_faces = icospheres(vs) if kind == "icospheres" else (cloud600(vs), None)
    return cref.compare(xyz, faces, ref_xyz, ref_faces, vs, 8 * vs, 0.5 * vs)


def test_self_comparison_is_exactly_zero(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    got = eng.compare_reference(xyz, faces)
    V, F = len(xyz), len(faces)
    assert V > 4000 and F > 8000
    for k, want in (("xyz", xyz), ("normals", nrm), ("rgb", rgb), ("faces", faces)):      # the compared mesh: extract_mesh_indexed's, bit for bit
        assert got[k].dtype == want.dtype and bits(got[k]) == bits(want), k
    for pre, name in (("vertex_", "to_reference"), ("ref_", "to_reconstruction")):
        d = got[pre + "dist"]
        assert d.shape == (V,) and bits(d) == bits(np.zeros(V, f32))      # exactly 0.0, and +0.0
        assert (got[pre + "nearest"] >= 0).all() and (got[pre + "nearest"] < F).all() and not got[pre + "side"].any()
        s = got[name]
        assert s["n"] == s["n_valid"] == s["n_matched"] == s["n_within_tau"] == V and s["sum_d"] == s["sum_d2"] == s["sum_signed"] == 0
        assert s["hist"].tolist() == [V] + [0] * 15 and s["max"] == s["mean"] == s["rms"] == s["mean_signed"] == 0.0
        # the nearest face is the smallest-numbered one that holds the vertex
        first = np.full(V, F, np.int64); np.minimum.at(first, faces.ravel(), np.repeat(np.arange(F), 3))
        assert (got[pre + "nearest"] <= first).all() and (got[pre + "nearest"] == first).mean() > 0.99
    assert got["precision"] == got["recall"] == got["fscore"] == 1.0


@pytest.mark.parametrize("kind", ["icospheres", "cloud"])
def test_equals_the_exhaustive_yardstick_bit_for_bit(pieces, kind):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    yardstick.mesh = (xyz, faces, vs)
    exp = yardstick(kind)
    ref_xyz, ref_faces = icospheres(vs) if kind == "icospheres" else (cloud600(vs), None)
    got = eng.compare_reference(ref_xyz, ref_faces, 8 * vs, 0.5 * vs)
    assert_equals_yardstick(got, exp, kind)
    sv, sr = got["to_reference"], got["to_reconstruction"]
    assert 0 < sv["n_matched"] < sv["n"] == len(xyz) and sr["n"] == len(ref_xyz)      # the big piece and the torus are farther than 8 vs from every icosphere
    if kind == "icospheres":
        assert sr["n_matched"] == sr["n"] == 648 and len(ref_faces) == 1280 and (got["ref_side"] == 1).all() and sr["mean_signed"] == sr["mean"] > 0
        assert 0.0 < got["precision"] < 1.0 and got["recall"] > 0.5
    else:
        assert sr["n_matched"] == sr["n"] - 1 and np.isinf(got["ref_dist"][11]) and got["ref_nearest"][11] == -1 and got["ref_nearest"][7] >= 0
        assert not got["vertex_side"].any()      # a cloud has no sides


def test_the_grid_and_the_launch_size_never_decide(pieces, monkeypatch):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    yardstick.mesh = (xyz, faces, vs)
    for kind in ("icospheres", "cloud"):
        ref_xyz, ref_faces = icospheres(vs) if kind == "icospheres" else (cloud600(vs), None)
        base = eng.compare_reference(ref_xyz, ref_faces, 8 * vs, 0.5 * vs)
        assert_equals_yardstick(base, yardstick(kind), kind)
        for cell in (0.5, 1.0, 3.7, 16.0):
            same_result(base, eng.compare_reference(ref_xyz, ref_faces, 8 * vs, 0.5 * vs, grid_cell=cell * vs))
    assert eng.get_tuning()["effective"]["compare_chunk"] == 2 ** 24
    monkeypatch.setenv("PSGSDF_COMPARE_CHUNK", "64")      # (read when a context is created)
    v, dim, _ = pieces_volume(torus=True)
    small = upload(v, dim, vs)
    monkeypatch.delenv("PSGSDF_COMPARE_CHUNK")
    assert small.get_tuning()["effective"]["compare_chunk"] == 64
    for kind in ("icospheres", "cloud"):
        ref_xyz, ref_faces = icospheres(vs) if kind == "icospheres" else (cloud600(vs), None)
        same_result(eng.compare_reference(ref_xyz, ref_faces, 8 * vs, 0.5 * vs), small.compare_reference(ref_xyz, ref_faces, 8 * vs, 0.5 * vs))
    small.close()


@pytest.fixture(scope="module")
def plane_engine(built):
    v, dim, n = plane()
    return upload(v, dim, 0.01), n


def plane_cloud(h, vs):
    q, m = plane_samples()
    return (q.astype(f64) + h * vs * m.astype(f64)).astype(f32)


@pytest.mark.parametrize("h", [0.37, -0.37, 2.5])
def test_plane_distances_and_sides(plane_engine, h):
    eng, n = plane_engine
    vs = vs_of(eng)
    got = eng.compare_reference(plane_cloud(h, vs), None, 8 * vs, 0.5 * vs)
    d = got["ref_dist"].astype(f64)
    err = np.abs(d - abs(h) * vs).max() / vs
    s = got["to_reconstruction"]
    print(f"plane h = {h}: {s['n_matched']} of {s['n']} matched, |dist - |h|| <= {err:.2e} vs, mean_signed {s['mean_signed'] / vs:.6f} vs, sides {np.unique(got['ref_side']).tolist()}")
    assert s["n"] == s["n_valid"] == s["n_matched"] == 300
    assert err <= 1e-4      # the project's bound for this exact-on-a-plane model at |u| <= 48 (test_occlusion_cpu)
    assert (got["ref_side"] == (1 if h > 0 else -1)).all()
    assert np.sign(s["mean_signed"]) == np.sign(h) and abs(abs(s["mean_signed"]) - abs(h) * vs) <= 1e-4 * vs and abs(s["mean"]) == abs(s["mean_signed"])
    assert s["n_within_tau"] == (300 if abs(h) <= 0.5 else 0) and got["recall"] == (1.0 if abs(h) <= 0.5 else 0.0)


def test_the_radius_is_a_cut(plane_engine):
    eng, n = plane_engine
    vs = vs_of(eng)
    pts = plane_cloud(2.5, vs)
    xyz, _, _, faces, _ = eng.extract_mesh_indexed()
    d_all = cref.nearest(pts, xyz, faces, 2 * vs)["d_all"]
    assert (np.abs(d_all - 2 * vs) > 1e-3 * vs).all()      # a condition of the comparison: no point sits on the radius
    got = eng.compare_reference(pts, None, 2 * vs, 0.5 * vs)
    s = got["to_reconstruction"]
    assert np.isinf(got["ref_dist"]).all() and (got["ref_dist"] > 0).all() and (got["ref_nearest"] == -1).all() and not got["ref_side"].any()
    assert s["n"] == s["n_valid"] == 300 and s["n_matched"] == 0 and s["n_within_tau"] == 0 and not s["hist"].any()
    assert s["mean"] == s["rms"] == s["max"] == s["mean_signed"] == 0.0 and s["sum_d"] == s["sum_d2"] == s["sum_signed"] == 0
    assert got["recall"] == 0.0 and got["fscore"] == 0.0
    # ... and with the radius just above, all of them match
    got = eng.compare_reference(pts, None, 3 * vs, 0.5 * vs)
    assert got["to_reconstruction"]["n_matched"] == 300 and got["to_reconstruction"]["hist"][13] == 300      # 16 * 2.5 / 3 = 13.3


def test_invalid_queries_and_empty_inputs(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    pts = cloud600(vs)[:40].copy()
    pts[3, 1] = np.nan; pts[9, 2] = np.inf
    got = eng.compare_reference(pts, None, 8 * vs, 0.5 * vs)
    s = got["to_reconstruction"]
    assert s["n"] == 40 and s["n_valid"] == 38 and np.isnan(got["ref_dist"][[3, 9]]).all() and (got["ref_nearest"][[3, 9]] == -1).all() and np.isfinite(np.delete(got["ref_dist"], [3, 9, 11])).all()
    clean = np.delete(pts, [3, 9], 0)
    ok = eng.compare_reference(clean, None, 8 * vs, 0.5 * vs)
    assert bits(np.delete(got["ref_dist"], [3, 9])) == bits(ok["ref_dist"]) and s["sum_d"] == ok["to_reconstruction"]["sum_d"] and s["n_matched"] == ok["to_reconstruction"]["n_matched"]
    assert got["recall"] == s["n_within_tau"] / 38
    # the cloud given as degenerate faces (i, i, i): the cloud mode's distances, nearest and (zero) sides
    tri = np.repeat(np.arange(len(clean), dtype=np.int32)[:, None], 3, 1)
    deg = eng.compare_reference(clean, tri, 8 * vs, 0.5 * vs)
    for k in ("vertex_dist", "vertex_nearest", "vertex_side", "ref_dist", "ref_nearest", "ref_side"):
        assert bits(deg[k]) == bits(ok[k]), k
    # a face index out of range: PSGSDF_ERR_ARG and *out untouched
    f = eng._fn("compare_reference")
    P = ctypes.c_void_p
    f.argtypes = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, P, P]
    par = capi.CompareParams(8 * vs, 0.5 * vs, 0.0, (ctypes.c_int32 * 2)(0, 0))
    for bad in (len(clean), -1):
        out = capi.Compare(); ctypes.memset(ctypes.byref(out), 0xAB, ctypes.sizeof(out))
        t = tri.copy(); t[5, 2] = bad
        assert f(eng.ctx, None, clean.ctypes.data, len(clean), t.ctypes.data, len(t), ctypes.byref(par), ctypes.byref(out)) == -1
        assert bytes(out) == b"\xab" * ctypes.sizeof(out)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # more than 64 voxels
        eng.compare_reference(clean, None, 65 * vs, vs)
    # no reference: return 0 with every vertex unmatched
    got = eng.compare_reference(np.zeros((0, 3), f32))
    assert len(got["ref_dist"]) == 0 and got["to_reconstruction"]["n"] == 0 and got["recall"] == 0.0 and got["precision"] == 0.0
    assert len(got["vertex_dist"]) == len(xyz) and np.isinf(got["vertex_dist"]).all() and (got["vertex_nearest"] == -1).all() and got["to_reference"]["n_valid"] == len(xyz) and got["to_reference"]["n_matched"] == 0
    # no surface: 0 vertices with every reference point unmatched
    v, dim, _ = pieces_volume(torus=True)
    v = dict(v, weight=np.zeros_like(v["weight"]))
    empty = upload(v, dim, vs)
    got = empty.compare_reference(clean, None, 8 * vs, 0.5 * vs)
    assert len(got["xyz"]) == 0 and len(got["faces"]) == 0 and len(got["vertex_dist"]) == 0 and got["to_reference"]["n"] == 0
    assert np.isinf(got["ref_dist"]).all() and (got["ref_nearest"] == -1).all() and got["to_reconstruction"]["n_valid"] == len(clean) and got["to_reconstruction"]["n_matched"] == 0
    empty.close()


def test_filter_compares_the_kept_mesh(pieces):
    eng, (xyz, nrm, rgb, faces, _) = pieces
    vs = vs_of(eng)
    ref_xyz, ref_faces = icospheres(vs, lift=0.0)      # covers the four small pieces; the largest component is the bumpy sphere
    full = eng.compare_reference(ref_xyz, ref_faces)
    kept = eng.compare_reference(ref_xyz, ref_faces, keep_largest=1)
    comp = eng.extract_mesh_components(keep_largest=1)
    for k in ("xyz", "normals", "rgb", "faces"):
        assert kept[k].dtype == comp[k].dtype and bits(kept[k]) == bits(comp[k]), k
    assert 0 < len(kept["xyz"]) < len(xyz) and len(kept["vertex_dist"]) == len(kept["xyz"])
    print(f"filter: recall {full['recall']:.4f} unfiltered, {kept['recall']:.4f} with keep_largest=1; precision {full['precision']:.4f} / {kept['precision']:.4f}")
    assert kept["recall"] < full["recall"] and full["recall"] > 0.9
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # a filter psgsdf_extract_mesh_components refuses
        eng.compare_reference(ref_xyz, ref_faces, keep_largest=-1)


def test_leaves_everything_else_alone(pieces):
    eng, mesh0 = pieces
    vs = vs_of(eng)
    ref_xyz, ref_faces = icospheres(vs)
    same_result(eng.compare_reference(ref_xyz, ref_faces), eng.compare_reference(ref_xyz, ref_faces))
    for x, y in zip(mesh0, eng.extract_mesh_indexed()):
        assert bits(x) == bits(y)
    ends = []
    for compare in (False, True):
        e, sc = scene_engine("SH1")
        if compare:
            xyz, _, _, faces, _ = e.extract_mesh_indexed()
            got = e.compare_reference(xyz, faces)
            assert got["to_reference"]["n_matched"] == len(xyz) > 1000 and got["fscore"] == 1.0
        e.iterate(capi.ALL, 1)
        v = e.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], e.download_poses(), e.download_light()))
        e.close()
    for x, y in zip(*ends):
        assert bits(x) == bits(y)


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "compare")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 3
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e and "compare_reference" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_compare_ply(built, tmp_path):
    from test_compare_cpu import read_compare_ply
    from test_mesh_indexed_cpu import read_ply_indexed
    plain = str(tmp_path / "plain") + "/"; os.makedirs(plain)
    r = subprocess.run([EXE, "--config_file", voxelps_config(plain, **{"max iter": 4}), "--indexed-mesh"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    skip = ("config.json", "saved_config.json")
    before = sorted(f for f in os.listdir(plain) if f not in skip)
    meshes = [f[:-len("_mesh_indexed.ply")] for f in before if f.endswith("_mesh_indexed.ply")]
    assert "init" in meshes and "after_iter_3" in meshes and not any("compare" in f for f in before)
    last = "after_iter_3"
    ref = plain + last + "_mesh_indexed.ply"
    out = str(tmp_path / "cmp") + "/"; os.makedirs(out)
    r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4}), "--indexed-mesh", "--compare-ply", ref], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(f for f in os.listdir(out) if f not in skip) == sorted(before + [m + s for m in meshes for s in ("_compare.txt", "_mesh_compare.ply")])      # the only new files
    for f in before:      # the flag changes no other file
        assert filecmp.cmp(plain + f, out + f, shallow=False), f
    _, verts, faces = read_ply_indexed(ref)
    largest = max(float(np.abs(verts[a]).max()) for a in "xyz")
    bound = 3 * 2.0 ** -24 * largest      # the writer's float offset and its inverse, one rounding each, plus the subtraction
    rec = {}
    for ln in open(out + last + "_compare.txt").read().splitlines():
        w = ln.split()
        if w[0] in ("to_reference", "to_reconstruction"):
            rec.setdefault(w[0], {}).update({"hist": [int(x) for x in w[2:]]} if w[1] == "hist" else dict(zip(w[1::2], (float(x) for x in w[2::2]))))
        elif w[0] == "precision":
            rec.update(dict(zip(w[0::2], (float(x) for x in w[1::2]))))
    print(f"voxelPS --compare-ply on its own {last}: precision {rec['precision']}, recall {rec['recall']}, max {rec['to_reference']['max']:.3e} / {rec['to_reconstruction']['max']:.3e} m (bound {bound:.3e})")
    assert rec["precision"] == rec["recall"] == rec["fscore"] == 1.0
    for s in ("to_reference", "to_reconstruction"):
        assert rec[s]["n"] == rec[s]["n_matched"] == len(verts) and rec[s]["max"] <= bound and sum(rec[s]["hist"]) == len(verts)
    head, v, f = read_compare_ply(out + last + "_mesh_compare.ply")
    assert np.array_equal(f, faces) and bits(v["xyz"]) == bits(np.stack([verts[a] for a in "xyz"], 1)) and (v["distance"] <= bound).all() and any(h.startswith("comment compare precision 1 recall 1") for h in head)
    # another dump of the same run is a different surface: its distances to that reference are not all zero
    w = next(ln for ln in open(out + "init_compare.txt").read().splitlines() if ln.startswith("to_reference mean_voxels")).split()
    assert float(w[w.index("rms") + 1]) > 0.0
