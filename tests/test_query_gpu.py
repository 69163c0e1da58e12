"""Field queries on the device (include/psgsdf_query.h, csrc/query.hip; DESIGN.md 22 "Field queries").  Points and projections against the yardstick
tests/_query_ref.py bit for bit -- the arithmetic is double without contraction and per query, so nothing is left to a tolerance -- and against the
closed forms of test_query_cpu directly, so that a wrong yardstick cannot hide behind agreement.  Rays against the yardstick within the project's cap
for this walk (test_bake_gpu.VOXEL_SHARE: the device walks in float32, the yardstick in float64), xyz, normal and rgb recomputed from the device's
own t and voxel bit for bit, and against closed form.  Then independence of the queries, launches in chunks, isolation, errors, ranks, voxelPS."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _query_ref as qref
from _ranks import run_spec
from psgradientsdf_amd import capi, synth
from test_bake_gpu import VOXEL_SHARE, same_bits
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config
from test_occlusion_cpu import VS, VS32, corner_samples, corner_volume, plane
from test_query_cpu import (BOUND, RAY_CASES, TOL, check_corner_rays, check_mixed, check_plane, check_sphere_points, check_sphere_projection, check_sphere_rays, corner_rays,
                            mixed_points, plane_points, sphere_points, sphere_ray_analytic, sphere_rays, sphere_volume)

pytestmark = pytest.mark.gpu
f32 = np.float32
MODELS = ("cell", "trilinear")
ULPS = 64 * 64 * 2.0 ** -24      # voxels: 64 float32 ulps at 64 voxels (about ten float32 operations on values below 64 voxels, amplified by at most 4)


def same_result(a, b):
    """two results of a query call: every array bit for bit, the counts equal"""
    keys = [k for k in a if k != "counts" and not k.startswith("t_walk")]
    assert sorted(keys) == sorted(k for k in b if k != "counts" and not k.startswith("t_walk"))
    same_bits(a, b, keys)
    assert a["counts"] == b["counts"]


def state(eng):
    return eng.download_volume(), [int(x) for x in eng.info().dim], vs_of(eng)


@pytest.fixture(scope="module")
def sphere(built):
    v, dim = sphere_volume()
    return upload(v, dim, VS)


@pytest.fixture(scope="module")
def corner(built):
    v, dim = corner_volume()
    return upload(v, dim, VS)


@pytest.fixture(scope="module")
def pieces(built):
    v, dim, vs = pieces_volume(torus=True)
    return upload(v, dim, vs)


@pytest.fixture(scope="module")
def pieces_vertices(pieces):
    xyz = pieces.extract_mesh_indexed()[0]
    rng = np.random.default_rng(13)
    return xyz, (xyz.astype(np.float64) + rng.uniform(-1.5, 1.5, size=xyz.shape) * vs_of(pieces)).astype(f32)


def assert_bit_for_bit(eng, pts, tag):
    v, dim, vs = state(eng)
    for model in MODELS:
        same_result(eng.query_points(pts, model), qref.query_points(v, dim, vs, pts, model))
        for tol, iters in ((TOL * vs, 16), (0.0, 3)):
            got, exp = eng.project_points(pts, model, tol, iters), qref.project_points(v, dim, vs, pts, model, tol, iters)
            same_result(got, exp)
            print(f"{tag}, model {model}, tol {tol:.1e}, max_iters {iters}: {len(pts)} points bit for bit, {got['counts']}")


def test_sphere_points_and_projections_equal_the_yardstick_bit_for_bit(sphere):
    assert_bit_for_bit(sphere, sphere_points()[0], "sphere")


def test_every_status_equals_the_yardstick_bit_for_bit(corner):
    pts, _ = mixed_points()
    assert_bit_for_bit(corner, pts, "mixed statuses")
    for model in MODELS:
        check_mixed(corner.query_points(pts, model), model)


def test_mesh_vertices_equal_the_yardstick_bit_for_bit(pieces, pieces_vertices):
    xyz, jittered = pieces_vertices
    assert_bit_for_bit(pieces, xyz, "welded mesh")
    assert_bit_for_bit(pieces, jittered, "welded mesh jittered by 1.5 voxels")


@pytest.mark.parametrize("model", MODELS)
def test_closed_forms_on_the_device(sphere, pieces, pieces_vertices, model):
    q, off = sphere_points()
    got = sphere.query_points(q, model)
    check_sphere_points(got, model, "device")
    pr = sphere.project_points(q, model, TOL * vs_of(sphere), 16)
    conv = check_sphere_projection(pr, model, "device")
    started = got["status"] == qref.OK
    if model == "trilinear":
        assert np.array_equal(conv, started) and pr["iterations"][conv].max() <= 4
        far = conv & (np.abs(off) > BOUND)
        assert np.array_equal(np.sign(pr["distance"][far]), np.sign(off[far]))
    v, dim, _ = plane()
    check_plane(upload(v, dim, VS).query_points(plane_points()[0], model), model, "device")
    xyz = pieces_vertices[0]
    m = pieces.query_points(xyz, model)
    worst = np.abs(m["dist"]).max() / vs_of(pieces)
    print(f"device welded mesh, model {model}: {m['counts']['n_ok']} of {len(xyz)} vertices valid, max |phi| {worst:.2e} voxel")
    assert len(xyz) == 4280 and (m["status"] == qref.OK).all()
    if model == "trilinear":
        assert worst <= 1e-5


def assert_rays_match(eng, o, w, t_min, t_max, closed_t, tag):
    """the device's rays against the yardstick's; closed_t: the analytic parameters (mesh units) the yardstick's own deviation is taken from"""
    v, dim, vs = state(eng)
    got = eng.cast_rays(o, w, t_min, t_max)
    exp = qref.cast_rays(v, dim, vs, o, w, t_min, np.inf if t_max is None else t_max)
    differ = (got["status"] != exp["status"]) | (got["voxel"] != exp["voxel"])
    share = differ.sum() / len(o)
    both = ~differ & (got["voxel"] >= 0)
    wn = w.astype(np.float64); wn /= np.linalg.norm(wn, axis=1)[:, None]
    # the closed form is that of a clean hit (status 0): a buried ray's t is t_min on both sides, exactly
    steep = both & (got["status"] == qref.HIT) & (np.abs((got["normal"].astype(np.float64) * wn).sum(1)) >= 0.25)
    assert steep.any() and np.isfinite(closed_t[steep]).all()
    ref_dev = np.abs(exp["t"].astype(np.float64) - closed_t)[steep].max() / vs
    err = np.abs(got["t"].astype(np.float64) - exp["t"].astype(np.float64))[steep].max() / vs
    buried = both & (got["status"] == qref.BURIED)
    print(f"{tag}: {len(o)} rays, {got['counts']}, {int(differ.sum())} differ in status or voxel ({share:.2e}, cap {VOXEL_SHARE}); {int(steep.sum())} agreed clean hits with |m.w| >= 0.25: "
          f"|t_dev - t_ref| up to {err:.2e} voxel (bound {ref_dev:.2e} + {ULPS:.1e}); {int(buried.sum())} agreed buried rays")
    assert share <= VOXEL_SHARE
    assert err <= ref_dev + ULPS
    assert np.array_equal(got["t"][buried], exp["t"][buried]) and (got["t"][buried] == f32(t_min)).all()
    # normal and rgb follow from the voxel alone, xyz from the walk's float32 t and the UNSHIFTED origin: xyz = (float)(o + ((double) t + t_min) w)
    hit = got["voxel"] >= 0
    xyz, nrm, col = qref.ray_outputs(v, vs, o, w, 0.0, got["t"], got["voxel"])      # (from the call's own float32 T)
    same_bits(dict(normal=nrm, rgb=col), got, ("normal", "rgb"))
    if t_min == 0.0:      # T is then the walk's own float32 t: xyz follows from it exactly
        same_bits(dict(xyz=xyz), got, ("xyz",))
    else:
        # the call's t is (float) T: T lies within half a float32 ulp of it, which moves o + T w by at most |w[a]| ulp(t) / 2 (|w| = 1), and the
        # two roundings to float32 can then differ by one ulp of the coordinate
        tol = 0.5 * np.spacing(got["t"]).astype(np.float64)[:, None] * np.abs(wn) + np.spacing(np.abs(xyz)).astype(np.float64)
        off = np.abs(got["xyz"].astype(np.float64) - xyz.astype(np.float64))
        print(f"{tag}: xyz against o + t w from the call's own t: worst {float((off / tol)[hit].max()):.2f} of its rounding bound; t_min w alone would be {t_min / vs:.2f} voxel")
        assert (off <= tol)[hit].all()
        # a buried ray's walk parameter is 0 on both sides: its point is (float)(o + t_min w), the same bits
        assert np.array_equal(got["xyz"][buried], exp["xyz"][buried])
    miss = ~hit
    assert not got["t"][miss].any() and not got["xyz"][miss].any() and not got["normal"][miss].any() and not got["rgb"][miss].any()
    assert np.array_equal(miss, (got["status"] == qref.MISS) | (got["status"] == qref.RAY_INVALID))
    cn = got["counts"]
    assert cn == dict(n=len(o), n_valid=int((got["status"] != qref.RAY_INVALID).sum()), n_hits=int((~miss).sum()), n_buried=int((got["status"] == qref.BURIED).sum()))
    return got


def test_sphere_rays(sphere):
    o, w = sphere_rays()
    _, t, _ = sphere_ray_analytic(o, w)
    got = assert_rays_match(sphere, o, w, 0.0, None, t, "sphere")
    check_sphere_rays(got, "device")


def test_corner_rays_and_their_ends(corner):
    o, w, t = corner_rays()
    for t_min, t_max in RAY_CASES:
        assert_rays_match(corner, o, w, t_min * VS32, t_max * VS32, t, f"corner ({t_min}, {t_max}]")
    check_corner_rays(lambda o, w, a, b: corner.cast_rays(o, w, a, None if np.isinf(b) else b), "device")
    # invalid rays take no part
    o, w = o[:70].copy(), w[:70].copy()
    o[3, 1] = np.nan; w[10] = 0; w[33, 2] = np.inf; o[64, 0] = -np.inf
    got = corner.cast_rays(o, w)
    bad = np.zeros(70, bool); bad[[3, 10, 33, 64]] = True
    assert np.array_equal(got["status"] == qref.RAY_INVALID, bad) and got["counts"]["n_valid"] == 66 and (got["voxel"][bad] == -1).all()
    v, dim, vs = state(corner)
    exp = qref.cast_rays(v, dim, vs, o, w)
    assert np.array_equal(got["status"], exp["status"]) and np.array_equal(got["voxel"], exp["voxel"])


def three_calls(eng, pts, o, w):
    vs = vs_of(eng)
    return [eng.query_points(pts, "cell"), eng.query_points(pts, "trilinear"), eng.project_points(pts, "cell"), eng.project_points(pts, "trilinear", 0.0, 5),
            eng.cast_rays(o, w), eng.cast_rays(o, w, 0.5 * vs, 9 * vs)]


def subset(r, idx):
    return {k: (x[idx] if k != "counts" else None) for k, x in r.items()}


def test_queries_are_independent_and_launches_change_no_bit(sphere, monkeypatch):
    q = sphere_points()[0][:1000].copy()
    q[17, 0] = np.nan; q[500] = [-1.0, 0.1, 0.1]
    o, w = sphere_rays()
    o, w = o[:1000].copy(), w[:1000].copy()
    w[5] = 0
    whole = three_calls(sphere, q, o, w)
    idx = np.r_[3:40, 490:520:3, 999]
    for a, b in zip(three_calls(sphere, q[idx], o[idx], w[idx]), whole):      # a subset of a call equals the same queries inside the whole call
        a, b = subset(a, slice(None)), subset(b, idx)
        same_bits(a, b, [k for k in a if k != "counts"])
    for n in (1, 63, 64, 65):
        for a, b in zip(three_calls(sphere, q[:n], o[:n], w[:n]), whole):
            assert a["counts"]["n"] == n
            same_bits(subset(a, slice(None)), subset(b, slice(0, n)), [k for k in a if k != "counts"])
    assert sphere.get_tuning()["effective"]["query_chunk"] == 2 ** 30
    monkeypatch.setenv("PSGSDF_QUERY_CHUNK", "128")      # (read when a context is created)
    v, dim = sphere_volume()
    small = upload(v, dim, VS)
    monkeypatch.setenv("PSGSDF_QUERY_CHUNK", "100")      # not a multiple of 64: refused
    with pytest.raises(capi.PsgsdfError):
        upload(v, dim, VS)
    monkeypatch.delenv("PSGSDF_QUERY_CHUNK")
    assert small.get_tuning()["effective"]["query_chunk"] == 128 and small.get_tuning()["env"]["PSGSDF_QUERY_CHUNK"] == "128"
    for a, b in zip(three_calls(small, q, o, w), whole):      # eight launches each
        same_result(a, b)
    none = sphere.query_points(np.zeros((0, 3), f32))
    assert none["status"].shape == (0,) and none["normal"].shape == (0, 3) and all(x == 0 for x in none["counts"].values())
    assert sphere.project_points(np.zeros((0, 3), f32))["xyz"].shape == (0, 3) and sphere.cast_rays(np.zeros((0, 3), f32), np.zeros((0, 3), f32))["t"].shape == (0,)


def test_two_calls_same_bits_and_the_other_calls_undisturbed(built):
    from test_bake_gpu import scene_engine
    eng = scene_engine("SH1")[0]
    vs = vs_of(eng)
    idx0, bake0, rep0 = eng.extract_mesh_indexed(), eng.bake_lod(2 * vs, 4), eng.render_report()
    occ0 = eng.occlusion_points(idx0[0], idx0[1], 16)
    xyz, nrm = idx0[0], idx0[1]
    a, b = three_calls(eng, xyz, xyz + nrm * vs, -nrm), three_calls(eng, xyz, xyz + nrm * vs, -nrm)
    for x, y in zip(a, b):
        same_result(x, y)
    assert a[1]["counts"]["n_ok"] > 0.9 * len(xyz) and a[4]["counts"]["n_hits"] > 0.9 * len(xyz)
    for x, y in zip(idx0, eng.extract_mesh_indexed()):
        assert np.array_equal(x, y)
    same_bits(bake0, eng.bake_lod(2 * vs, 4))
    o1 = eng.occlusion_points(idx0[0], idx0[1], 16)
    same_bits(occ0, o1, [k for k in occ0 if k != "counts"]); assert occ0["counts"] == o1["counts"]
    assert rep0 == eng.render_report()


def test_a_call_between_two_iterations_changes_nothing(built):
    ends = []
    for ask in (False, True):
        sc = synth.make_scene(N=32, F=3, W=64, H=48, model="SH1")
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo()
        eng.iterate(capi.ALL, 1)
        if ask:
            xyz, nrm, _, _, _ = eng.extract_mesh_indexed()
            r = three_calls(eng, xyz, xyz + nrm * vs_of(eng), -nrm)
            assert r[0]["counts"]["n_ok"] == len(xyz) and r[3]["counts"]["n"] == len(xyz) and r[4]["counts"]["n_valid"] == len(xyz)
        eng.iterate(capi.ALL, 1)
        v = eng.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], eng.download_poses(), eng.download_light()))
    for x, y in zip(*ends):
        assert x.tobytes() == y.tobytes()


def test_errors(corner):
    eng = corner
    q, _ = corner_samples()
    up = np.tile(f32([0, 0, 1]), (len(q), 1))
    bad = [lambda: eng.query_points(q, 2), lambda: eng.query_points(q, -1), lambda: eng.project_points(q, 2), lambda: eng.project_points(q, max_iters=0), lambda: eng.project_points(q, max_iters=65),
           lambda: eng.project_points(q, tol=-1e-6), lambda: eng.project_points(q, tol=float("nan")), lambda: eng.project_points(q, tol=float("inf")), lambda: eng.project_points(q, reserved=1.0),
           lambda: eng.cast_rays(q, up, 1.0, 1.0), lambda: eng.cast_rays(q, up, 2.0, 1.0), lambda: eng.cast_rays(q, up, -1.0), lambda: eng.cast_rays(q, up, float("nan")),
           lambda: eng.cast_rays(q, up, float("inf")), lambda: eng.cast_rays(q, up, 0.0, float("nan"))]
    for call in bad:
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # PSGSDF_ERR_ARG
            call()
    assert eng.project_points(q, "cell", 0.0, 64)["counts"]["n"] == len(q)      # the ends of the ranges are in; the context still works
    assert eng.cast_rays(q + f32([0, 0, 0.01]), -up)["counts"]["n_hits"] == len(q)
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    fresh = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    for call in (lambda: fresh.query_points(q), lambda: fresh.project_points(q), lambda: fresh.cast_rays(q, up)):
        with pytest.raises(capi.PsgsdfError, match="rc=-4"):      # PSGSDF_ERR_STATE: no volume yet
            call()


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the context
    goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    outs = run_spec("_query_ranks_worker.py", tmp_path, "query", "json", 2, 150, {"N": 40, "F": 4, "callers": [1]})
    res = [json.load(open(o)) for o in outs]
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 3
    for e, name in zip(res[1]["errors"], ("query_points", "project_points", "cast_rays")):
        assert "rc=-3" in e and "rank 1 of 2" in e and name in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def read_query_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    kinds = {"float": "<f4", "uchar": "u1"}
    dt = np.dtype([(h.split()[2], kinds[h.split()[1]]) for h in head if h.startswith("property")])
    assert len(raw) == end + nv * dt.itemsize and not any(h.startswith("element face") for h in head)
    return head, np.frombuffer(raw, dt, nv, end)


def test_voxelps_query_ply(built, tmp_path):
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    first = str(tmp_path / "plain") + "/"
    for name, extra in (("plain", ["--indexed-mesh"]), ("points", ["--indexed-mesh", "--query-ply", first + "after_iter_3_mesh_indexed.ply"]),
                        ("project", ["--indexed-mesh", "--query-ply", first + "after_iter_3_mesh_indexed.ply", "--query-model", "cell", "--query-project"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    plain = sorted(f for f in os.listdir(outs["plain"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in plain if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes and not any("_query" in f for f in plain)
    _, verts, _ = read_ply_indexed(first + "after_iter_3_mesh_indexed.ply")
    xyz = np.stack([verts[k] for k in "xyz"], 1)
    for name in ("points", "project"):
        assert sorted(f for f in os.listdir(outs[name]) if f not in skip) == sorted(plain + [m + "_query.ply" for m in meshes])      # the only new files
        for f in plain:
            assert filecmp.cmp(outs["plain"] + f, outs[name] + f, shallow=False), f
    head, rec = read_query_ply(outs["points"] + "after_iter_3_query.ply")
    assert rec.dtype.names == ("x", "y", "z", "distance", "nx", "ny", "nz", "red", "green", "blue", "weight", "status") and len(rec) == len(xyz)
    assert any(h.startswith("comment query points model trilinear") for h in head)
    assert np.array_equal(np.stack([rec[k] for k in "xyz"], 1), xyz)
    ok = rec["status"] == 0
    worst = np.abs(rec["distance"][ok]).max() / 0.004
    print(f"after_iter_3: {len(rec)} vertices of its own mesh, status {np.bincount(rec['status']).tolist()}, max |phi| {worst:.2e} voxel")
    # The run's own vertices are zeros of the trilinear cell they were cut from.  Every vertex lies ON an edge of the grid, so float32 rounding of
    # its position can hand it to any of the cells that share the edge, and one of those may have an unobserved corner: status 2, never 1 or 3.
    # Positions reach 96 x 0.004 = 0.384, one float32 ulp there is 7.5e-6 voxel; the mesher's frame costs a few roundings per coordinate (DESIGN.md
    # 21 documents one ulp from the frame alone) and phi has a unit gradient: 6 ulps per coordinate, times sqrt(3), are 7.8e-5 voxel, below 1e-4.
    assert set(np.unique(rec["status"]).tolist()) <= {0, 2} and ok.sum() >= 0.95 * len(rec) and worst <= 1e-4
    assert not rec["distance"][~ok].any() and not rec["weight"][~ok].any()
    head, rec = read_query_ply(outs["project"] + "init_query.ply")
    assert rec.dtype.names == ("x", "y", "z", "distance", "residual", "iterations", "status") and len(rec) == len(xyz)
    assert any(h.startswith("comment query project model cell") for h in head)
    conv = rec["status"] == 0
    print(f"init: the last mesh's vertices projected under the cell model, status {np.bincount(rec['status']).tolist()}, moved up to {np.abs(rec['distance'][conv]).max() / 0.004:.3f} voxel")
    assert conv.sum() > 0.5 * len(rec) and (np.abs(rec["residual"][conv]) <= f32(1e-3 * f32(0.004))).all()
