"""Connected components of the welded mesh on the device (include/psgsdf_mesh.h psgsdf_extract_mesh_components, csrc/mesh_cc.hip; DESIGN.md
"Mesh components"): everything against the yardstick tests/_mesh_components_ref.py applied to the same context's own extract_mesh_indexed()."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components  # noqa: F401  (the yardstick's; a missing scipy fails here, not inside a test)

import _mesh_components_ref as cref
import _mesh_ref as ref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_mesh_components_cpu import pieces_volume
from test_mesh_indexed_gpu import EXE, GOLD, analytic_engine, synth_engine, voxelps_config

pytestmark = pytest.mark.gpu
FILTERS = (dict(min_faces=100), dict(min_area=50.0), dict(keep_largest=2), dict(keep_largest=1, min_faces=6000))      # min_area in units of vs^2


def upload(v, dim, vs):
    sc = synth.make_scene(N=dim[0], F=2, W=64, H=48, model="SH1")
    g = capi.GridDesc(); g.dim[:] = list(dim); g.voxel_size = vs; g.shift[:] = [0.0, 0.0, 0.0]; g.truncation = 5 * vs
    eng = capi.load_engine(g, sc.K, capi.default_settings(capi.SH1), 0)
    n = dim[0] * dim[1] * dim[2]
    eng.upload_volume(v["dist"], v["grad"], v["weight"], v["rgb"], np.zeros((n, 1), np.uint64), 1)
    return eng


def vs_of(eng):
    return float(np.float32(eng.info().voxel_size))


def assert_matches_yardstick(eng, tag, **flt):
    """the device's answer for one filter against the yardstick on the context's own unfiltered welded mesh; returns (device dict, yardstick dict)"""
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    vs = vs_of(eng)
    got = eng.extract_mesh_components(**flt)
    exp = cref.components(xyz, faces, vs, nrm, rgb, **flt)
    t, e = got["components"], exp["components"]
    assert len(t) == len(e), (tag, len(t), len(e))
    for k in cref.INT_FIELDS:
        assert np.array_equal(t[k], e[k]), (tag, k, t[k][:8], e[k][:8])
    assert np.array_equal(t["lo"], e["lo"]) and np.array_equal(t["hi"], e["hi"]), tag
    err = np.abs(t["area"] - e["area"]); tol = e["n_faces"] * vs * vs / 2 ** 24
    print(f"{tag} {flt}: {len(t)} components, kept {int(t['kept'].sum())}, largest {int(t['n_faces'].max()) if len(t) else 0} of {len(faces)} faces; "
          f"area max error {float((err / (vs * vs / 2 ** 24)).max()) if len(t) else 0.0:.3f} units, bit-equal {bool(np.array_equal(t['area'], e['area']))}")
    assert (err <= tol).all(), (tag, err.max(), tol.min())
    assert np.array_equal(t["kept"], e["kept"]) and not t["reserved"].any(), (tag, t["kept"], e["kept"])
    for k in ("xyz", "normals", "rgb", "faces", "vertex_component"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (tag, k, got[k].shape, exp[k].shape)
    return got, exp


def test_five_pieces_labels_table_and_filters(built):
    v, dim, vs = pieces_volume()
    eng = upload(v, dim, vs)
    full = eng.extract_mesh_indexed()
    assert (len(full[0]), len(full[3])) == (3612, 7204)
    got, exp = assert_matches_yardstick(eng, "five pieces")
    for q, k in enumerate(("xyz", "normals", "rgb", "faces")):      # nothing filtered: the welded mesh itself
        assert np.array_equal(got[k], full[q]), k
    t = got["components"]
    assert t["n_faces"].tolist() == [228, 5708, 516, 708, 44] and t["first_vertex"].tolist() == [0, 54, 238, 3232, 3246] and t["kept"].all()
    assert (t["n_vertices"] - t["n_edges"] + t["n_faces"]).tolist() == [2] * 5 and not t["n_boundary_edges"].any() and not t["n_nonmanifold_edges"].any()
    f32vs = vs_of(eng)
    kept = []
    for flt in FILTERS:
        flt = dict(flt)
        if "min_area" in flt:
            flt["min_area"] *= f32vs * f32vs
        g, _ = assert_matches_yardstick(eng, "five pieces", **flt)
        kept.append(g["components"]["kept"].tolist())
    assert kept[0] == [1, 1, 1, 1, 0] and kept[2] == [0, 1, 0, 1, 0] and kept[3] == [0] * 5
    assert 0 < sum(kept[1]) < 5      # (50 vs^2 lies between the pieces' areas)


def test_handle_and_boundary(built):
    v, dim, vs = pieces_volume(torus=True)
    eng = upload(v, dim, vs)
    got, _ = assert_matches_yardstick(eng, "torus")
    t = got["components"]
    assert t["n_faces"].tolist() == [228, 5708, 516, 1336, 708, 44]
    assert (t["n_vertices"] - t["n_edges"] + t["n_faces"]).tolist() == [2, 2, 2, 0, 2, 2]
    assert t["n_vertices"][3] == 668 and t["first_vertex"][3] == 3232
    assert not t["n_boundary_edges"].any() and not t["n_nonmanifold_edges"].any()
    assert_matches_yardstick(eng, "torus", keep_largest=3)
    eng, _, vs, _ = analytic_engine(hole=True)
    got, _ = assert_matches_yardstick(eng, "hole")
    xyz, _, _, faces, _ = eng.extract_mesh_indexed()
    bnd = ref.topology(faces, len(xyz))[2]
    assert len(got["components"]) == 1 and got["components"]["n_boundary_edges"][0] == len(bnd) > 0


def test_sokrates_fused_and_optimised(built):
    from test_render_gpu import _load_multiview
    K, color, depth, poses = _load_multiview(GOLD)
    F, vs = len(poses), 0.004
    ys, xs = np.nonzero(depth[0] > 0)
    z = depth[0][ys, xs].astype(np.float64)
    pc = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], 1)
    centre = (pc @ poses[0][:3, :3].T.astype(np.float64) + poses[0][:3, 3]).mean(0)
    g = capi.GridDesc(); g.dim[:] = [128, 128, 128]; g.voxel_size = vs; g.shift[:] = [float(x) for x in centre]; g.truncation = 5 * vs
    eng = capi.load_engine(g, K.reshape(-1), capi.default_settings(capi.SH1), 0)
    eng.volume_init(F)
    for f in range(F):
        eng.integrate_frame(color[f], depth[f], eng.estimate_normals(depth[f]), poses[f], f, z_min=0.5, z_max=3.5)
    eng.set_keyframes(np.arange(F, dtype=np.int32), np.stack(color), np.stack(poses).reshape(F, 16))
    eng.init()
    eng.init_albedo()
    got, _ = assert_matches_yardstick(eng, "sokrates fused")
    t = got["components"]
    nf = int(t["n_faces"].sum())
    print(f"sokrates fused: {len(t)} components, faces {sorted(t['n_faces'].tolist(), reverse=True)[:16]}")
    assert len(t) > 1
    one, _ = assert_matches_yardstick(eng, "sokrates fused", keep_largest=1)
    assert one["components"]["kept"].sum() == 1 and len(np.unique(one["vertex_component"])) == 1
    assert len(one["faces"]) >= 0.99 * nf and len(one["faces"]) == t["n_faces"].max()
    assert_matches_yardstick(eng, "sokrates fused", min_faces=9)
    eng.optimize(capi.ALL)
    got, _ = assert_matches_yardstick(eng, "sokrates optimised")
    t = got["components"]
    print(f"sokrates optimised: {len(t)} components, largest share {t['n_faces'].max() / t['n_faces'].sum():.5f}")
    assert_matches_yardstick(eng, "sokrates optimised", keep_largest=1)


@pytest.mark.parametrize("model,N,refine", [("SH1", 64, False), ("SH1", 32, True)])
def test_synthetic_scenes_through_the_optimiser(built, model, N, refine):
    eng = synth_engine(model, N, refine)
    tag = f"{model} N={N}{' refined' if refine else ''}"
    got, _ = assert_matches_yardstick(eng, tag)
    assert len(got["faces"]) > 1000
    assert_matches_yardstick(eng, tag, keep_largest=1)
    assert_matches_yardstick(eng, tag, min_faces=4)


def test_reproducible_leaves_the_full_mesh_alone_empty_and_state_error(built):
    v, dim, vs = pieces_volume(torus=True)
    eng = upload(v, dim, vs)
    full = eng.extract_mesh_indexed()
    for flt in (dict(), dict(keep_largest=2), dict(min_faces=300)):
        a, b = eng.extract_mesh_components(**flt), eng.extract_mesh_components(**flt)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (flt, k)
    again = eng.extract_mesh_indexed()      # after a filtered call: still the whole mesh
    for x, y in zip(full, again):
        assert np.array_equal(x, y)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # PSGSDF_ERR_ARG
        eng.extract_mesh_components(keep_largest=-1)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.extract_mesh_components(min_area=float("nan"))
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):
        eng.extract_mesh_components()
    n = 32 ** 3
    eng.upload_volume(np.full(n, 1.0, np.float32), np.zeros((3, n), np.float32), np.ones(n, np.float32), np.zeros((3, n), np.float32), np.zeros((n, 1), np.uint64), 1)
    got = eng.extract_mesh_components(keep_largest=1)
    assert len(got["components"]) == 0 and len(got["xyz"]) == 0 and len(got["faces"]) == 0 and len(got["vertex_component"]) == 0
    assert got["components"].dtype == capi.MESH_COMPONENT_DTYPE == cref.DTYPE


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "mesh_components")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_clean_mesh(built, tmp_path):
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    for name, extra in (("plain", []), ("indexed", ["--indexed-mesh"]), ("clean", ["--indexed-mesh", "--mesh-keep-largest", "1"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    plain = sorted(f for f in os.listdir(outs["plain"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in plain if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    names = sorted(f for f in os.listdir(outs["clean"]) if f not in skip)
    assert names == sorted(plain + [m + s for m in meshes for s in ("_mesh_indexed.ply", "_mesh_clean.ply", "_mesh_components.txt")])
    for f in plain:      # the flags change no other file
        assert filecmp.cmp(outs["plain"] + f, outs["clean"] + f, shallow=False), f
    for m in meshes:
        assert filecmp.cmp(outs["indexed"] + m + "_mesh_indexed.ply", outs["clean"] + m + "_mesh_indexed.ply", shallow=False), m
        head, verts, faces = read_ply_indexed(outs["clean"] + m + "_mesh_indexed.ply")
        chead, cverts, cfaces = read_ply_indexed(outs["clean"] + m + "_mesh_clean.ply")
        lab, first = cref.labels_of(faces, len(verts))
        big = int(np.argmax(np.bincount(lab[faces[:, 0]])))      # (argmax: the first of equals = the smaller first vertex)
        assert f"comment components kept 1 of {len(first)}" in chead and [h for h in chead if not h.startswith(("comment components", "element"))] == [h for h in head if not h.startswith("element")]
        vk = lab == big
        assert cverts.tobytes() == verts[vk].tobytes(), m      # positions, normals, colours bit-equal
        new = np.cumsum(vk) - 1
        assert np.array_equal(cfaces, new[faces[vk[faces[:, 0]]]]), m
        assert len(cref.labels_of(cfaces, len(cverts))[1]) == 1
        lines = open(outs["clean"] + m + "_mesh_components.txt").read().splitlines()
        assert len(lines) == len(first), m
        rows = np.array([ln.split() for ln in lines], np.float64)
        assert rows.shape[1] == 14 and rows[:, 0].astype(int).tolist() == first.tolist() and rows[:, 13].astype(int).tolist() == [int(i == big) for i in range(len(first))]
        print(f"{m}: {len(first)} components, the largest {len(cfaces)} of {len(faces)} faces")
