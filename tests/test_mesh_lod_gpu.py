"""The level-of-detail mesh by vertex clustering on the device (include/psgsdf_mesh.h psgsdf_extract_mesh_lod, csrc/mesh_lod.hip; DESIGN.md "Level of
detail"): everything against the yardstick tests/_mesh_lod_ref.py applied to the same context's own extract_mesh_indexed(), or to its
extract_mesh_components(**filter) when a filter is given.  Positions, colours, faces, the vertex map and the input sizes must match exactly; normals
within 2^-22 (the squares under the root are not exact in double and the compiler may contract them: a bound on double-rounding differences)."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _mesh_lod_ref as lref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, synth_engine, voxelps_config

pytestmark = pytest.mark.gpu
NORMAL_TOL = 2.0 ** -22
EXACT = ("xyz", "rgb", "faces", "vertex_map")


def input_mesh(eng, **flt):
    if flt:
        m = eng.extract_mesh_components(**flt)
        return m["xyz"], m["normals"], m["rgb"], m["faces"]
    return eng.extract_mesh_indexed()[:4]


def assert_matches_yardstick(eng, s, tag, src=None, **flt):
    """the device's answer for a cell of s voxels against the yardstick on the context's own input mesh (src, if the caller has it already)"""
    vs = vs_of(eng)
    xyz, nrm, rgb, faces = src if src is not None else input_mesh(eng, **flt)
    got = eng.extract_mesh_lod(s * vs, **flt)
    exp = lref.lod(xyz, nrm, rgb, faces, vs, s * vs)
    err = float(np.abs(got["normals"] - exp["normals"]).max()) if len(got["normals"]) == len(exp["normals"]) and len(exp["normals"]) else 0.0
    print(f"{tag} cell {s} vs {flt}: {got['n_vertices_in']} / {got['n_faces_in']} -> {len(got['xyz'])} vertices / {len(got['faces'])} faces (yardstick {len(exp['xyz'])} / {len(exp['faces'])}), "
          f"{exp['n_clusters']} clusters, {exp['n_collapsed']} collapsed, {exp['n_duplicates']} duplicates, {int((exp['vertex_map'] < 0).sum())} unmapped; normals max error {err:.3e}")
    assert got["n_vertices_in"] == len(xyz) and got["n_faces_in"] == len(faces), tag
    for k in EXACT:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (tag, s, k, got[k].shape, exp[k].shape)
    assert got["normals"].dtype == np.float32 and got["normals"].shape == exp["normals"].shape and err <= NORMAL_TOL, (tag, s, err)
    return got, exp


@pytest.fixture(scope="module")
def pieces(built):
    v, dim, vs = pieces_volume()
    eng = upload(v, dim, vs)
    src = input_mesh(eng)
    assert (len(src[0]), len(src[3])) == (3612, 7204)
    return eng, src


# wall ties (whole numbers of voxels), a cell that is no multiple, duplicates (2), a vanishing piece (4), everything in one cluster (64)
@pytest.mark.parametrize("s,sizes", [(0.25, (3396, 6772)), (1, (1985, 3960)), (1.37, None), (2, (785, 1560)), (3, (368, 721)), (4, (218, 424)), (64, (0, 0))])
def test_five_pieces(pieces, s, sizes):
    eng, src = pieces
    got, exp = assert_matches_yardstick(eng, s, "five pieces", src=src)
    if sizes:
        assert (len(got["xyz"]), len(got["faces"])) == sizes
    if s == 64:
        assert len(got["vertex_map"]) == 3612 and (got["vertex_map"] == -1).all()
    if s == 4:
        assert int((got["vertex_map"] < 0).sum()) == 24


@pytest.mark.parametrize("flt", [dict(keep_largest=2), dict(min_faces=300)])
def test_filtered_input(built, flt):
    v, dim, vs = pieces_volume(torus=True)
    eng = upload(v, dim, vs)
    full = eng.extract_mesh_indexed()
    got, _ = assert_matches_yardstick(eng, 2, "torus", **flt)
    assert 0 < got["n_vertices_in"] < len(full[0]) and len(got["vertex_map"]) == got["n_vertices_in"] and len(got["faces"]) > 100


@pytest.mark.parametrize("model,N,refine", [("SH1", 64, False), ("SH1", 32, True)])
def test_synthetic_scenes_through_the_optimiser(built, model, N, refine):
    """stored gradients of an optimised state as normals; refined: the voxel size has halved and the cell is given in the new one"""
    eng = synth_engine(model, N, refine)
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model=model)
    assert abs(vs_of(eng) / float(sc.voxel_size) - (0.5 if refine else 1.0)) < 1e-6
    tag = f"{model} N={N}{' refined' if refine else ''}"
    src = input_mesh(eng)
    assert len(src[3]) > 1000
    for s in (1, 2, 2.5):
        got, _ = assert_matches_yardstick(eng, s, tag, src=src)
    assert 0 < len(got["faces"]) < len(src[3]) // 4
    assert_matches_yardstick(eng, 2, tag, keep_largest=1)


def test_reproducible_leaves_the_other_calls_alone_errors_and_empty(built):
    v, dim, vs = pieces_volume(torus=True)
    eng = upload(v, dim, vs)
    vs = vs_of(eng)
    full = eng.extract_mesh_indexed()
    comp = eng.extract_mesh_components(keep_largest=1)
    for flt in (dict(), dict(keep_largest=2)):
        a, b = eng.extract_mesh_lod(2 * vs, **flt), eng.extract_mesh_lod(2 * vs, **flt)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (flt, k)
    for x, y in zip(full, eng.extract_mesh_indexed()):      # after the call: still the whole mesh, and the same filtered one
        assert np.array_equal(x, y)
    again = eng.extract_mesh_components(keep_largest=1)
    for k in comp:
        assert comp[k].tobytes() == again[k].tobytes(), k
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # PSGSDF_ERR_ARG
            eng.extract_mesh_lod(cell)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.extract_mesh_lod(2 * vs, keep_largest=-1)
    with pytest.raises(capi.PsgsdfError, match="rc=-3"):      # PSGSDF_ERR_UNSUPPORTED: coordinates beyond 2^20 cells
        eng.extract_mesh_lod(1e-7 * vs)
    assert_matches_yardstick(eng, 3, "after the refusals")      # the context still works
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):      # PSGSDF_ERR_STATE
        eng.extract_mesh_lod(0.1)
    n = 32 ** 3
    eng.upload_volume(np.full(n, 1.0, np.float32), np.zeros((3, n), np.float32), np.ones(n, np.float32), np.zeros((3, n), np.float32), np.zeros((n, 1), np.uint64), 1)
    for flt in (dict(), dict(keep_largest=1)):
        got = eng.extract_mesh_lod(0.1, **flt)
        assert got["n_vertices_in"] == 0 and got["n_faces_in"] == 0 and all(len(got[k]) == 0 for k in EXACT + ("normals",))


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "mesh_lod")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_mesh_lod(built, tmp_path):
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    for name, extra in (("plain", []), ("indexed", ["--indexed-mesh"]), ("lod", ["--indexed-mesh", "--mesh-lod", "2"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    plain = sorted(f for f in os.listdir(outs["plain"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in plain if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    names = sorted(f for f in os.listdir(outs["lod"]) if f not in skip)
    assert names == sorted(plain + [m + s for m in meshes for s in ("_mesh_indexed.ply", "_mesh_lod.ply")])      # the only new files
    assert sorted(f for f in os.listdir(outs["indexed"]) if f not in skip) == sorted(plain + [m + "_mesh_indexed.ply" for m in meshes])
    for f in plain:      # the flag changes no other file
        assert filecmp.cmp(outs["plain"] + f, outs["lod"] + f, shallow=False), f
    for m in meshes:
        assert filecmp.cmp(outs["indexed"] + m + "_mesh_indexed.ply", outs["lod"] + m + "_mesh_indexed.ply", shallow=False), m
        head, verts, faces = read_ply_indexed(outs["lod"] + m + "_mesh_indexed.ply")
        lhead, lverts, lfaces = read_ply_indexed(outs["lod"] + m + "_mesh_lod.ply")
        assert f"comment lod cell 2 voxels from {len(verts)} vertices {len(faces)} faces" in lhead
        assert [h for h in lhead if not h.startswith(("comment lod", "element"))] == [h for h in head if not h.startswith("element")]
        # the voxel size: %.9g digits reproduce a float32
        vs = float(np.float32(float(next(h for h in head if h.startswith("comment grid origin")).split()[-1])))
        cols = lambda rec, ks, dt: np.stack([rec[k] for k in ks], 1).astype(dt)
        exp = lref.lod(cols(verts, "xyz", np.float32), cols(verts, ("nx", "ny", "nz"), np.float32), cols(verts, ("red", "green", "blue"), np.uint8), faces, vs, 2.0 * vs)
        assert np.array_equal(cols(lverts, "xyz", np.float32), exp["xyz"]) and np.array_equal(cols(lverts, ("red", "green", "blue"), np.uint8), exp["rgb"]), m
        assert np.array_equal(lfaces, exp["faces"]), m
        assert np.abs(cols(lverts, ("nx", "ny", "nz"), np.float32) - exp["normals"]).max() <= NORMAL_TOL, m
        sizes = [os.path.getsize(outs["lod"] + m + s) for s in ("_mesh_indexed.ply", "_mesh_lod.ply")]
        print(f"{m}: {len(verts)} vertices / {len(faces)} faces / {sizes[0]} B -> {len(lverts)} / {len(lfaces)} / {sizes[1]} B at 2 voxels")
        assert 0 < len(lfaces) < len(faces) // 3
