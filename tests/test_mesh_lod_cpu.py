"""The level-of-detail mesh by vertex clustering without a GPU (include/psgsdf_mesh.h psgsdf_extract_mesh_lod, DESIGN.md "Level of detail"): the
yardstick tests/_mesh_lod_ref.py on a hand-written mesh whose answer is spelled out here (so that a wrong yardstick cannot hide) and on the analytic
five-piece volume of test_mesh_components_cpu, the refusals of `voxelPS --mesh-lod`, and the new kernels' resources."""
import os
import subprocess

import numpy as np
import pytest

import _mesh_lod_ref as lref
import _mesh_ref as ref
from test_mesh_components_cpu import EXE, HIPCC, pieces_volume

f32 = np.float32


def test_hand_written_mesh():
    """cell = 1, vs = 0.5.  Clusters: A = {0, 1}, B = {2} (x = 1.0 exactly: on the wall, so in the upper cell), C = {3, 4}, D = {5}, E = {6, 7},
    G = {8}, H = {9, 10} (negative coordinates)."""
    xyz = np.array([[0.25, 0.25, 0.25], [0.75, 0.5, 0.25], [1.0, 0.25, 0.25], [0.5, 1.5, 0.5], [0.25, 1.25, 0.75], [1.5, 1.5, 0.5],
                    [2.5, 0.5, 0.5], [2.25, 0.75, 0.25], [2.5, 1.5, 0.5], [-0.25, 0.5, 0.5], [-0.5, 0.25, 0.25]], f32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0.1, 0.2, 0.3], [1, 0, 0], [0, 1, 0], [0, 0.6, 0.8], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]], f32)
    rgb = np.array([[10, 20, 30], [11, 21, 33], [7, 8, 9], [100, 0, 255], [101, 0, 255], [50, 60, 70], [1, 1, 1], [2, 2, 2], [3, 3, 3], [1, 2, 3], [2, 2, 4]], np.uint8)
    faces = np.array([[0, 1, 2],      # A A B: collapses
                      [0, 2, 3],      # A B C: kept
                      [4, 2, 1],      # C B A: the triple of face 1 the other way round -- the lower index wins
                      [2, 5, 3],      # B D C: kept
                      [6, 7, 8],      # E E G: collapses, and nothing else uses E or G
                      [9, 0, 3]],     # H A C: kept
                     np.int32)
    assert lref.clusters(xyz, 1.0).tolist()[2] == [1, 0, 0] and lref.clusters(xyz, 1.0).tolist()[9] == [-1, 0, 0]
    got = lref.lod(xyz, nrm, rgb, faces, 0.5, 1.0)
    assert got["n_vertices_in"] == 11 and got["n_faces_in"] == 6 and got["n_clusters"] == 7 and got["n_collapsed"] == 2 and got["n_duplicates"] == 1
    assert got["vertex_map"].tolist() == [0, 0, 1, 2, 2, 3, -1, -1, -1, 4, 4]      # by smallest member: A B C D H (H has the smallest key and the last number)
    assert got["faces"].tolist() == [[0, 1, 2], [1, 3, 2], [4, 0, 2]] and got["faces"].dtype == np.int32
    assert got["xyz"].dtype == f32 and got["xyz"].tolist() == [[0.5, 0.375, 0.25], [1.0, 0.25, 0.25], [0.375, 1.375, 0.625], [1.5, 1.5, 0.5], [-0.375, 0.375, 0.375]]
    assert got["rgb"].tolist() == [[11, 21, 32], [7, 8, 9], [101, 0, 255], [50, 60, 70], [2, 2, 4]]      # halves round up: 10.5, 20.5, 31.5
    r = 0.7071067811865476
    exp_n = np.array([[0, 0, 1], [0.1, 0.2, 0.3], [r, r, 0], [0, 0.6, 0.8], [0, 0, 0]], f32)      # B and D keep their (here: not even unit) normals; H cancels
    assert np.abs(got["normals"] - exp_n).max() <= 2.0 ** -22
    assert got["normals"][1].tobytes() == nrm[2].tobytes() and got["normals"][3].tobytes() == nrm[5].tobytes() and got["normals"][4].tolist() == [0, 0, 0]
    assert got["xyz"][1].tobytes() == xyz[2].tobytes()
    # arguments the call refuses
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lref.lod(xyz, nrm, rgb, faces, 0.5, cell)
    with pytest.raises(ValueError):
        lref.lod(xyz, nrm, rgb, faces, 0.5, 1e-6)      # 2.5 / 1e-6 > 2^20
    empty = lref.lod(np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32), 0.5, 1.0)
    assert len(empty["xyz"]) == 0 and len(empty["faces"]) == 0 and len(empty["vertex_map"]) == 0


def invariants(got, xyz, faces, cell):
    """what holds for any correct output, whatever the mesh"""
    f, vm = got["faces"].astype(np.int64), got["vertex_map"].astype(np.int64)
    V = len(got["xyz"])
    assert len(got["normals"]) == V and len(got["rgb"]) == V and len(vm) == len(xyz)
    if len(f):
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()      # three distinct vertices
        assert len(np.unique(np.sort(f, 1), axis=0)) == len(f)                                                # no two faces share a triple
    assert np.array_equal(np.unique(f), np.arange(V))                                                         # every output vertex is used by a face
    assert np.array_equal(np.unique(vm[vm >= 0]), np.arange(V)) and vm.min(initial=0) >= -1                   # the map is onto 0 .. V - 1
    firsts = np.full(V, len(vm), np.int64)
    np.minimum.at(firsts, vm[vm >= 0], np.nonzero(vm >= 0)[0])
    assert (np.diff(firsts) > 0).all()                                                                        # ordered by smallest member
    # every kept face is an input face mapped, and they come in input order
    mapped = vm[np.asarray(faces, np.int64)]
    rows = {}
    for q, row in enumerate(mapped.tolist()):
        rows.setdefault(tuple(row), q)
    src = [rows[tuple(r)] for r in f.tolist()]
    assert src == sorted(src) and len(set(src)) == len(src)
    c = lref.clusters(xyz, cell)
    for o in range(min(V, 50)):      # the members of an output vertex are one cluster
        assert len(np.unique(c[vm == o], axis=0)) == 1


COUNTS = {0.25: (3396, 6772), 1: (1985, 3960), 2: (785, 1560), 3: (368, 721), 4: (218, 424), 64: (0, 0)}


def test_yardstick_on_five_pieces():
    v, dim, vs = pieces_volume()
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    assert (len(xyz), len(faces)) == (3612, 7204)
    vs32 = float(f32(vs))
    wall = np.abs(xyz.astype(np.float64) / (2 * vs32) - np.round(xyz.astype(np.float64) / (2 * vs32))).min()
    assert wall == 0.0      # vertices sit exactly on cell walls: the quotient's bits decide
    for s, (nv, nf) in COUNTS.items():
        got = lref.lod(xyz, nrm, rgb, faces, vs, s * vs32)
        assert (len(got["xyz"]), len(got["faces"])) == (nv, nf), (s, len(got["xyz"]), len(got["faces"]))
        invariants(got, xyz, faces, s * vs32)
        if s == 0.25:
            assert got["n_single"] == 3209 and got["n_duplicates"] == 0
            vm = got["vertex_map"]; m = vm >= 0
            one = np.bincount(vm[m], minlength=nv) == 1      # single-member clusters keep their bits
            src = np.full(nv, len(vm)); np.minimum.at(src, vm[m], np.nonzero(m)[0])
            for k, a in (("xyz", xyz), ("normals", nrm), ("rgb", rgb)):
                assert got[k][one].tobytes() == a[src[one]].tobytes(), k
        if s == 2:
            assert got["n_collapsed"] == 5640 and got["n_duplicates"] == 4
        if s == 4:
            assert got["n_clusters"] == 220 and int((got["vertex_map"] < 0).sum()) == 24      # the 44-face sphere collapses
        if s == 64:
            assert got["n_clusters"] == 1 and (got["vertex_map"] == -1).all()
        # positions: the mean of the members within the fixed point's half unit per member and float32's rounding
        if nv:
            vm = got["vertex_map"]; m = vm >= 0
            mean = np.zeros((nv, 3)); np.add.at(mean, vm[m], xyz[m].astype(np.float64)); mean /= np.bincount(vm[m])[:, None]
            assert np.abs(got["xyz"] - mean).max() <= 0.5 * vs32 / 2 ** 20 + np.spacing(f32(48 * vs32))
            assert np.abs(np.linalg.norm(got["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_yardstick_with_the_torus():
    v, dim, vs = pieces_volume(torus=True)
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    assert (len(xyz), len(faces)) == (4280, 8540)
    vs32 = float(f32(vs))
    for s, exp in ((2, (933, 1851)), (3, (441, 871))):
        got = lref.lod(xyz, nrm, rgb, faces, vs, s * vs32)
        assert (len(got["xyz"]), len(got["faces"])) == exp
        invariants(got, xyz, faces, s * vs32)


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_lod_on_several_gpus_and_a_bad_cell(tmp_path):
    r = subprocess.run([EXE, "--config_file", str(tmp_path / "none.json"), "--mesh-lod", "2", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--mesh-lod" in r.stderr and "--gpus" in r.stderr
    assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read
    for bad in ("0", "-1", "two", "nan", "inf"):
        r = subprocess.run([EXE, "--config_file", str(tmp_path / "none.json"), "--mesh-lod", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--mesh-lod" in r.stderr and "load the config file" not in r.stdout, (bad, r.stdout + r.stderr)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lod_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    res = resources("mesh_lod.hip", tmp_path)
    ks = {k: v for k, v in res.items() if "k_mlod_" in k}
    assert len(ks) == 5 and all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in ks.values()), ks
