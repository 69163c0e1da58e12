"""The welded mesh's definition without a GPU (include/psgsdf_mesh.h, DESIGN.md "Welded meshes"): the numpy restatement tests/_mesh_ref.py gives a
closed, oriented surface of the right genus on an analytic object, its z-slab shares concatenate to the one-piece arrays, and the binary PLY writer
of `voxelPS --indexed-mesh` writes what a PLY reader expects."""
import os
import subprocess

import numpy as np
import pytest

import _mesh_ref as ref
from psgradientsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")


def bumpy_volume(N=40, vs=0.01):
    """synth's bumpy sphere sampled on an N^3 grid: dist, its analytic gradient, weight 1 within 3 vs of the surface, a smooth albedo"""
    c = np.array([0.47, 0.52, 0.45]) * N * vs
    ax = np.arange(N) * vs
    X = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)      # x fastest
    f, g = synth._shape_f(X, c, 0.3 * N * vs, 0.01 * N * vs)
    rgb = synth._albedo(X, c, N * vs)
    v = dict(dist=f.astype(np.float32), grad=g.T.astype(np.float32), weight=(np.abs(f) < 3 * vs).astype(np.float32), rgb=rgb.T.astype(np.float32))
    # the cells stop one plane short of the crop box's far side (the reference's loop bound): an unobserved voxel with d = 0 in the far corner
    # stretches the box, so that the whole object is inside the cell range
    v["dist"][-1] = 0.0; v["weight"][-1] = 0.0
    return v, (N, N, N), vs, c


def test_restatement_is_closed_oriented_and_genus_zero():
    v, dim, vs, c = bumpy_volume()
    xyz, nrm, rgb, faces, first = ref.mesh(v, dim, vs)
    assert len(faces) > 5000 and first == 0
    closed, chi, bnd, over = ref.topology(faces, len(xyz))
    assert closed and chi == 2 and len(bnd) == 0 and over == 0
    assert np.array_equal(np.unique(faces), np.arange(len(xyz)))      # no unreferenced vertex
    # (positions: index * vs -- the frame's origin -vs lo cancels the crop box's offset -- the frame of the analytic field)
    p = xyz[faces].astype(np.float64)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    out = synth._shape_f(p.mean(1), c, 0.3 * 40 * vs, 0.01 * 40 * vs)[1]
    assert (np.einsum("ij,ij->i", fn, out) > 0).mean() >= 0.999
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-6)
    g = synth._shape_f(xyz.astype(np.float64), c, 0.3 * 40 * vs, 0.01 * 40 * vs)[1]
    cos = np.einsum("ij,ij->i", nrm.astype(np.float64), g) / np.linalg.norm(g, axis=1)
    assert np.median(np.degrees(np.arccos(np.clip(cos, -1, 1)))) < 3.0 and (cos > 0).all()      # vertex normals: the field's outward normal


@pytest.mark.parametrize("n_slabs", [2, 3, 4])
def test_slab_shares_concatenate_to_one_piece(n_slabs):
    v, dim, vs, _ = bumpy_volume(N=36)
    one = ref.mesh(v, dim, vs)
    cuts = [0] + [int(x) for x in np.linspace(0, dim[2], n_slabs + 1)[1:-1].round() + np.arange(n_slabs - 1) % 2] + [dim[2]]
    shares = ref.mesh(v, dim, vs, cuts=cuts)
    assert sum(len(s[3]) > 0 for s in shares) >= 2
    for q in range(4):
        assert np.array_equal(np.concatenate([s[q] for s in shares]), one[q])
    assert [s[4] for s in shares] == list(np.cumsum([0] + [len(s[0]) for s in shares[:-1]]))


def test_holes_have_boundary_only_at_unobserved_cells():
    v, dim, vs, _ = bumpy_volume(N=32)
    w = v["weight"].reshape(32, 32, 32).copy()
    w[12:16, 4:12, 8:20] = 0                      # a block of unobserved voxels through the surface
    v["weight"] = w.reshape(-1)
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    closed, chi, bnd, over = ref.topology(faces, len(xyz))
    assert not closed and over == 0 and len(bnd) > 0


def read_ply_indexed(path):
    """(header lines, vertex records, faces) of a binary little-endian PLY with the welded mesh's record layout"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize and vt.itemsize == 27 and ft.itemsize == 13
    verts = np.frombuffer(raw, vt, nv, end)
    fc = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (fc["n"] == 3).all()
    return head, verts, fc["v"].copy()


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_selftest_ply_indexed_parses_back(tmp_path):
    out = str(tmp_path / "octa.ply")
    r = subprocess.run([EXE, "--selftest-ply-indexed", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    head, verts, faces = read_ply_indexed(out)
    assert head == ["ply", "format binary_little_endian 1.0", "comment grid origin -0.25 0.5 1 voxel size 0.00400000019",
                    "element vertex 6", "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                    "property uchar red", "property uchar green", "property uchar blue", "element face 8", "property list uchar int vertex_indices", "end_header"]
    xyz = np.stack([verts[k] for k in "xyz"], 1)
    assert np.array_equal(xyz, np.array([[1.5, 0, 0], [-1.5, 0, 0], [0, 2.25, 0], [0, -2.25, 0], [0, 0, 0.75], [0, 0, -0.75]], np.float32))
    assert np.array_equal(np.stack([verts[k] for k in ("nx", "ny", "nz")], 1), np.sign(xyz))
    assert np.array_equal(np.stack([verts[k] for k in ("red", "green", "blue")], 1), [[255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3], [128, 64, 32], [7, 77, 177]])
    assert np.array_equal(faces, [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    closed, chi, _, _ = ref.topology(faces, 6)
    p = xyz[faces].astype(np.float64)
    assert closed and chi == 2 and (np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(1)) > 0).all()
