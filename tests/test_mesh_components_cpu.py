"""Connected components of the welded mesh without a GPU (include/psgsdf_mesh.h psgsdf_extract_mesh_components, DESIGN.md "Mesh components"):
the yardstick tests/_mesh_components_ref.py itself on an analytic volume of five separate closed pieces (so that a wrong reference cannot hide),
the refusal of `voxelPS --gpus N --mesh-keep-largest K`, and the new kernels' resources."""
import os
import subprocess

import numpy as np
import pytest

import _mesh_components_ref as cref
import _mesh_ref as ref
from psgradientsdf_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
HIPCC = "/opt/rocm/bin/hipcc"

SPHERES = (((0.15, 0.2, 0.2), 2.6), ((0.85, 0.8, 0.3), 3.7), ((0.8, 0.15, 0.8), 1.3), ((0.2, 0.85, 0.85), 4.4))      # centre / (N vs), radius in voxels
TORUS = ((0.2, 0.25, 0.78), 6.0, 2.0)                                                                               # centre / (N vs), major, minor radius in voxels


def pieces_volume(N=48, vs=0.01, torus=False):
    """synth's bumpy sphere (radius 0.25 N vs) and four small spheres far from it and from each other, optionally a torus (axis z): the pointwise
    minimum of their distances with the gradient of whichever is nearer, weight 1 within 3 vs of the surface, a smooth albedo; x fastest.  The
    unobserved voxel with d = 0 in the far corner stretches the crop box beyond the objects (test_mesh_indexed_cpu.bumpy_volume)."""
    L = N * vs
    c = np.array([0.47, 0.52, 0.45]) * L
    ax = np.arange(N) * vs
    X = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)
    f, g = synth._shape_f(X, c, 0.25 * L, 0.01 * L)
    f = f.copy(); g = g.copy()
    for cs, r in SPHERES:
        p = X - np.array(cs) * L
        n = np.maximum(np.linalg.norm(p, axis=1), 1e-12)
        fs = n - r * vs
        m = fs < f
        f[m] = fs[m]; g[m] = (p / n[:, None])[m]
    if torus:
        ct, R, r = TORUS
        p = X - np.array(ct) * L
        rho = np.maximum(np.hypot(p[:, 0], p[:, 1]), 1e-12)
        q = np.maximum(np.hypot(rho - R * vs, p[:, 2]), 1e-12)
        ft = q - r * vs
        gt = np.stack([(rho - R * vs) / q * p[:, 0] / rho, (rho - R * vs) / q * p[:, 1] / rho, p[:, 2] / q], 1)
        m = ft < f
        f[m] = ft[m]; g[m] = gt[m]
    rgb = synth._albedo(X, c, L)
    v = dict(dist=f.astype(np.float32), grad=g.T.astype(np.float32).copy(), weight=(np.abs(f) < 3 * vs).astype(np.float32), rgb=rgb.T.astype(np.float32).copy())
    v["dist"][-1] = 0.0; v["weight"][-1] = 0.0
    return v, (N, N, N), vs


def closed_pieces(table):
    return bool(((table["n_boundary_edges"] == 0) & (table["n_nonmanifold_edges"] == 0)).all())


def euler(table):
    return (table["n_vertices"] - table["n_edges"] + table["n_faces"]).tolist()


def test_yardstick_on_five_closed_pieces():
    v, dim, vs = pieces_volume()
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    assert (len(xyz), len(faces)) == (3612, 7204)
    lab, t = cref.analyse(xyz, faces, vs)
    assert t["n_faces"].tolist() == [228, 5708, 516, 708, 44]
    assert t["first_vertex"].tolist() == [0, 54, 238, 3232, 3246]      # the pieces interleave in vertex order
    assert closed_pieces(t) and euler(t) == [2] * 5
    assert t["n_vertices"].sum() == len(xyz) and t["n_edges"].sum() == len(ref.edges(faces)) // 2
    assert (np.diff(lab) != 0).sum() > 5 and np.array_equal(np.unique(lab), np.arange(5))
    for k in range(5):      # the labels: smallest vertex, nothing shared between pieces, boxes of the pieces' own vertices
        own = np.nonzero(lab == k)[0]
        assert own[0] == t["first_vertex"][k] and len(own) == t["n_vertices"][k]
        assert np.array_equal(t["lo"][k], xyz[own].min(0)) and np.array_equal(t["hi"][k], xyz[own].max(0))
    assert (lab[faces] == lab[faces[:, :1]]).all()
    # area: the fixed-point sum is the plain float64 sum up to half a unit per face; a sphere of radius r has about 4 pi r^2
    p = xyz[faces].astype(np.float64)
    plain = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    for k in range(5):
        assert abs(t["area"][k] - plain[lab[faces[:, 0]] == k].sum()) <= 0.5 * t["n_faces"][k] * vs * vs / 2 ** 24
    assert abs(t["area"].min() / (vs * vs) - 17.2) < 0.05
    for k, (_, r) in zip((0, 2, 4, 3), SPHERES):
        assert abs(t["area"][k] / (4 * np.pi * (r * vs) ** 2) - 1) < 0.25, (k, r)      # (marching cubes cuts the corners of a sphere of 1.3 voxels: 0.81)

    got = cref.components(xyz, faces, vs, nrm, rgb, keep_largest=2)
    assert got["components"]["kept"].tolist() == [0, 1, 0, 1, 0]
    assert len(got["faces"]) == 5708 + 708 and np.array_equal(np.unique(got["vertex_component"]), [1, 3])
    got = cref.components(xyz, faces, vs, nrm, rgb, min_faces=100)
    assert got["components"]["kept"].tolist() == [1, 1, 1, 1, 0]
    assert len(got["faces"]) == 7204 - 44 and len(got["xyz"]) == 3612 - int(t["n_vertices"][4])
    # the filtered mesh: dense numbers, the kept pieces closed again, the same positions
    assert np.array_equal(np.unique(got["faces"]), np.arange(len(got["xyz"])))
    lab2, t2 = cref.analyse(got["xyz"], got["faces"], vs)
    assert t2["n_faces"].tolist() == [228, 5708, 516, 708] and closed_pieces(t2) and euler(t2) == [2] * 4
    assert np.array_equal(t2["area"], t["area"][:4]) and np.array_equal(t2["lo"], t["lo"][:4])
    closed, chi, bnd, over = ref.topology(got["faces"], len(got["xyz"]))
    assert closed and chi == 8 and over == 0
    # ties of keep_largest go to the smaller first vertex; an impossible filter keeps nothing and still lists everything
    tie = t.copy(); tie["n_faces"] = 7
    assert cref.keep(tie, keep_largest=2).tolist() == [1, 1, 0, 0, 0]
    none = cref.components(xyz, faces, vs, nrm, rgb, keep_largest=1, min_faces=6000)
    assert len(none["xyz"]) == 0 and len(none["faces"]) == 0 and len(none["components"]) == 5 and not none["components"]["kept"].any()


def test_yardstick_sees_a_handle():
    v, dim, vs = pieces_volume(torus=True)
    xyz, nrm, rgb, faces, _ = ref.mesh(v, dim, vs)
    lab, t = cref.analyse(xyz, faces, vs)
    assert t["n_faces"].tolist() == [228, 5708, 516, 1336, 708, 44] and closed_pieces(t)
    assert euler(t) == [2, 2, 2, 0, 2, 2]
    assert t["n_vertices"][3] == 668 and t["first_vertex"][3] == 3232


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
@pytest.mark.parametrize("flag", [["--mesh-keep-largest", "1"], ["--mesh-min-faces", "10"]])
def test_voxelps_refuses_the_filter_on_several_gpus(tmp_path, flag):
    r = subprocess.run([EXE, "--config_file", str(tmp_path / "none.json"), "--gpus", "2"] + flag, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert flag[0] in r.stderr and "--gpus" in r.stderr
    assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_component_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    res = resources("mesh_cc.hip", tmp_path)
    ks = {k: v for k, v in res.items() if "k_mcomp_" in k}
    assert len(ks) == 9 and all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in ks.values()), ks
