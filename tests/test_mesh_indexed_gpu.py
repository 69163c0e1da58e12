"""The welded, indexed mesh on the device (include/psgsdf_mesh.h psgsdf_extract_mesh_indexed, csrc/mesh.hip; DESIGN.md "Welded meshes"):
against the numpy restatement tests/_mesh_ref.py, against psgsdf_extract_mesh's non-indexed faces, its topology on a closed object and around
holes, the empty cases, multi-rank shares, voxelPS --indexed-mesh, and the kernels' resources."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _mesh_ref as ref
from _ranks import NCU, run_spec, stitch
from psgradientsdf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS")
GOLD = os.path.join(ROOT, "tests", "golden", "sokrates_small")


def ulps(a, b):
    """distance in units of the last place between float32 arrays"""
    a, b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def state(eng):
    v = eng.download_volume(); i = eng.info()
    return v, [int(x) for x in i.dim], float(i.voxel_size)


def assert_matches_restatement(got, v, dim, vs):
    xyz, nrm, rgb, faces, first = got
    exp = ref.mesh(v, dim, vs)
    assert first == 0 and np.array_equal(faces, exp[3]), (len(faces), len(exp[3]))
    assert len(xyz) == len(exp[0])
    assert ulps(xyz, exp[0]).max() <= 1
    assert np.abs(nrm - exp[1]).max() <= 2e-7
    assert np.abs(rgb.astype(int) - exp[2].astype(int)).max() <= 1


def assert_same_surface_as_extract_mesh(eng, got, vs, tag):
    """the non-indexed mesh of the same state: the same faces in the same order, the same corner positions up to the reversed edges' rounding"""
    xyz, _, _, faces, _ = got
    xn, _ = eng.extract_mesh()
    assert len(xn) == 3 * len(faces), (tag, len(xn) // 3, len(faces))
    p = xyz[faces].reshape(-1, 3)
    tol = np.maximum(2 * np.spacing(np.abs(xn)), np.float32(1e-6 * vs))
    bad = np.abs(p - xn) > tol
    exact = (p == xn).all(1).mean()
    print(f"{tag}: {len(faces)} faces, {len(xyz)} vertices (non-indexed: {len(xn)}); corners bit-equal {exact:.4f}; beyond tolerance {int(bad.any(1).sum())}")
    assert not bad.any()
    assert exact > 0.25      # (the cell edges that run along their axis give the same float: about two thirds of the corners)


def synth_engine(model, N, refine=False):
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model=model)
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.load_scene(sc)
    eng.init_albedo(); eng.normalize_weights()
    eng.iterate(capi.ALL, 2)
    if refine:
        eng.upsample2x()
        eng.iterate(capi.ALL, 1)
    return eng


@pytest.mark.parametrize("model,N,refine", [("SH1", 64, False), ("LED", 48, False), ("SH1", 32, True)])
def test_matches_the_restatement_and_extract_mesh(built, model, N, refine):
    eng = synth_engine(model, N, refine)
    got = eng.extract_mesh_indexed()
    v, dim, vs = state(eng)
    assert len(got[3]) > 1000
    assert_matches_restatement(got, v, dim, vs)
    assert_same_surface_as_extract_mesh(eng, got, vs, f"{model} N={N}{' refined' if refine else ''}")
    again = eng.extract_mesh_indexed()      # reproducible bit for bit
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_sokrates_fused_and_optimised(built):
    """the sokrates fixture fused at its poses (128^3 at 4 mm, tests/test_render_gpu.py's set-up) and optimised"""
    from test_render_gpu import _load_multiview
    K, color, depth, poses = _load_multiview(GOLD)
    F, vs = len(poses), 0.004
    d0 = depth[0]
    ys, xs = np.nonzero(d0 > 0)
    z = d0[ys, xs].astype(np.float64)
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
    eng.optimize(capi.ALL)
    got = eng.extract_mesh_indexed()
    v, dim, vs = state(eng)
    assert len(got[3]) > 10000
    assert_matches_restatement(got, v, dim, vs)
    assert_same_surface_as_extract_mesh(eng, got, vs, "sokrates")
    closed, chi, bnd, over = ref.topology(got[3], len(got[0]))
    print(f"sokrates: vertices {len(got[0])}, faces {len(got[3])}, non-indexed vertices {3 * len(got[3])}; boundary edges {len(bnd)}, chi {chi}")
    assert over == 0


def analytic_engine(N=48, hole=False):
    """synth's bumpy sphere, uploaded as a volume (its analytic distance and gradient); weight 1 within 3 voxels of the surface.  An unobserved
    voxel with d = 0 in the far corner stretches the crop box beyond the object (the cells stop one plane short of its far side)."""
    sc = synth.make_scene(N=N, F=2, W=64, H=48, model="SH1")
    vs = float(sc.voxel_size)
    idx = np.stack(np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)
    X = idx * vs
    c = np.array([0.47, 0.52, 0.45]) * N * vs
    R0, A = 0.3 * N * vs, 0.01 * N * vs
    f, gr = synth._shape_f(X, c, R0, A)
    dist = f.astype(np.float32); weight = (np.abs(f) < 3 * vs).astype(np.float32)
    dist[-1] = 0.0; weight[-1] = 0.0
    if hole:
        w = weight.reshape(N, N, N); w[N // 2 - 2:N // 2 + 2, 2:N // 2, N // 3:2 * N // 3] = 0
    rgb = synth._albedo(X, c, N * vs).T.astype(np.float32)
    g = capi.GridDesc(); g.dim[:] = [N, N, N]; g.voxel_size = vs; g.shift[:] = [0.0, 0.0, 0.0]; g.truncation = 5 * vs
    eng = capi.load_engine(g, sc.K, capi.default_settings(capi.SH1), 0)
    eng.upload_volume(dist, gr.T.astype(np.float32).copy(), weight, rgb, np.zeros((N ** 3, 1), np.uint64), 1)
    return eng, (c, R0, A), vs, weight


def test_closed_object_topology_and_normals(built):
    eng, (c, R0, A), vs, _ = analytic_engine(N=96)      # (the bumps change fastest near the poles: the stored gradients resolve them from about 96 voxels on)
    xyz, nrm, rgb, faces, first = got = eng.extract_mesh_indexed()
    v, dim, _ = state(eng)
    assert_matches_restatement(got, v, dim, vs)
    closed, chi, bnd, over = ref.topology(faces, len(xyz))
    assert closed and chi == 2 and over == 0
    assert np.array_equal(np.unique(faces), np.arange(len(xyz)))
    lin = np.round(xyz / vs).astype(np.int64)
    on_grid = (np.abs(xyz / vs - lin) < 1e-4).all(1)         # snapped corners sit on voxel centres; every other vertex has a position of its own
    u = np.unique(xyz[~on_grid], axis=0)
    assert len(u) == int((~on_grid).sum())
    gt = synth._shape_f(xyz.astype(np.float64), c, R0, A)[1]
    ang = np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", nrm, gt) / np.linalg.norm(gt, axis=1), -1, 1)))
    print(f"normals vs analytic: median {np.median(ang):.3f} deg, p99 {np.percentile(ang, 99):.3f} deg")
    assert np.median(ang) < 3 and np.percentile(ang, 99) < 10
    p = xyz[faces].astype(np.float64)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", fn, nrm[faces].sum(1)) > 0).mean() >= 0.999


def test_holes_leave_boundaries_only_at_unobserved_cells(built):
    eng, _, vs, weight = analytic_engine(hole=True)
    xyz, nrm, rgb, faces, _ = got = eng.extract_mesh_indexed()
    v, dim, _ = state(eng)
    assert_matches_restatement(got, v, dim, vs)
    closed, chi, bnd, over = ref.topology(faces, len(xyz))
    assert not closed and over == 0 and len(bnd) > 0
    N = dim[0]
    lo, hi = ref.crop_box(v["dist"], dim, vs)
    w = weight.reshape(N, N, N)
    for e in bnd:      # the cells around a boundary edge: one of them is next to an unobserved voxel, or the edge is on the crop border
        mid = (xyz[e[0]].astype(np.float64) + xyz[e[1]]) / 2 / vs
        a, b = np.floor(mid - 1).astype(int), np.ceil(mid + 1).astype(int) + 1
        near = w[max(a[2], 0):b[2], max(a[1], 0):b[1], max(a[0], 0):b[0]]
        border = (mid <= lo + 1).any() or (mid >= hi - 2).any()
        assert (near == 0).any() or border, mid


def test_empty_volume_state_error_and_reproducible(built):
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):
        eng.extract_mesh_indexed()
    n = 32 ** 3
    eng.upload_volume(np.full(n, 1.0, np.float32), np.zeros((3, n), np.float32), np.ones(n, np.float32), np.zeros((3, n), np.float32), np.zeros((n, 1), np.uint64), 1)
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    assert len(xyz) == 0 and len(faces) == 0 and first == 0


def run_ranks(tmp_path, world, timeout=150, **spec):
    return [dict(np.load(o)) for o in run_spec("_mesh_ranks_worker.py", tmp_path, "mesh", "npz", world, timeout, spec)]


@pytest.mark.parametrize("world,mode,N", [(2, "iterate", 48), (3, "refine", 32), (4, "fuse_rebalance", 48), (3, "iterate", 40)])
def test_rank_shares_concatenate_to_the_single_context(built, tmp_path, world, mode, N):
    res = run_ranks(tmp_path, world, model="SH1", N=N, F=5, mode=mode)
    res.sort(key=lambda r: int(r["cut"][0]))
    dim = [int(x) for x in res[0]["dim"]]; vs = float(res[0]["vs"]); n = dim[0] * dim[1] * dim[2]
    v = dict(dist=stitch(res, "dist"), grad=stitch(res, "grad"), weight=stitch(res, "weight"), rgb=stitch(res, "rgb_vol"))
    sc = synth.make_scene(N=N, F=2, W=64, H=48, model="SH1")
    g = capi.GridDesc(); g.dim[:] = dim; g.voxel_size = vs; g.shift[:] = [float(x) for x in sc.shift]; g.truncation = 5 * vs
    one = capi.load_engine(g, sc.K, capi.default_settings(capi.SH1), 0)
    one.upload_volume(v["dist"], v["grad"], v["weight"], v["rgb"], np.zeros((n, 1), np.uint64), 1)
    exp = one.extract_mesh_indexed()
    assert len(exp[3]) > 1000 and sum(len(r["faces"]) > 0 for r in res) >= 2
    for q, k in enumerate(("xyz", "nrm", "rgb", "faces")):
        assert np.array_equal(np.concatenate([r[k] for r in res]), exp[q]), k
    assert [int(r["first"]) for r in res] == list(np.cumsum([0] + [len(r["xyz"]) for r in res[:-1]]))
    assert all(bool(r["same_again"]) for r in res)
    assert_matches_restatement(exp, v, dim, vs)


def voxelps_config(out, **kw):
    cfg = {"input": GOLD + "/", "output": out, "pose filename": "pose.txt", "datatype": "multiview", "first": 0, "last": 7, "voxel size": 0.004,
           "truncation factor": 5, "zmin": 0.5, "zmax": 3.5, "sharpness threshold": 0.0, "model type": "SH1", "loss function": "cauchy",
           "reg albedo": 0.0, "reg norm": 10.0, "reg laplacian": 0.0, "max iter": 7, "damping": 1.0, "converge threshold": 1e-9, "lambda": 0.2,
           "upsample": False, "--light": True, "--albedo": True, "--distance": True, "--pose": True, "grid dim": 96}
    cfg.update(kw)
    json.dump(cfg, open(out + "config.json", "w"))
    return out + "config.json"


def ascii_mesh(path):
    raw = open(path, "rb").read()
    cut = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:cut].decode()
    nv = int(head.split("element vertex ")[1].split()[0]); nf = int(head.split("element face ")[1].split()[0])
    lines = raw[cut:].split(b"\n")
    v = np.array(b" ".join(lines[:nv]).split(), np.float64).reshape(nv, -1)
    return v[:, :3], nf


def test_voxelps_indexed_mesh(built, tmp_path):
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    runs = (("plain", [], {}), ("indexed", ["--indexed-mesh"], {}),
            ("ranks", ["--indexed-mesh", "--gpus", "2", "--transport", "sockets"], {"VOXELPS_SHARE_GPU": "1", "VOXELPS_CU_MASKS": f"0:{NCU // 2},{NCU // 2}:{NCU}"}))
    for name, extra, env in runs:
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, upsample=name != "ranks", damping=10.0 if name != "ranks" else 1.0)] + extra,
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    plain = sorted(f for f in os.listdir(outs["plain"]) if f not in skip)
    names = sorted(f for f in os.listdir(outs["indexed"]) if f not in skip)
    meshes = [f for f in plain if f.endswith("_mesh.ply")]
    assert {"init_mesh.ply", "after_iter_3_mesh.ply"} <= set(meshes) and any(f.startswith("upsample_after_") for f in meshes)
    assert names == sorted(plain + [f[:-len("_mesh.ply")] + "_mesh_indexed.ply" for f in meshes])
    for f in plain:      # the flag changes no other file
        assert filecmp.cmp(outs["plain"] + f, outs["indexed"] + f, shallow=False), f
    for f in meshes:
        head, verts, faces = read_ply_indexed(outs["indexed"] + f[:-len("_mesh.ply")] + "_mesh_indexed.ply")
        xyz = np.stack([verts[k] for k in "xyz"], 1).astype(np.float64)
        a, nf = ascii_mesh(outs["plain"] + f)
        assert len(faces) == nf, f
        p = xyz[faces].reshape(-1, 3)
        assert (np.abs(p - a) <= 1e-5 * np.maximum(np.abs(a), 1e-3) + 1e-9).all(), f      # within %g's six digits
        sizes = (len(verts), len(faces), os.path.getsize(outs["indexed"] + f[:-len("_mesh.ply")] + "_mesh_indexed.ply"), os.path.getsize(outs["plain"] + f))
        print(f"{f}: indexed {sizes[0]} vertices / {sizes[1]} faces / {sizes[2]} B; non-indexed {3 * sizes[1]} vertices / {sizes[3]} B")
    # two ranks: the init state is the single process's bit for bit, so is its indexed file; later files have the slabs' rank-order sums in them
    one = str(tmp_path / "one_small") + "/"; os.makedirs(one)
    r = subprocess.run([EXE, "--config_file", voxelps_config(one), "--indexed-mesh"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert filecmp.cmp(one + "init_mesh_indexed.ply", outs["ranks"] + "init_mesh_indexed.ply", shallow=False)
    for f in os.listdir(one):
        if f.endswith("_mesh_indexed.ply"):
            h1, v1, f1 = read_ply_indexed(one + f)
            h2, v2, f2 = read_ply_indexed(outs["ranks"] + f)
            assert abs(len(f1) - len(f2)) <= 0.01 * len(f1), f


def test_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import resources
    res = resources("mesh.hip", tmp_path)
    ks = {k: v for k, v in res.items() if "k_wmesh_" in k}
    assert len(ks) == 4 and all(v["scratch"] == 0 for v in ks.values()), ks
