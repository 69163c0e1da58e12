"""Baked detail maps on the device (include/psgsdf_bake.h psgsdf_bake_lod, csrc/bake.hip; DESIGN.md "Baked detail maps"): everything against the
yardstick tests/_bake_ref.py on the context's own downloaded state and its own level-of-detail mesh.  The level-of-detail arrays, the texture
coordinates, the face plane and the atlas size must match exactly; the hit voxel on all but 2e-3 of the owned texels (the cap
test_render_gpu.test_restatement_equality_on_an_optimised_state gives the same walk for rays that pass a cell wall within rounding: the yardstick
walks in float64, the device in float32); where the voxel agrees the displacement within 1e-5 * 2 reach (that test's relative bound on the ray
parameter, whose range here is 2 reach), normals within 2^-22 per component, albedo bytes within 1 (clamp and rounding may fall on either side of
a half)."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _bake_ref as bref
import _render_ref as rref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of
from test_mesh_indexed_gpu import EXE, voxelps_config

pytestmark = pytest.mark.gpu
NORMAL_TOL = 2.0 ** -22
VOXEL_SHARE = 2e-3
LOD_KEYS = ("xyz", "normals", "rgb", "faces", "vertex_map", "n_vertices_in", "n_faces_in")
COUNTS = ("n_texels", "n_hits", "n_hits_off_band", "n_buried", "n_misses")


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def assert_matches_yardstick(eng, s, R, tag, reach_vs=None, band=False, **flt):
    """the device's bake for a cell of s voxels against the yardstick on the context's own state; returns (device dict, yardstick dict)"""
    vs = vs_of(eng)
    cell = s * vs
    reach = cell if reach_vs is None else reach_vs * vs
    got = eng.bake_lod(cell, R, None if reach_vs is None else reach, **flt)
    lod = eng.extract_mesh_lod(cell, **flt)
    same_bits(lod, got, LOD_KEYS)                                     # the level-of-detail arrays: extract_mesh_lod's, bit for bit
    v = eng.download_volume()
    dim = [int(x) for x in eng.info().dim]
    band_lin = eng.download_band() if band else None
    exp = bref.bake(v, dim, vs, lod, R, reach, band_lin=band_lin)
    assert (got["width"], got["height"]) == (exp["width"], exp["height"]), tag
    for k in ("uv", "face"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (tag, k)
    own = got["face"] >= 0
    T = int(own.sum())
    differ = own & (got["voxel"] != exp["voxel"])
    share = differ.sum() / max(T, 1)
    same = own & ~differ
    hit = same & (got["voxel"] >= 0)
    d_err = float(np.abs(got["displacement"][hit] - exp["displacement"][hit]).max()) if hit.any() else 0.0
    cmp_n = same & ~exp["on_band"]                                    # (the band's normals and albedo: checked against the renderer's gather by the caller)
    n_err = float(np.abs(got["normal"][cmp_n] - exp["normal"][cmp_n]).max()) if cmp_n.any() else 0.0
    a_err = int(np.abs(got["albedo"][cmp_n].astype(np.int32) - exp["albedo"][cmp_n].astype(np.int32)).max()) if cmp_n.any() else 0
    print(f"{tag} cell {s} vs, R {R}, reach {reach / vs:g} vs {flt}: {len(lod['faces'])} faces, {got['width']} x {got['height']}, {T} texels, {got['n_hits']} hits "
          f"({got['n_hits_off_band']} off the band), {got['n_buried']} buried, {got['n_misses']} misses; another voxel on {int(differ.sum())} texels ({share:.2e}); "
          f"displacement max error {d_err / (2 * reach):.2e} of 2 reach, normals {n_err:.2e}, albedo {a_err}")
    assert share <= VOXEL_SHARE, (tag, share)
    assert d_err <= 1e-5 * reach * 2, (tag, d_err)
    assert n_err <= NORMAL_TOL and a_err <= 1, (tag, n_err, a_err)
    assert (got["displacement"][same & ~hit] == 0).all()
    pad = ~own
    assert (got["voxel"][pad] == -1).all() and not got["albedo"][pad].any() and not got["normal"][pad].any() and not got["displacement"][pad].any()
    # the counts are the sums over the planes
    assert got["n_texels"] == T and got["n_hits"] == int((got["voxel"] >= 0).sum()) and got["n_buried"] + got["n_misses"] == int((own & (got["voxel"] < 0)).sum())
    assert min(got[k] for k in COUNTS) >= 0 and abs(got["n_buried"] - exp["n_buried"]) <= int(differ.sum())
    on = np.isin(got["voxel"], band_lin) & (got["voxel"] >= 0) if band else np.zeros_like(own)
    assert got["n_hits_off_band"] == got["n_hits"] - int(on.sum())
    return got, exp


def plane_engine():
    dim, _, dist, grad, weight, _ = rref.plane_volume()
    v = dict(dist=dist, grad=grad, weight=weight, rgb=np.full((3, len(dist)), 0.5, np.float32))
    return upload(v, tuple(int(x) for x in dim), 0.01)


@pytest.fixture(scope="module")
def pieces(built):
    v, dim, vs = pieces_volume()
    return upload(v, dim, vs)


@pytest.mark.parametrize("s,faces", [(2, 1462), (4, 383)])
def test_plane_without_a_band(built, s, faces):
    """uploaded and never initialised: every hit is off-band; at 4 voxels the face count is odd, so the last block has padding"""
    eng = plane_engine()
    got, _ = assert_matches_yardstick(eng, s, 8, "plane")
    assert len(got["faces"]) == faces
    assert got["n_hits"] == got["n_texels"] == got["n_hits_off_band"] and got["n_buried"] == 0
    assert np.abs(got["displacement"]).max() <= 1e-4 * vs_of(eng)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_five_pieces(pieces, s, R):
    got, _ = assert_matches_yardstick(pieces, s, R, "five pieces")
    assert len(got["faces"]) == {2: 1560, 4: 424}[s]
    assert got["n_hits"] >= got["n_texels"] - int(VOXEL_SHARE * got["n_texels"]) and got["n_hits_off_band"] == got["n_hits"]


def test_five_pieces_largest_component(pieces):
    got, _ = assert_matches_yardstick(pieces, 2, 3, "five pieces", keep_largest=1)
    assert 0 < got["n_faces_in"] < 7204 and got["n_hits"] > 0


def test_five_pieces_short_reach_falls_back(pieces):
    got, exp = assert_matches_yardstick(pieces, 4, 3, "five pieces", reach_vs=0.25)
    assert got["n_texels"] == 3392 and got["n_buried"] > 1000 and got["n_misses"] > 0
    assert abs(got["n_buried"] - 2099) + abs(got["n_misses"] - 24) <= 2 * int(VOXEL_SHARE * 3392)


def scene_engine(model, refine=False):
    sc = synth.make_scene(N=32, F=3, W=64, H=48, model=model)
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.load_scene(sc)
    eng.init_albedo()
    eng.iterate(capi.ALL, 2)
    if refine:
        eng.upsample2x()
    return eng, sc


@pytest.mark.parametrize("model,refine", [("SH1", False), ("LED", False), ("SH1", True)])
def test_synthetic_scene_hits_come_from_the_band(built, model, refine):
    """an optimised state: the hits' normal and albedo are the band's -- what eng.render gathers at the same voxel"""
    eng, sc = scene_engine(model, refine)
    got, exp = assert_matches_yardstick(eng, 2, 4, f"{model}{' refined' if refine else ''}", band=True)
    assert got["n_hits"] > 1000 and got["n_hits_off_band"] < got["n_hits"]
    seen = {}
    for f in range(sc.F):
        r = eng.render(frame=f, channels=capi.R_VOXEL | capi.R_NORMAL | capi.R_ALBEDO)
        m = r["voxel"] >= 0
        for vx, n, a in zip(r["voxel"][m].tolist(), r["normal"][:, m].T, r["albedo"][:, m].T):
            seen[vx] = (n, a)
    band = np.isin(got["voxel"], eng.download_band()) & (got["voxel"] >= 0)
    ys, xs = np.nonzero(band)
    checked = 0
    for y, x in zip(ys.tolist(), xs.tolist()):
        rec = seen.get(int(got["voxel"][y, x]))
        if rec is None:
            continue
        checked += 1
        assert got["normal"][y, x].tobytes() == rec[0].tobytes(), (y, x)
        assert np.abs(got["albedo"][y, x].astype(np.int32) - bref.colour_byte(rec[1]).astype(np.int32)).max() <= 1, (y, x)
    print(f"{model}: {int(band.sum())} band hits, {checked} of them at voxels a keyframe view hits too")
    assert checked > 300


def test_two_calls_same_bits_and_the_other_calls_undisturbed(built):
    eng, sc = scene_engine("SH1")
    vs = vs_of(eng)
    lod0, idx0, rep0 = eng.extract_mesh_lod(2 * vs), eng.extract_mesh_indexed(), eng.render_report()
    a, b = eng.bake_lod(2 * vs, 4), eng.bake_lod(2 * vs, 4)
    same_bits(a, b)
    same_bits(lod0, eng.extract_mesh_lod(2 * vs))
    for x, y in zip(idx0, eng.extract_mesh_indexed()):
        assert np.array_equal(x, y)
    assert rep0 == eng.render_report()
    c = eng.bake_lod(2 * vs, 4, keep_largest=1)
    same_bits(eng.extract_mesh_lod(2 * vs, keep_largest=1), c, LOD_KEYS)


def test_a_bake_between_two_iterations_changes_nothing(built):
    ends = []
    for bake in (False, True):
        sc = synth.make_scene(N=32, F=3, W=64, H=48, model="SH1")
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo()
        eng.iterate(capi.ALL, 1)
        if bake:
            assert eng.bake_lod(2 * vs_of(eng), 4)["n_hits"] > 1000
        eng.iterate(capi.ALL, 1)
        v = eng.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], eng.download_poses(), eng.download_light()))
    for x, y in zip(*ends):
        assert x.tobytes() == y.tobytes()


def test_errors_and_the_empty_mesh(pieces):
    eng = pieces
    vs = vs_of(eng)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):      # PSGSDF_ERR_ARG
        eng.bake_lod(2 * vs, 0)
    for reach in (0.0, float("nan"), -1.0, float("inf")):
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):
            eng.bake_lod(2 * vs, 4, reach)
    for cell in (0.0, float("nan")):                           # what extract_mesh_lod refuses
        with pytest.raises(capi.PsgsdfError, match="rc=-1"):
            eng.bake_lod(cell, 4, vs)
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.bake_lod(2 * vs, 4, keep_largest=-1)
    with pytest.raises(capi.PsgsdfError, match="rc=-3"):      # PSGSDF_ERR_UNSUPPORTED: 1560 faces in 28 blocks a row of 601 texels
        eng.bake_lod(2 * vs, 600)
    got = eng.bake_lod(64 * vs, 4)                             # everything in one cluster: an empty level-of-detail mesh
    assert got["width"] == 0 and got["height"] == 0 and len(got["faces"]) == 0 and len(got["xyz"]) == 0 and got["uv"].shape == (0, 3, 2)
    assert all(got[k] == 0 for k in COUNTS) and all(got[k].size == 0 for k in ("albedo", "normal", "displacement", "voxel", "face"))
    assert got["albedo"].shape == (0, 0, 3) and got["n_vertices_in"] == 3612
    assert_matches_yardstick(eng, 4, 2, "after the refusals")      # the context still works
    sc = synth.make_scene(N=32, F=2, W=64, H=48, model="SH1")
    fresh = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    with pytest.raises(capi.PsgsdfError, match="rc=-4"):      # PSGSDF_ERR_STATE: no volume yet
        fresh.bake_lod(0.1, 4)


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "bake")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e and "bake_lod" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_mesh_bake(built, tmp_path):
    from PIL import Image
    from test_bake_cpu import read_mtl, read_obj
    from test_mesh_indexed_cpu import read_ply_indexed
    outs = {}
    for name, extra in (("lod", ["--mesh-lod", "2"]), ("bake", ["--mesh-lod", "2", "--mesh-bake", "4"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    lod = sorted(f for f in os.listdir(outs["lod"]) if f not in skip)
    meshes = [f[:-len("_mesh_lod.ply")] for f in lod if f.endswith("_mesh_lod.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    new = [m + s for m in meshes for s in ("_mesh_lod.obj", "_mesh_lod.mtl", "_mesh_lod_albedo.png", "_mesh_lod_normal.png")]
    assert sorted(f for f in os.listdir(outs["bake"]) if f not in skip) == sorted(lod + new)      # the only new files
    for f in lod:      # the flag changes no other file
        assert filecmp.cmp(outs["lod"] + f, outs["bake"] + f, shallow=False), f
    for m in meshes:
        base = outs["bake"] + m + "_mesh_lod"
        _, verts, faces = read_ply_indexed(base + ".ply")
        v, vn, vt, f, lib, mtl = read_obj(base + ".obj")
        assert len(v) == len(vn) == len(verts) and len(f) == len(faces) and len(vt) == 3 * len(faces)
        assert np.array_equal(f[:, :, 0], faces + 1) and np.array_equal(f[:, :, 2], faces + 1) and np.array_equal(f[:, :, 1].ravel(), np.arange(3 * len(faces)) + 1)
        assert np.array_equal(v, np.stack([verts[k] for k in "xyz"], 1)) and np.array_equal(vn, np.stack([verts[k] for k in ("nx", "ny", "nz")], 1))
        L = bref.layout(len(faces), 4)
        uv = bref.uv(len(faces), 4).reshape(-1, 2)
        assert np.array_equal(vt[:, 0], uv[:, 0]) and np.array_equal(vt[:, 1], np.float32(1) - uv[:, 1])
        mt = read_mtl(base + ".mtl")
        assert lib == m + "_mesh_lod.mtl" and mtl == mt["newmtl"] and mt["map_Kd"] == m + "_mesh_lod_albedo.png" and mt["norm"] == m + "_mesh_lod_normal.png"
        alb, nrm = (np.asarray(Image.open(base + s).convert("RGB")) for s in ("_albedo.png", "_normal.png"))
        assert alb.shape == nrm.shape == (L["H"], L["W"], 3)
        own = L["face"] >= 0
        n = nrm[own].astype(np.float64) / 127.5 - 1.0
        print(f"{m}: {len(faces)} faces, atlas {L['W']} x {L['H']}, {int(own.sum())} texels, normal length {np.linalg.norm(n, axis=1).min():.3f} .. {np.linalg.norm(n, axis=1).max():.3f}")
        ln = np.linalg.norm(n, axis=1)
        assert abs(np.median(ln) - 1) < 0.02 and ln.max() < 1.02 and alb[own].max() > 0      # unit normals up to the bytes' rounding
        assert not alb[~own].any() and (nrm[~own] == 128).all()                               # padding: albedo 0, normal (0, 0, 0)
