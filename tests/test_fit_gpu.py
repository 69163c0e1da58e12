"""The photometric fit per band row and per vertex of the welded mesh on the device (include/psgsdf_fit.h, csrc/fit.hip; DESIGN.md "Photometric fit per
voxel and vertex"): its sums against psgsdf_energy, its rows against the float64 restatement tests/_fit_ref.py, the vertex attributes against their
definition, no side effects on the optimisation, the error returns, and `voxelPS --mesh-fit`.

Row deviations (check against the restatement).  The deviation of a row is |device - restatement| over the larger of the restatement's value of the row
and its mean over the observed rows: a residual is the difference of two float32 colours of order 0.1 .. 1, so a row whose residuals are near zero has no
relative precision of its own.  Largest deviation measured on the MI355X over the cases below, per model; the bounds are four times that:
    SH1  loss 8.826e-05  sum_r2 7.120e-05      (32^3 refined from 24^3, 3 keyframes: about one observation per row)
    SH2  loss 2.185e-05  sum_r2 1.540e-05      (32^3, 3 keyframes)
    LED  loss 3.216e-05  sum_r2 2.580e-05      (32^3 refined from 24^3, 3 keyframes, 8-bit)
With 65 keyframes (18 observations per row) the same figures are 4e-6 .. 1.1e-5.  What explains them: the float32 projection is good to a few 1e-6 pixels
and the images fall from the object's colour to black within a pixel at the silhouette, so a sample moves by up to a few 1e-6 of full scale -- against
residuals of 0.05.  The sum over the rows, which is what tests/test_parity_gpu.py's E_ps margin (1e-5) is about, is asserted at that margin below.
"""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import _fit_ref as fref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_fit_cpu import assert_header_matches_columns, header_fit_numbers, read_ply_fit
from test_mesh_indexed_cpu import read_ply_indexed
from test_mesh_indexed_gpu import EXE, ulps, voxelps_config

pytestmark = pytest.mark.gpu
ROW_TOL = {"SH1": (4 * 8.826e-05, 4 * 7.120e-05), "SH2": (4 * 2.185e-05, 4 * 1.540e-05), "LED": (4 * 3.216e-05, 4 * 2.580e-05)}      # (loss, sum_r2): four times the measured deviations above
E_PS_MARGIN = 1e-5      # what tests/test_parity_gpu.py allows E_ps against the float32 oracle
SUM_TOL = 2.0 ** -29      # two sums of the same <= 2^24 non-negative doubles in different orders: 2^24 x 2^-53


def settings(model, **kw):
    return capi.default_settings(getattr(capi, model), **kw)


def engine(sc, st=None, u8=False):
    st = st or settings(sc.model)
    eng = capi.load_engine(sc, sc.K, st, 0)
    eng.load_scene(sc, u8=u8)
    return eng


def state_of(eng, sc):
    """everything the restatement needs, downloaded from the context (the images: the scene's own floats; u8 scenes hold byte * scale exactly)"""
    i = eng.info()
    v = eng.download_volume(want_vis=True)
    st = dict(v, band=eng.download_band(), dim=[int(x) for x in i.dim], vs=float(i.voxel_size), origin=[float(x) for x in i.origin], poses=eng.download_poses(),
              light=eng.download_light(), images=sc.images, K=(float(sc.K[0]), float(sc.K[4]), float(sc.K[2]), float(sc.K[5])), model=sc.model_id,
              loss=int(eng._settings.loss), lam=float(eng._settings.lambda_))
    return st


def row_deviation(got, exp, seen):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    if not seen.any():
        return 0.0
    scale = np.maximum(exp, exp[seen].mean(0))
    return float((np.abs(got - exp) / scale)[seen].max())


def check_rows_and_vertices(eng, sc, tag, popcount=True, need_margin=2.0):
    """checks 1, 3 and 4 on the context's current state; returns (band fit, mesh fit, restatement, state)"""
    st = state_of(eng, sc)
    e_ps = eng.energy()[0]
    bf, mf = eng.band_fit(), eng.extract_mesh_fit()
    S = len(st["band"])
    assert S > 500 and S % 256 != 0, (tag, S)      # more than one workgroup, and a tail workgroup
    assert bf["n_obs"].shape == (S,) and bf["loss"].shape == (S,) and bf["sum_r2"].shape == (S, 3)
    assert bf["n_obs"].dtype == np.int32 and bf["loss"].dtype == np.float64 and bf["sum_r2"].dtype == np.float32
    again_b, again_m = eng.band_fit(), eng.extract_mesh_fit()
    assert all(bf[k].tobytes() == again_b[k].tobytes() for k in bf) and all(mf[k].tobytes() == again_m[k].tobytes() for k in mf), tag
    # 1. the sums are the energy's
    rel = abs(bf["loss"].sum() / S - e_ps) / e_ps
    print(f"{tag}: band {S} rows, {int(bf['n_obs'].sum())} observations, E_ps {e_ps:.9g}, |sum(loss) / S - E_ps| / E_ps = {rel:.3e} (bound {SUM_TOL:.3e})")
    assert rel <= SUM_TOL, (tag, rel)
    # 3. every row against the float64 forward model
    exp = fref.band_fit(st, need_margin=need_margin)
    if popcount:
        assert np.array_equal(exp["n_obs"], fref.popcount_below(st["vis"][st["band"]], sc.F)), tag
    assert np.array_equal(bf["n_obs"], exp["n_obs"]), (tag, int((bf["n_obs"] != exp["n_obs"]).sum()))
    seen = exp["n_obs"] > 0
    empty = ~seen
    assert (bf["loss"][empty] == 0).all() and (bf["sum_r2"][empty] == 0).all()
    dl, dr = row_deviation(bf["loss"], exp["loss"], seen), row_deviation(bf["sum_r2"], exp["sum_r2"], seen)
    tl, tr = ROW_TOL[sc.model]
    total = abs(bf["loss"].sum() - exp["loss"].sum()) / exp["loss"].sum()
    print(f"{tag}: projections >= {exp['margin_px']:.2f} px from the border, depth >= {exp['min_depth']:.3f}; largest row deviation loss {dl:.3e} (bound {tl:.3e}), "
          f"sum_r2 {dr:.3e} (bound {tr:.3e}); sum of the rows {total:.3e} (bound {E_PS_MARGIN:.0e})")
    assert dl <= tl and dr <= tr and total <= E_PS_MARGIN, (tag, dl, dr, total)
    # 4. the vertex attributes from the downloaded rows and the restatement's keys
    dim, vs = st["dim"], st["vs"]
    keys, ref_mesh = fref.mesh_keys(st, dim, vs)
    idx = eng.extract_mesh_indexed()
    for k, a in zip(("xyz", "normals", "rgb", "faces"), idx):
        assert mf[k].dtype == a.dtype and np.array_equal(mf[k], a), (tag, k)
    assert len(keys) == len(mf["xyz"]) and np.array_equal(ref_mesh[3], mf["faces"]) and len(keys) > 500, (tag, len(keys), len(mf["xyz"]))
    n, rms, loss = fref.vertex_fit(bf["n_obs"], bf["loss"], bf["sum_r2"], st["band"], keys, dim)
    assert mf["n_obs"].dtype == np.int32 and mf["rms"].dtype == np.float32 and mf["loss"].dtype == np.float32
    assert np.array_equal(mf["n_obs"], n), tag
    u = max(int(ulps(mf["rms"], rms).max()), int(ulps(mf["loss"], loss).max()))
    print(f"{tag}: {len(keys)} vertices, {int((n == 0).sum())} unobserved; rms / loss within {u} ulp")
    assert u <= 1, (tag, u)
    z = n == 0
    assert (mf["rms"][z] == 0).all() and (mf["loss"][z] == 0).all()
    return bf, mf, exp, st, keys


def advanced(sc, u8=False, refine=False, st=None):
    """a state one alternation into the optimisation (every block has moved off its initial value); refine: after the 2x refinement"""
    eng = engine(sc, st, u8)
    eng.init_albedo(); eng.normalize_weights()
    eng.iterate(capi.ALL, 1)
    if refine:
        eng.upsample2x()
        eng.iterate(capi.ALL, 1)
    return eng


# (b) F = 3 and F = 65 (a second visibility word), (c) the three models, (d) float and 8-bit keyframes, (e) a refined state; (a): asserted in every case
CASES = [("SH1", 32, 3, False, False), ("SH2", 24, 65, True, False), ("LED", 24, 65, False, False), ("LED", 32, 3, True, False), ("SH2", 32, 3, False, False),
         ("SH1", 24, 65, True, False), ("SH1", 24, 3, False, True), ("LED", 24, 3, True, True)]


@pytest.mark.parametrize("model,N,F,u8,refine", CASES)
def test_rows_vertices_and_sums(built, model, N, F, u8, refine):
    sc = synth.make_scene(N=N, F=F, W=64, H=48, model=model, u8=u8)
    eng = advanced(sc, u8, refine)
    i = eng.info()
    assert i.vis_words == (F + 63) // 64 and (int(i.dim[0]) == (2 * N if refine else N))
    if refine:
        assert abs(float(i.voxel_size) / float(sc.voxel_size) - 0.5) < 1e-6
    check_rows_and_vertices(eng, sc, f"{model} N={N} F={F}{' u8' if u8 else ''}{' refined' if refine else ''}")


@pytest.mark.parametrize("loss", [capi.L2, capi.CAUCHY, capi.HUBER, capi.TUKEY, capi.TRUNC_L2])
def test_sums_equal_the_energy_for_every_loss(built, loss):
    sc = synth.make_scene(N=32, F=3, W=64, H=48, model="SH1")
    st = settings("SH1", loss=loss, **{"lambda": 0.05})      # (residuals on both sides of the thresholds)
    eng = advanced(sc, st=st)
    S = eng.info().n_band
    bf = eng.band_fit()
    e_ps = eng.energy()[0]
    pop = fref.popcount_below(eng.download_volume(want_vis=True)["vis"][eng.download_band()], sc.F)
    rel = abs(bf["loss"].sum() / S - e_ps) / e_ps
    r = np.sqrt(bf["sum_r2"].astype(np.float64).sum() / (3.0 * bf["n_obs"].sum()))
    print(f"loss {loss}: E_ps {e_ps:.9g}, relative difference of the sums {rel:.3e}; observations {int(bf['n_obs'].sum())}; overall rms {r:.5f}")
    assert np.array_equal(bf["n_obs"], pop) and rel <= SUM_TOL
    if loss == capi.L2:      # the loss IS the squared residual: the two per-row sums agree to float rounding
        assert np.allclose(bf["loss"], bf["sum_r2"].astype(np.float64).sum(1), rtol=1e-5, atol=0)


def test_no_side_effects(built):
    """two contexts on one scene, two times two iterations each; the first is asked for its fit before and in between"""
    sc = synth.make_scene(N=32, F=4, W=64, H=48, model="SH1")
    res = []
    for ask in (True, False):
        eng = engine(sc)
        eng.init_albedo(); eng.normalize_weights()
        recs = []
        for _ in range(2):
            if ask:
                a, b = eng.band_fit(), eng.extract_mesh_fit()
                assert len(a["loss"]) == eng.info().n_band and len(b["faces"]) > 1000
            recs += eng.iterate(capi.ALL, 2)
        res.append(dict(vol=eng.download_volume(), light=eng.download_light(), poses=eng.download_poses(), energy=eng.energy(), mesh=eng.extract_mesh_indexed(), recs=recs))
    a, b = res
    for k in ("dist", "grad", "weight", "rgb"):
        assert a["vol"][k].tobytes() == b["vol"][k].tobytes(), k
    assert a["light"].tobytes() == b["light"].tobytes() and a["poses"].tobytes() == b["poses"].tobytes()
    assert a["energy"] == b["energy"] and a["recs"] == b["recs"]
    for x, y in zip(a["mesh"], b["mesh"]):
        assert np.array_equal(x, y)


def test_unobserved_row_and_vertex_next_to_a_voxel_outside_the_band(built):
    """(f), by editing the volume before the upload.  The engine's band holds a voxel only if some keyframe sees it (k_band_flags), so a voxel whose
    visibility words are cleared is no band row: the vertices of the mesh around it then have an end voxel outside the band.  The row that counts no
    observation is a voxel seen by keyframe 2 only, and keyframe 2's camera is moved sideways until the object is out of its image: the bit is set,
    the projection fails.  Every other row keeps its bit of keyframe 2 and counts the two other keyframes."""
    import copy
    sc = copy.deepcopy(synth.make_scene(N=32, F=3, W=64, H=48, model="SH1"))
    n = 32
    inner = np.zeros((n, n, n), bool); inner[2:-2, 2:-2, 2:-2] = True
    cand = np.nonzero((sc.vis != 0).any(1) & (sc.weight > 0) & inner.reshape(-1))[0]
    order = cand[np.argsort(np.abs(sc.dist[cand]))]
    A = int(order[0])                                                                      # the voxel nearest to the surface: cleared
    B = int(next(x for x in order[1:] if abs(int(x) // (n * n) - A // (n * n)) > 3))       # some planes away: seen by keyframe 2 only
    sc.vis[A] = 0
    sc.vis[B] = np.uint64(4)
    P = sc.poses.reshape(3, 4, 4).copy()
    P[2, :3, 3] += 3.0 * float(sc.extent) * P[2, :3, 0]      # along the camera's x axis: the depth stays, the column moves by more than 100 pixels
    sc.poses = np.ascontiguousarray(P.reshape(3, 16))
    eng = engine(sc)
    eng.init_albedo()
    bf, mf, exp, st, keys = check_rows_and_vertices(eng, sc, "edited volume", popcount=False)
    band = st["band"]
    assert A not in set(band.tolist()) and B in set(band.tolist())
    rB = int(np.searchsorted(band, B))
    assert bf["n_obs"][rB] == 0 and bf["loss"][rB] == 0 and (bf["sum_r2"][rB] == 0).all()
    pop = fref.popcount_below(st["vis"][band], 3)
    assert pop[rB] == 1 and (bf["n_obs"] < pop).sum() > 100 and (bf["n_obs"] > 0).sum() > 100      # bits of keyframe 2 are set and do not count
    typ, lin = keys & 3, keys >> 2
    hi = lin + np.array([1, n, n * n, 0])[typ]
    row = np.full(n ** 3, -1); row[band] = np.arange(len(band))
    outside = (row[lin] < 0) | (row[hi] < 0)
    at_A = (lin == A) | (hi == A)
    assert at_A.any() and outside[at_A].all(), "no mesh vertex has the cleared voxel as an end"
    half = at_A & ((row[lin] >= 0) | (row[hi] >= 0)) & (mf["n_obs"] > 0)
    assert half.any()      # a vertex that lives on its one band end alone
    r = row[np.where(row[lin] >= 0, lin, hi)][half]
    assert np.array_equal(mf["n_obs"][half], bf["n_obs"][r])


def test_overall_rms_falls_with_the_optimisation(built):
    sc = synth.make_scene(N=32, F=6, W=64, H=48, model="SH1")
    x = np.arange(sc.rgb.shape[1])
    sc.rgb = np.clip(sc.rgb * (1.0 + 0.3 * np.sin(0.37 * x))[None, :], 0.02, 0.98).astype(np.float32)      # a perturbed albedo
    eng = engine(sc)
    overall = lambda b: float(np.sqrt(b["sum_r2"].astype(np.float64).sum() / (3.0 * b["n_obs"].sum())))
    before = overall(eng.band_fit())
    eng.optimize(capi.ALL)
    after = overall(eng.band_fit())
    mf = eng.extract_mesh_fit()
    print(f"overall rms residual: {before:.5f} with the perturbed albedo, {after:.5f} after optimize; vertices: median rms {np.median(mf['rms']):.5f}, median observations {np.median(mf['n_obs'])}")
    assert after < before


def test_errors_and_the_empty_mesh(built):
    sc = synth.make_scene(N=24, F=3, W=64, H=48, model="SH1")
    eng = capi.load_engine(sc, sc.K, settings("SH1"), 0)
    for call in (eng.band_fit, eng.extract_mesh_fit):      # before a volume
        with pytest.raises(capi.PsgsdfError, match="rc=-4"):
            call()
    eng.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)
    eng.set_keyframes(sc.frame_idx, sc.images, sc.poses)
    for call in (eng.band_fit, eng.extract_mesh_fit):      # a volume and keyframes, no band
        with pytest.raises(capi.PsgsdfError, match="rc=-4"):
            call()
    assert len(eng.extract_mesh_indexed()[3]) > 500      # (which psgsdf_extract_mesh_indexed does not need)
    eng.init()
    assert len(eng.extract_mesh_fit()["faces"]) > 500
    # an empty mesh on a context with a band: no voxel carries a weight, so no cell is valid
    eng = capi.load_engine(sc, sc.K, settings("SH1"), 0)
    eng.upload_volume(sc.dist, sc.grad, np.zeros_like(sc.weight), sc.rgb, sc.vis, sc.vis_words)
    eng.set_keyframes(sc.frame_idx, sc.images, sc.poses)
    eng.init()
    assert eng.info().n_band > 500 and len(eng.band_fit()["loss"]) == eng.info().n_band
    m = eng.extract_mesh_fit()
    assert all(len(m[k]) == 0 for k in m) and m["n_obs"].dtype == np.int32 and m["rms"].dtype == np.float32


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "fit", N=32, F=3)
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 500 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_mesh_fit(built, tmp_path):
    outs = {}
    for name, extra in (("indexed", ["--indexed-mesh"]), ("fit", ["--indexed-mesh", "--mesh-fit"])):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", voxelps_config(out, **{"max iter": 4})] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out
    skip = ("config.json", "saved_config.json")
    base = sorted(f for f in os.listdir(outs["indexed"]) if f not in skip)
    meshes = [f[:-len("_mesh.ply")] for f in base if f.endswith("_mesh.ply")]
    assert "init" in meshes and "after_iter_3" in meshes
    assert sorted(f for f in os.listdir(outs["fit"]) if f not in skip) == sorted(base + [m + "_mesh_fit.ply" for m in meshes])      # the only new files
    for f in base:      # the flag changes no other file
        assert filecmp.cmp(outs["indexed"] + f, outs["fit"] + f, shallow=False), f
    observed = 0
    for m in meshes:
        head, verts, faces = read_ply_fit(outs["fit"] + m + "_mesh_fit.ply")
        ihead, iverts, ifaces = read_ply_indexed(outs["fit"] + m + "_mesh_indexed.ply")
        assert np.array_equal(faces, ifaces), m
        for k in iverts.dtype.names:
            assert verts[k].tobytes() == iverts[k].tobytes(), (m, k)
        assert [h for h in head if not h.startswith(("comment fit", "property"))] == [h for h in ihead if not h.startswith("property")]
        assert_header_matches_columns(head, verts)
        rms, n = header_fit_numbers(head)
        print(f"{m}: {len(verts)} vertices, {n} observations, overall rms {rms:.5f}")
        unseen = verts["n_obs"] == 0
        assert (verts["quality"][unseen] == 0).all() and (verts["loss"][unseen] == 0).all() and (verts["quality"][~unseen] > 0).all()
        observed += n > 0
    assert header_fit_numbers(read_ply_fit(outs["fit"] + "after_iter_3_mesh_fit.ply")[0])[1] > 1000 and observed >= len(meshes) - 1      # (init: written before the band exists)
    r = subprocess.run([EXE, "--config_file", outs["fit"] + "config.json", "--gpus", "2", "--mesh-fit"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--mesh-fit needs a single process" in r.stderr
