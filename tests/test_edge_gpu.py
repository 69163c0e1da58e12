"""Edge cases through the C ABI against the oracle: more than 64 keyframes (two visibility words), one keyframe, a band of a
handful of voxels, an empty band, non-default robust losses on an LED scene, a keyframe subset of the fused sequence."""
import copy

import numpy as np
import pytest

from psgradientsdf_amd import capi, synth

pytestmark = pytest.mark.gpu


def pair(sc, st, solver="eigen"):
    """engine and oracle on one scene; solver = "eigen": both solve the light / pose blocks as the reference does (one global float Jacobi-PCG:
    psgsdf_set_frame_solver(1) / the oracle's solver_mode 1), "ldlt": the engine as shipped against the oracle's direct solves"""
    from oracle import oracle
    eng = capi.load_engine(sc, sc.K, st, 0); orc = oracle.Oracle(sc, sc.K, st, threads=4, solver_mode=1 if solver == "eigen" else 0)
    if solver == "eigen":
        eng.set_frame_solver(1)
    for api in (eng, orc):
        api.load_scene(sc)
    return eng, orc


def compare(eng, orc, sc, iters=2, tol=2e-4, flags=capi.ALL, margins=None, max_vs=1e-4):
    """round 6: EVERY band voxel within the north star's 1e-4 voxel (round 5 asserted q999 <= 2e-4 and max <= 1e-2), what was achieved on record"""
    from conftest import sdf_margin
    for api in (eng, orc):
        api.init_albedo(); api.normalize_weights()
    re_, ro = eng.iterate(flags, iters), orc.iterate(flags, iters)
    band = eng.download_band()
    assert np.array_equal(band, orc.download_band())
    e_rel = max(abs(a["e_total"] - b["e_total"]) / (abs(b["e_total"]) + 1e-300) for a, b in zip(re_, ro))
    for a, b in zip(re_, ro):
        assert abs(a["e_total"] - b["e_total"]) <= tol * abs(b["e_total"]) + 1e-12, (a["e_total"], b["e_total"])
    if len(band):
        ve, vo = eng.download_volume(), orc.download_volume()
        m = sdf_margin(ve["dist"], vo["dist"], band, float(sc.voxel_size))
        if margins:
            margins(sdf=m, e_total_rel=float(e_rel), rgb=float(np.abs(ve["rgb"][:, band] - vo["rgb"][:, band]).max()), tolerance={"max_vs": max_vs, "e_total_rel": tol})
        assert m["q999_vs"] <= 1e-4 and m["max_vs"] <= max_vs, m
    return re_


def test_two_visibility_words(built, margins):
    sc = synth.make_scene(N=32, F=70, W=96, H=72, model="SH1")
    assert sc.vis_words == 2
    eng, orc = pair(sc, capi.default_settings(capi.SH1))
    assert eng.info().n_band == orc.info().n_band > 500
    compare(eng, orc, sc, margins=margins)


def test_single_keyframe(built, margins):
    sc = synth.make_scene(N=32, F=1, W=128, H=96, model="SH1")
    eng, orc = pair(sc, capi.default_settings(capi.SH1))
    compare(eng, orc, sc, iters=1, margins=margins)


def test_keyframe_subset_of_the_sequence(built, margins):
    """visibility is recorded per SEQUENCE frame; the optimiser uses a subset as keyframes (Optimizer.cpp:30-47 select_vis)"""
    sc = synth.make_scene(N=32, F=9, W=128, H=96, model="SH1")
    keep = np.array([1, 4, 7], np.int32)
    sub = copy.copy(sc)
    sub.F = len(keep); sub.frame_idx = keep.copy(); sub.images = np.ascontiguousarray(sc.images[keep]); sub.poses = np.ascontiguousarray(sc.poses[keep])
    if hasattr(sc, "light_gt") and np.ndim(sc.light_gt) == 2:
        sub.light_gt = sc.light_gt[keep]
    eng, orc = pair(sub, capi.default_settings(capi.SH1))
    assert eng.info().n_frames == 3
    compare(eng, orc, sub, margins=margins)


def test_tiny_and_empty_band(built, margins):
    sc = synth.make_scene(N=24, F=3, W=96, H=72, model="SH1")
    # tiny: keep the visibility of a handful of voxels only
    tiny = copy.copy(sc); tiny.vis = sc.vis.copy()
    near = np.nonzero((np.abs(sc.dist) <= np.sqrt(3) * sc.voxel_size) & (sc.vis != 0).any(axis=1))[0]
    keep = near[:: max(1, len(near) // 5)][:5]
    mask = np.ones(len(sc.dist), bool); mask[keep] = False
    tiny.vis[mask] = 0
    eng, orc = pair(tiny, capi.default_settings(capi.SH1))
    assert eng.info().n_band == orc.info().n_band == len(keep)
    # five isolated voxels cannot determine 4 light + 6 pose unknowns per frame (those blocks are singular to rounding): compare the
    # per-voxel blocks tightly, and only require the full iteration to run
    compare(eng, orc, tiny, iters=1, tol=5e-4, flags=capi.ALBEDO | capi.DIST, margins=margins)
    r = eng.iterate(capi.ALL, 1)
    assert len(r) == 1 and np.isfinite(r[0]["e_total"])
    # empty: nothing was ever seen
    empty = copy.copy(sc); empty.vis = np.zeros_like(sc.vis)
    eng = capi.load_engine(empty, empty.K, capi.default_settings(capi.SH1), 0); eng.load_scene(empty)
    assert eng.info().n_band == 0
    eng.init_albedo()
    recs = eng.iterate(capi.ALL, 1)          # must not crash or hang; energies of an empty band are 0
    assert len(recs) == 1 and recs[0]["cg_iters"] == 0


LOSSES = {0: "L2", 2: "Huber", 3: "Tukey", 4: "truncated L2"}      # (1 = Cauchy: every shipped config, every other test)


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("SH2", capi.SH2), ("LED", capi.LED)])
@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_other_robust_losses(built, margins, loss, name, mid):
    """computeWeight / computeLoss (Optimizer.cpp:140-186) for L2, Huber, Tukey and truncated L2 on ALL three shading models (round 5: LED only): the
    run-time-loss instances of every sweep (the compiled-in one is Cauchy), two iterations, every band voxel.  Twelve keyframes: enough for the reference's
    SH2 light solve to converge (tests/golden/make_golden.py)."""
    sc = synth.make_scene(N=32, F=12, W=128, H=96, model=name)
    st = capi.default_settings(mid, loss=loss)
    eng, orc = pair(sc, st)
    compare(eng, orc, sc, iters=2, tol=2e-4, margins=margins)


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("SH2", capi.SH2), ("LED", capi.LED)])
def test_without_reference_quirks(built, margins, name, mid):
    """ref_quirks = 0: the LED neighbour-column sign (B6) and the 'skip the update unless CG reports Success' gates (B8; LED poses) are off"""
    sc = synth.make_scene(N=32, F=12 if mid == capi.SH2 else 5, W=128, H=96, model=name)
    st = capi.default_settings(mid, ref_quirks=0)
    if mid == capi.LED:
        st.reg_weight_n, st.reg_weight_l, st.damping = 0.1, 5.0, 3.0      # config_basket_LED.json
    eng, orc = pair(sc, st)
    compare(eng, orc, sc, iters=2, tol=2e-4, margins=margins)


def test_laplacian_and_upsample_schedule(built):
    """psgsdf_optimize with the 2x refinement at iteration 5 and the Laplacian schedule (PsOptimizer.cpp:386-413)"""
    sc = synth.make_scene(N=24, F=5, W=128, H=96, model="SH1")
    st = capi.default_settings(capi.SH1, upsample=1, max_it=8, conv_threshold=0.0)
    eng, orc = pair(sc, st)
    re_, ce = eng.optimize(capi.ALL); ro, co = orc.optimize(capi.ALL)
    assert len(re_) == len(ro) and ce == co
    assert [r["upsampled"] for r in re_] == [r["upsampled"] for r in ro]
    assert [(r["converged"], r["diverged"]) for r in re_] == [(r["converged"], r["diverged"]) for r in ro]
    for a, b in zip(re_, ro):
        assert abs(a["e_total"] - b["e_total"]) <= 2e-3 * abs(b["e_total"]), (a["e_total"], b["e_total"])
    assert eng.info().n_band == orc.info().n_band


def test_zero_right_hand_side_of_the_distance_system(built):
    """black keyframes, zero albedo, no regularisers: every residual and every Jacobian entry is zero, so the distance system is 0 x = 0.
    Eigen's CG returns x = 0 at once (|b| = 0: zero iterations, Success) and the update is applied as a no-op that accepts every voxel.
    The persistent solve learns |b|^2 only with the sums of its first pass -- it must come to the same end, not divide 0 by 0 into the state."""
    sc = synth.make_scene(N=32, F=4, W=128, H=96, model="SH1")
    sc = copy.copy(sc); sc.images = np.zeros_like(sc.images)
    st = capi.default_settings(capi.SH1, reg_weight_n=0.0, reg_weight_l=0.0)
    eng, orc = pair(sc, st)
    for api in (eng, orc):
        api.init_albedo()                                 # mean of black pixels: albedo 0
    d0 = eng.download_volume()["dist"].copy()
    se, so = eng.step(capi.DIST), orc.step(capi.DIST)
    assert se["cg_iters"] == so["cg_iters"] == 0 and se["cg_converged"] == so["cg_converged"] == 1
    assert se["applied"] == so["applied"] and se["n_accepted"] == so["n_accepted"] == eng.info().n_band
    v = eng.download_volume()
    assert np.array_equal(v["dist"], d0) and np.isfinite(v["grad"]).all()
    assert np.array_equal(v["dist"], orc.download_volume()["dist"])


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("LED", capi.LED)])
def test_cg_iteration_cap(built, name, mid):
    """the distance solve cut off after 3 CG iterations (`cg_max_it`): not converged.  With the reference's quirk B8 the SH optimiser then SKIPS
    the distance update (PsOptimizer.cpp:168-170) while the LED optimiser applies it anyway (LedOptimizer.cpp:195) -- the rule the persistent
    solve kernel applies itself in its epilogue."""
    sc = synth.make_scene(N=32, F=6, W=128, H=96, model=name)
    st = capi.default_settings(mid, cg_max_it=3)
    eng, orc = pair(sc, st)
    for api in (eng, orc):
        api.init_albedo(); api.normalize_weights()
    d0 = eng.download_volume()["dist"].copy()
    se, so = eng.step(capi.DIST), orc.step(capi.DIST)
    assert se["cg_iters"] == so["cg_iters"] == 3 and se["cg_converged"] == so["cg_converged"] == 0
    assert se["applied"] == so["applied"] == (1 if mid == capi.LED else 0)
    band = eng.download_band(); vs = float(sc.voxel_size)
    ve, vo = eng.download_volume(), orc.download_volume()
    if mid == capi.LED:
        assert se["n_accepted"] == so["n_accepted"] > 0
        assert np.abs(ve["dist"][band] - vo["dist"][band]).max() <= 1e-4 * vs and not np.array_equal(ve["dist"], d0)
    else:
        assert np.array_equal(ve["dist"], d0) and np.array_equal(vo["dist"], d0)      # nothing applied


def test_persistent_solve_gives_up_instead_of_hanging(built):
    """fault injection: one workgroup of the persistent distance-step kernel stops publishing in pass 2.  Every wait inside the kernel is
    bounded: the others raise the abort flag, the kernel ends, the host gets PSGSDF_ERR_DEVICE (a message, not a hang) -- and the context
    keeps working afterwards."""
    import time
    sc = synth.make_scene(N=48, F=6, W=160, H=120, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(capi.SH1), 0); eng.load_scene(sc)
    eng.init_albedo(); eng.normalize_weights()
    eng.debug_time_pcg_solve(passes=4, reps=1)                     # the kernel applies to this band
    t0 = time.time()
    with pytest.raises(RuntimeError, match="gave up waiting"):
        eng.debug_time_pcg_solve(passes=-7, reps=1)
    assert time.time() - t0 < 60
    recs = eng.iterate(capi.ALL, 2)                                # the next distance step resets the abort flag
    assert all(np.isfinite(r["e_total"]) for r in recs) and recs[1]["e_total"] < recs[0]["e_total"] * 1.01
    assert recs[0]["cg_iters"] > 3


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("LED", capi.LED)])
def test_persistent_solve_falls_back_to_the_per_pass_kernels(built, name, mid, monkeypatch, capfd):
    """A persistent distance solve that cannot get all its workgroups co-resident (another process holding CUs; here: fault injection into the
    2nd solve of the context, PSGSDF_FAULT_SOLVE) must not fail the optimisation: the step is re-run on the per-pass kernels, once logged, and
    the results are those of a context that ran the per-pass kernels all along (bit for bit) -- and the oracle's, to the usual tolerance."""
    sc = synth.make_scene(N=40, F=6, W=160, H=120, model=name)
    st = capi.default_settings(mid)
    monkeypatch.setenv("PSGSDF_FAULT_SOLVE", "2")
    eng = capi.load_engine(sc, sc.K, st, 0, dev=True)      # (fault injection exists in the development build only)
    prod = capi.load_engine(sc, sc.K, st, 0)
    tp, td = prod.get_tuning(), eng.get_tuning()
    assert td["env"]["PSGSDF_FAULT_SOLVE"] == "2" and td["effective"]["fault_solve"] == 2 and "dev" in td["build"]
    assert tp["ignored_dev_only"] == {"PSGSDF_FAULT_SOLVE": "2"} and tp["effective"]["fault_solve"] == 0 and "PSGSDF_FAULT_SOLVE" not in tp["env"]      # the product library says it ignores it
    prod.close()
    monkeypatch.delenv("PSGSDF_FAULT_SOLVE"); monkeypatch.setenv("PSGSDF_PCG_PERSIST", "0")
    ref = capi.load_engine(sc, sc.K, st, 0)
    assert ref.get_tuning()["env"] == {"PSGSDF_PCG_PERSIST": "0"} and ref.get_tuning()["effective"]["pcg_persist"] == 0
    monkeypatch.delenv("PSGSDF_PCG_PERSIST")
    from oracle import oracle
    orc = oracle.Oracle(sc, sc.K, st)
    for api in (eng, ref, orc):
        api.load_scene(sc); api.init_albedo(); api.normalize_weights()
    r_e, r_r, r_o = eng.iterate(capi.ALL, 3), ref.iterate(capi.ALL, 3), orc.iterate(capi.ALL, 3)
    assert eng.debug_sync_stats()["persist_fallbacks"] == 1 and ref.debug_sync_stats()["persist_fallbacks"] == 0
    assert "per-pass kernels" in capfd.readouterr().err
    # the solve that fell back and every solve of `ref` ran the per-pass kernels (Eigen's recurrences in float), the other solves of `eng` the
    # pipelined ones in double: rounding-level differences only
    assert np.allclose([r["e_total"] for r in r_e], [r["e_total"] for r in r_r], rtol=2e-6) and all(abs(a["cg_iters"] - b["cg_iters"]) <= 1 for a, b in zip(r_e, r_r))
    band = eng.download_band(); vs = float(sc.voxel_size)
    ve, vr, vo = eng.download_volume(), ref.download_volume(), orc.download_volume()
    assert np.abs(ve["dist"][band] - vr["dist"][band]).max() <= 5e-5 * vs and np.abs(ve["rgb"][:, band] - vr["rgb"][:, band]).max() <= 5e-5 and np.abs(eng.download_poses() - ref.download_poses()).max() <= 1e-6
    d = np.abs(ve["dist"][band] - vo["dist"][band]) / vs
    assert d.max() <= 1e-4, (np.quantile(d, 0.999), d.max())      # three iterations, no refinement: every band voxel (tests/test_parity_gpu.py OPT_MAX_VS)
    for a, b in zip(r_e, r_o):
        assert abs(a["e_total"] - b["e_total"]) <= 2e-4 * abs(b["e_total"])


def test_tuning_report_follows_the_knob_table(built, monkeypatch):
    """psgsdf_get_tuning on contexts that are only created (no volume, no kernel): a knob the report used to leave out (PSGSDF_AREG_DEVICE), the two
    variables that share one member (PSGSDF_XCD_MAP first, PSGSDF_XCD_STRIPE on top), the one variable that sets two members (PSGSDF_FM_SOLVE), and
    a refused CU mask (lo < hi is the table's rule; hi <= the device's CUs is psgsdf_create's)."""
    grid = capi.GridDesc(); grid.dim[:] = [8, 8, 8]; grid.voxel_size = 0.01
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)

    def tuning():
        eng = capi.load_engine(grid, K, capi.default_settings(capi.SH1), 0)
        t = eng.get_tuning(); eng.close()
        return t
    t = tuning()
    assert t["env"] == {} and t["ignored_dev_only"] == {} and t["effective"]["areg_device"] == 1
    assert t["effective"]["xcd_map"] == 163 and t["effective"]["fm_solve"] == 1 and t["effective"]["fm_solve_led"] == 1 and t["effective"]["cu_mask"] == [-1, -1]
    monkeypatch.setenv("PSGSDF_AREG_DEVICE", "0")
    t = tuning()
    assert t["env"] == {"PSGSDF_AREG_DEVICE": "0"} and t["effective"]["areg_device"] == 0
    monkeypatch.delenv("PSGSDF_AREG_DEVICE")
    monkeypatch.setenv("PSGSDF_XCD_MAP", "3"); monkeypatch.setenv("PSGSDF_XCD_STRIPE", "2")
    t = tuning()
    assert t["effective"]["xcd_map"] == 515 and t["env"] == {"PSGSDF_XCD_MAP": "3", "PSGSDF_XCD_STRIPE": "2"}
    monkeypatch.delenv("PSGSDF_XCD_MAP"); monkeypatch.delenv("PSGSDF_XCD_STRIPE")
    monkeypatch.setenv("PSGSDF_FM_SOLVE", "2")
    t = tuning()
    assert t["effective"]["fm_solve"] == 1 and t["effective"]["fm_solve_led"] == 0
    monkeypatch.delenv("PSGSDF_FM_SOLVE")
    monkeypatch.setenv("PSGSDF_CU_MASK", "8:8")
    with pytest.raises(capi.PsgsdfError, match=r"create failed rc=-1\b"):      # PSGSDF_ERR_ARG
        tuning()


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("LED", capi.LED)])
def test_exact_state_callback_between_speculative_iterations(built, name, mid, monkeypatch):
    """psgsdf_set_on_iter_period(3): `on_iter` -- the callback voxelPS writes its meshes from -- is invoked for every 3rd iteration only and must see exactly
    the state of that iteration, although the iterations in between are closed speculatively (next iteration's albedo / light already applied when the stop
    decision arrives).  Against a run that closes every iteration first (PSGSDF_SPECULATE=0, period 1): same records, same state at every due callback,
    same final state; the passive observer sees every record."""
    import hashlib
    sc = synth.make_scene(N=40, F=6, W=160, H=120, model=name)
    st = capi.default_settings(mid, max_it=9, conv_threshold=0.0)

    def run(period, speculate):
        monkeypatch.setenv("PSGSDF_SPECULATE", "1" if speculate else "0")
        eng = capi.load_engine(sc, sc.K, st, 0); eng.load_scene(sc)
        seen, observed = {}, []

        def on_iter(done, rec):
            v = eng.download_volume()
            seen[done] = (hashlib.sha1(v["dist"].tobytes()).hexdigest(), hashlib.sha1(v["rgb"].tobytes()).hexdigest(), hashlib.sha1(eng.download_light().tobytes()).hexdigest())
            return False
        eng.set_on_iter_period(period)
        eng.set_record_observer(lambda done, rec: observed.append(done) and False)
        recs, _ = eng.optimize(capi.ALL, on_iter=on_iter)
        v = eng.download_volume()
        stats = eng.debug_sync_stats()
        return recs, seen, observed, (hashlib.sha1(v["dist"].tobytes()).hexdigest(), hashlib.sha1(v["rgb"].tobytes()).hexdigest()), stats
    r0, seen0, obs0, fin0, st0 = run(1, False)
    r3, seen3, obs3, fin3, st3 = run(3, True)
    assert len(r0) == len(r3) >= 4 and [r["e_total"] for r in r0] == [r["e_total"] for r in r3] and [r["e_after"] for r in r0] == [r["e_after"] for r in r3]
    assert sorted(seen3) == [d for d in sorted(seen0) if d % 3 == 0] and len(seen3) >= 1
    assert all(seen3[d] == seen0[d] for d in seen3)
    assert fin0 == fin3 and obs0 == obs3 == sorted(seen0)
    assert st0["speculative_starts"] == 0 and st3["speculative_starts"] >= 2


@pytest.mark.parametrize("name,mid", [("SH1", capi.SH1), ("LED", capi.LED)])
def test_speculative_start_with_block_subsets(built, name, mid, monkeypatch):
    """the speculative start of an iteration (albedo / light with undo) under every shape the ablation flags of voxelPS can give the loop: only undoable
    blocks (the window is closed at the end of the iteration), an undoable block followed directly by the distance block, no undoable block at all --
    records and final state bit for bit those of the loop that closes every iteration first (PSGSDF_SPECULATE=0)."""
    sc = synth.make_scene(N=32, F=5, W=128, H=96, model=name)
    st = capi.default_settings(mid, max_it=6, conv_threshold=0.0)
    for flags in (capi.ALBEDO, capi.LIGHT, capi.ALBEDO | capi.LIGHT, capi.LIGHT | capi.DIST, capi.ALBEDO | capi.POSE, capi.DIST | capi.POSE, capi.ALBEDO | capi.DIST):
        out = []
        for spec in ("1", "0"):
            monkeypatch.setenv("PSGSDF_SPECULATE", spec)
            eng = capi.load_engine(sc, sc.K, st, 0); eng.load_scene(sc)
            recs, conv = eng.optimize(flags)
            v = eng.download_volume()
            out.append(([(r["e_total"], tuple(np.nan_to_num(r["e_after"], nan=-1.0)), r["cg_iters"], r["converged"], r["diverged"]) for r in recs], conv,
                        v["dist"].tobytes(), v["rgb"].tobytes(), eng.download_poses().tobytes(), eng.download_light().tobytes(), eng.debug_sync_stats()["speculative_starts"]))
            eng.close()
        assert out[0][:6] == out[1][:6], flags
        assert out[1][6] == 0

def _cropped(sc, x0, y0, W2, H2):
    """the same scene seen through a window of the keyframes: principal point shifted, everything outside the window is outside the image"""
    c = copy.copy(sc)
    c.images = np.ascontiguousarray(sc.images[:, y0:y0 + H2, x0:x0 + W2])
    if getattr(sc, "images_u8", None) is not None:
        c.images_u8 = np.ascontiguousarray(sc.images_u8[:, y0:y0 + H2, x0:x0 + W2])
    K = np.array(sc.K, np.float32).copy(); K[2] -= x0; K[5] -= y0
    c.K = K; c.W, c.H = W2, H2
    return c


def _border_observations(sc):
    """observations of the initial state whose bilinear cell hangs over the image's last row / column (Auxilary.h:55-57: nearest sample there)"""
    vs = float(sc.voxel_size)
    band = np.nonzero((np.abs(sc.dist) <= np.sqrt(3.0) * vs) & (sc.vis != 0).any(axis=1))[0]
    N = sc.dim.astype(np.int64)
    ix, iy, iz = band % N[0], (band // N[0]) % N[1], band // (N[0] * N[1])
    origin = sc.shift.astype(np.float64) - 0.5 * vs * (N - 1) if not hasattr(sc, "origin") else np.asarray(sc.origin, np.float64)
    xv = origin[None, :] + vs * np.stack([ix, iy, iz], 1)
    g = sc.grad[:, band].T.astype(np.float64); g /= np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    xs = xv - sc.dist[band, None].astype(np.float64) * g
    fx, cx, fy, cy = [float(sc.K[i]) for i in (0, 2, 4, 5)]
    n_border = n_in = 0
    for f in range(sc.F):
        P = sc.poses[f].reshape(4, 4).astype(np.float64)
        p = (xs - P[:3, 3]) @ P[:3, :3]
        vis = ((sc.vis[band, int(sc.frame_idx[f]) // 64] >> np.uint64(int(sc.frame_idx[f]) % 64)) & np.uint64(1)).astype(bool)
        m, n = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
        inside = vis & (m >= 0) & (m < sc.W) & (n >= 0) & (n < sc.H)
        n_in += int(inside.sum())
        n_border += int((inside & ((np.floor(m) + 1 >= sc.W) | (np.floor(n) + 1 >= sc.H))).sum())
    return n_border, n_in


@pytest.mark.parametrize("name,u8", [("SH1", False), ("SH1", True), ("SH2", False), ("LED", False)])
def test_observations_on_the_image_border(built, margins, name, u8):
    """The object hangs over the right and lower edge of every keyframe: observations leave the image (skipped), and some land in its LAST row / column,
    where the reference samples the nearest pixel and takes one-sided differences (Auxilary.h:55-57, 90-121).  Round 6's frame-major sweeps serve the
    nearest pixel from the clamped cell's taps and evaluate the one-sided differences behind their observation pipeline (device_common.h taps_colour,
    fm_for_each_obs): all four blocks against the oracle."""
    full = synth.make_scene(N=40, F=12 if name == "SH2" else 6, W=160, H=120, model=name, u8=u8)      # (SH2: the reference's light solve needs ~10 keyframes to converge, profiles/r06_notes.md section 1)
    sc = _cropped(full, 0, 0, 100, 78)     # the sphere projects to a disc of ~30 px around (79.5, 59.5): the window cuts its right and lower rim
    nb, nin = _border_observations(sc)
    assert nb >= 20 and nin > 4 * nb, (nb, nin)
    st = capi.default_settings(sc.model_id)
    from oracle import oracle
    eng = capi.load_engine(sc, sc.K, st, 0); orc = oracle.Oracle(sc, sc.K, st, threads=4, solver_mode=1)
    eng.set_frame_solver(1)
    for api in (eng, orc):
        api.load_scene(sc, u8=u8)
    compare(eng, orc, sc, iters=2, margins=margins)
    # (SH2: the poses inherit the light step's 1e-4 .. 1e-3 -- cond ~2e4 blocks in float, whoever solves them)
    assert np.abs(eng.download_poses() - orc.download_poses()).max() <= (2e-4 if name == "SH2" else 1e-5)
