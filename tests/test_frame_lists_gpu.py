"""The frame-major sweeps (k_sweep_light, k_sweep_pose) and the per-keyframe observation lists (k_obs_count, host prefix sum, k_obs_fill) at the edges
of their partition, against the oracle.

Every other scene of the suite comes from synth.make_scene unchanged: every keyframe sees about the same third of the band, no list is empty, none ends
on a wavefront (64), workgroup (256), chunk (256 x rows) or fill-block (2048) boundary, none is much shorter than the longest.  tests/_frame_lists.py
`skew` edits the visibility so that they do:

  A  lists of 0 / 1023 / 1024 / 1025 observations (the default chunk at this size is 1024), SH1 (float and RGBA8 keyframes), SH2, LED; the normal
     equations also at PSGSDF_FM_ROWS = 7 (an odd chunk of 1792) and 64 (gridDim.x == 1: a frame's only workgroup is its last arriver);
  B  lists of 1 / 63 / 64 / 65 / 255 / 256 / 257 / 0 observations, one list from the band's first rows and one from its last rows only; and the same
     scene with ONE keyframe that sees anything (obs_max from a single frame, every other frame's workgroups empty);
  C  the boundary between the two visibility words: frames 63 and 65 empty, 64 and 69 on the chunk boundary;
  D  lists rebuilt by the 2x refinement.

The per-frame normal equations are held to the bar of tests/test_parity_gpu.py test_normal_equations (2e-5), but relative to EACH FRAME's largest oracle
entry: a frame with one observation is invisible in a norm over all frames.  A frame without observations is exactly zero on both sides, and its pose
(SH models: and light) row keeps its bits through the iterations.  tests/test_frame_lists_cpu.py pins what the state tolerances rest on.

Not covered here: a thread that walks the full 64 observations (a keyframe with more than 16 128 observations needs a grid of about 110^3; the 128^3 /
256^3 runs of tests/test_fullsize_gpu.py and the benchmark run about 21 per thread), and the multi-rank gather (k_frame_gather).
"""
import numpy as np
import pytest

import _frame_lists as fl
from conftest import sdf_margin
from psgradientsdf_amd import capi

pytestmark = pytest.mark.gpu

SOLVERS = ["eigen", "ldlt"]      # tests/test_parity_gpu.py SOLVERS: the reference's global float PCG on both sides (primary) / direct solves on both sides


def pair(case, solver="eigen"):
    """engine and oracle on a case's scene, paired as tests/test_edge_gpu.py pair"""
    from oracle import oracle
    sc, u8, counts, st = fl.scene(case)
    eng = capi.load_engine(sc, sc.K, st, 0); orc = oracle.Oracle(sc, sc.K, st, threads=4, solver_mode=1 if solver == "eigen" else 0)
    if solver == "eigen":
        eng.set_frame_solver(1)
    for api in (eng, orc):
        api.load_scene(sc, u8=u8)
    return sc, counts, eng, orc


_oracle_systems = {}


def oracle_systems(case):
    """the oracle's band and per-frame normal equations of a case's initial state: computed once, shared by every launch shape"""
    if case not in _oracle_systems:
        from oracle import oracle
        sc, u8, counts, st = fl.scene(case)
        orc = oracle.Oracle(sc, sc.K, st, threads=4); orc.load_scene(sc, u8=u8)
        orc.init_albedo(); orc.normalize_weights()
        _oracle_systems[case] = (orc.download_band(), {blk: orc.debug_frame_system(blk) for blk in (capi.LIGHT, capi.POSE)})
    return _oracle_systems[case]


def set_rows(monkeypatch, rows):
    if rows is None:
        monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    else:
        monkeypatch.setenv("PSGSDF_FM_ROWS", str(rows))      # (fm_rows reads it at every launch)


def check_normal_equations(case, eng, margins, tag=""):
    """debug_frame_system(LIGHT / POSE) of the engine's initial state against the oracle's, frame by frame"""
    sc, u8, counts, st = fl.scene(case)
    band_o, systems = oracle_systems(case)
    eng.init_albedo(); eng.normalize_weights()
    band = eng.download_band()
    assert np.array_equal(band, band_o)
    n = fl.expected_counts(sc, counts, band)
    got, bad = {"counts": n}, []
    for blk, nm in ((capi.LIGHT, "light"), (capi.POSE, "pose")):
        (He, be), (Ho, bo) = eng.debug_frame_system(blk), systems[blk]
        assert He.shape == Ho.shape and be.shape == bo.shape
        if len(Ho) != sc.F:      # LED light: one global block, compared as tests/test_parity_gpu.py test_normal_equations does
            dev = [(fl.relmax(He, Ho), fl.relmax(be, bo))]
        else:
            dev = []
            for f in range(sc.F):
                if n[f] == 0:
                    assert not He[f].any() and not be[f].any() and not Ho[f].any() and not bo[f].any(), (nm, f)
                    dev.append((0.0, 0.0))
                else:
                    assert np.abs(Ho[f]).max() > 0 and np.abs(bo[f]).max() > 0, (nm, f)
                    dev.append((fl.relmax(He[f], Ho[f]), fl.relmax(be[f], bo[f])))
        for k, part in enumerate(("H", "b")):
            w = int(np.argmax([d[k] for d in dev]))
            got[f"{nm}_{part}"] = {"worst": float(dev[w][k]), "frame": w, "n_obs": n[w] if len(dev) == sc.F else sum(n)}
        bad += [(nm, f, n[f] if len(dev) == sc.F else sum(n), d) for f, d in enumerate(dev) if not (np.isfinite(d[0]) and np.isfinite(d[1]) and max(d) <= fl.NE_TOL)]
    margins(**{"normal_equations" + tag: got, "tolerance_normal_equations": fl.NE_TOL})
    print(case, tag, got)
    assert not bad, bad      # (block, frame, observations of the frame, (deviation of H, of b))
    return n


def check_state(eng, orc, re_, ro, margins, vs, tolerance):
    """the checks of tests/test_edge_gpu.py compare, and poses and light"""
    band = eng.download_band()
    assert np.array_equal(band, orc.download_band())
    assert len(re_) == len(ro)
    e_rel = max(abs(a["e_total"] - b["e_total"]) / (abs(b["e_total"]) + 1e-300) for a, b in zip(re_, ro))
    ve, vo = eng.download_volume(), orc.download_volume()
    m = sdf_margin(ve["dist"], vo["dist"], band, vs)
    got = {"pose": float(np.abs(eng.download_poses() - orc.download_poses()).max()), "light_rel": fl.relmax(eng.download_light(), orc.download_light()), "e_total_rel": float(e_rel)}
    margins(sdf=m, achieved=got, tolerance=tolerance)
    print(got, m)
    for a, b in zip(re_, ro):
        assert abs(a["e_total"] - b["e_total"]) <= tolerance["e_total_rel"] * abs(b["e_total"]) + 1e-12, (a["e_total"], b["e_total"])
    return band, m, got


def state_bits(eng):
    v = eng.download_volume()
    return v["dist"].tobytes(), v["rgb"].tobytes(), eng.download_poses().tobytes(), eng.download_light().tobytes()


def assert_rows_unchanged(eng, frames, P0, L0, name):
    P1, L1 = eng.download_poses(), eng.download_light()
    assert np.isfinite(P1).all() and np.isfinite(L1).all()
    for f in frames:
        assert P0[f].tobytes() == P1[f].tobytes(), (f, P0[f], P1[f], P1[f] - P0[f])
        if name != "LED":
            assert L0[f].tobytes() == L1[f].tobytes(), (f, L0[f], L1[f])


# ---------------------------------------------------------------------------------------------------------------- A: chunk boundaries
A_CASES = ["A-SH1", "A-SH1-u8", "A-SH2", "A-LED"]


@pytest.mark.parametrize("rows", [None, 7, 64])
@pytest.mark.parametrize("case", A_CASES)
def test_chunk_boundary_normal_equations(built, margins, monkeypatch, case, rows):
    set_rows(monkeypatch, rows)
    sc, counts, eng, _ = pair(case)
    n = check_normal_equations(case, eng, margins)
    assert [n[f] for f in (2, 4, 5, 6)] == [0, 1023, 1024, 1025]


def run_two_iterations(case, solver, margins, empty):
    sc, counts, eng, orc = pair(case, solver)
    name = fl.model_of(case)
    for api in (eng, orc):
        api.init_albedo(); api.normalize_weights()
    P0, L0 = eng.download_poses().copy(), eng.download_light().copy()
    re_, ro = eng.iterate(capi.ALL, 2), orc.iterate(capi.ALL, 2)
    tol = {"q999_vs": 1e-4, "max_vs": fl.TOL["dist_vs"], "pose": fl.TOL["pose"], "light_rel": fl.light_tol(name), "e_total_rel": fl.TOL["e_total_rel"]}
    band, m, got = check_state(eng, orc, re_, ro, margins, float(sc.voxel_size), tol)
    n = fl.expected_counts(sc, counts, band)
    margins(counts=n)
    assert m["q999_vs"] <= 1e-4 and m["max_vs"] <= fl.TOL["dist_vs"], m
    assert got["pose"] <= fl.TOL["pose"], got
    assert got["light_rel"] <= fl.light_tol(name), got
    assert_rows_unchanged(eng, empty, P0, L0, name)
    assert not np.array_equal(P0, eng.download_poses())
    return sc, eng, re_


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", A_CASES)
def test_chunk_boundary_iterations(built, margins, monkeypatch, case, solver):
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    sc, eng, re_ = run_two_iterations(case, solver, margins, empty=[2])
    if solver != "ldlt":
        return
    # the engine as shipped solves every frame in the sweeps' last workgroups; PSGSDF_FM_SOLVE=0 (read at create) runs k_solve_light / k_solve_pose behind
    # the sweeps instead: the same bits, on lists tests/test_knobs_gpu.py never sees
    assert eng.get_tuning()["effective"]["fm_solve"] == 1 and eng.get_tuning()["effective"]["frame_solve"] == "ldlt"
    _, u8, _, st = fl.scene(case)
    monkeypatch.setenv("PSGSDF_FM_SOLVE", "0")
    sep = capi.load_engine(sc, sc.K, st, 0)
    monkeypatch.delenv("PSGSDF_FM_SOLVE")
    assert sep.get_tuning()["effective"]["fm_solve"] == 0
    sep.load_scene(sc, u8=u8); sep.init_albedo(); sep.normalize_weights()
    rs = sep.iterate(capi.ALL, 2)
    assert [r["e_total"] for r in rs] == [r["e_total"] for r in re_] and [tuple(np.nan_to_num(r["e_after"], nan=-1.0)) for r in rs] == [tuple(np.nan_to_num(r["e_after"], nan=-1.0)) for r in re_]
    assert state_bits(sep) == state_bits(eng)


# ---------------------------------------------------------------------------------------------------------------- B: wavefront / workgroup boundaries, tiny and one-sided lists
B_COUNTS = [1, 63, 64, 65, 255, 256, 257, 0, 300, 300]


@pytest.mark.parametrize("rows", [None, 64])
@pytest.mark.parametrize("case", ["B-SH1", "B-LED"])
def test_short_lists_normal_equations(built, margins, monkeypatch, case, rows):
    set_rows(monkeypatch, rows)
    sc, counts, eng, _ = pair(case)
    n = check_normal_equations(case, eng, margins)
    assert n[:10] == B_COUNTS and n[10] > 1024      # (frame 10, untouched, sets obs_max: two chunks, the second one empty for every other frame)


@pytest.mark.parametrize("case", ["B-SH1", "B-LED"])
def test_short_lists_run(built, margins, monkeypatch, case):
    """Blocks built from a handful of voxels are singular to rounding (tests/test_edge_gpu.py test_tiny_and_empty_band): no state is compared.  One whole
    iteration must run and stay finite under both frame solvers, and the observation counts of the light and pose steps behind it equal the oracle's."""
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    for solver in SOLVERS:
        sc, counts, eng, orc = pair(case, solver)
        for api in (eng, orc):
            api.init_albedo(); api.normalize_weights()
        recs = eng.iterate(capi.ALL, 1)
        band = eng.download_band()
        assert len(recs) == 1 and np.isfinite(recs[0]["e_total"])
        assert np.isfinite(eng.download_poses()).all() and np.isfinite(eng.download_light()).all() and np.isfinite(eng.download_volume()["dist"][band]).all()
        if solver == "eigen":      # (the same algorithm on both sides: the singular directions are left alone alike)
            orc.iterate(capi.ALL, 1)
            n_obs = {}
            for blk, nm in ((capi.LIGHT, "light"), (capi.POSE, "pose")):
                se, so = eng.step(blk), orc.step(blk)
                n_obs[nm] = (se["n_obs"], so["n_obs"])
            margins(n_obs=n_obs, counts=fl.expected_counts(sc, counts, band))
            assert all(a == b > 0 for a, b in n_obs.values()), n_obs


@pytest.mark.parametrize("case", ["B1-SH1", "B1-LED"])
def test_one_keyframe_sees_everything(built, margins, monkeypatch, case):
    """obs_max comes from frame 10 alone; the workgroups of the ten other frames have nothing to walk, publish zero rows and solve 0 x = 0"""
    for rows in (None, 64):
        set_rows(monkeypatch, rows)
        sc, counts, eng, _ = pair(case, "ldlt")
        n = check_normal_equations(case, eng, margins, tag="" if rows is None else f"_rows{rows}")
        assert n[:10] == [0] * 10 and n[10] > 1024
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    P0, L0 = eng.download_poses().copy(), eng.download_light().copy()
    recs = eng.iterate(capi.ALL, 1)
    assert len(recs) == 1 and np.isfinite(recs[0]["e_total"])
    assert_rows_unchanged(eng, range(10), P0, L0, fl.model_of(case))
    assert P0[10].tobytes() != eng.download_poses()[10].tobytes()


# ---------------------------------------------------------------------------------------------------------------- C: the visibility-word boundary
def test_word_boundary_normal_equations(built, margins, monkeypatch):
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    sc, counts, eng, _ = pair("C-SH1")
    assert sc.vis_words == 2
    n = check_normal_equations("C-SH1", eng, margins)
    assert [n[f] for f in (63, 64, 65, 69)] == [0, 1024, 0, 1025] and n[62] > 1025 and n[66] > 1025


@pytest.mark.parametrize("solver", SOLVERS)
def test_word_boundary_iterations(built, margins, monkeypatch, solver):
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    run_two_iterations("C-SH1", solver, margins, empty=[63, 65])


# ---------------------------------------------------------------------------------------------------------------- D: lists rebuilt by the refinement
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", fl.OPTIMIZE_CASES)
def test_lists_rebuilt_by_the_refinement(built, margins, monkeypatch, case, solver):
    """psgsdf_optimize with the checks of tests/test_edge_gpu.py test_laplacian_and_upsample_schedule.  D-SH1: the settings of that test; the reference's
    loop leaves it through the divergence exit at iteration 5, before the refinement.  D-SH1-refined: damping 10, which carries the loop through the
    refinement at iteration 5 and one iteration on the rebuilt band and lists (tests/_frame_lists.py CASES)."""
    monkeypatch.delenv("PSGSDF_FM_ROWS", raising=False)
    sc, counts, eng, orc = pair(case, solver)
    margins(counts=fl.expected_counts(sc, counts, eng.download_band()))
    P0, L0 = eng.download_poses().copy(), eng.download_light().copy()
    (re_, ce), (ro, co) = eng.optimize(capi.ALL), orc.optimize(capi.ALL)
    assert len(re_) == len(ro) and ce == co
    assert [r["upsampled"] for r in re_] == [r["upsampled"] for r in ro]
    assert [(r["converged"], r["diverged"]) for r in re_] == [(r["converged"], r["diverged"]) for r in ro]
    refined = sum(r["upsampled"] for r in ro)
    assert refined == (1 if case == "D-SH1-refined" else 0) and tuple(eng.info().dim) == tuple(orc.info().dim) == ((48,) * 3 if refined else (24,) * 3)
    assert eng.info().n_band == orc.info().n_band
    band, m, got = check_state(eng, orc, re_, ro, margins, float(sc.voxel_size) / (2 if refined else 1), {"e_total_rel": fl.TOL_D_E})
    margins(records=len(re_), upsampled=[r["upsampled"] for r in re_], n_band=int(len(band)))
    assert_rows_unchanged(eng, [1], P0, L0, "SH1")
