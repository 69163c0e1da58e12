"""The oracle alone on every scene of tests/test_frame_lists_gpu.py: what that file's tolerances rest on.

  * the per-keyframe counts that tests/_frame_lists.py `skew` was asked for arrive in the oracle's band;
  * on every scene whose STATE the GPU file compares, the oracle and its own FMA build (the same source with multiply-adds contracted: the yardstick of
    tests/test_parity_gpu.py) deviate by at most ONE THIRD of each tolerance asserted there, in both solver modes -- the engine contracts multiply-adds
    as well, and the project's bars were set with about that head-room;
  * a keyframe without a single observation keeps its pose row (SH models: its light row too) bit for bit through two iterations, in both solver modes;
  * the refinement scene does not sit on a divergence edge: both builds write the same records.
"""
import numpy as np
import pytest

import _frame_lists as fl
from psgradientsdf_amd import capi

SOLVER_MODES = [1, 0]      # 1: the reference's global float Jacobi-PCG ("eigen"), 0: direct solves ("ldlt")


def oracles(case, mode, fma_too=True):
    from oracle import oracle
    sc, u8, counts, st = fl.scene(case)
    out = [oracle.Oracle(sc, sc.K, st, threads=8, solver_mode=mode)]
    if fma_too:
        out.append(oracle.Oracle(sc, sc.K, st, threads=8, solver_mode=mode, fma=True))
    for api in out:
        api.load_scene(sc, u8=u8)
    return sc, counts, out


@pytest.mark.parametrize("case", sorted(fl.CASES))
def test_requested_counts_arrive_in_the_band(margins, case):
    sc, counts, (orc,) = oracles(case, 1, fma_too=False)
    band = orc.download_band()
    got = fl.expected_counts(sc, counts, band)
    assert orc.info().n_band == len(band) == int(((sc.vis[band] != 0).any(axis=1)).sum())
    margins(counts=got, n_band=int(len(band)))
    if case.startswith("B-"):
        # frame 8: the band's first rows only; frame 9: its last rows only -- k_obs_fill starts frame 9 from a run of zeros (whole 256-row passes of
        # its first 2048-row block without a row), ends frame 8 with one, and frame 9's list goes on across the block boundary with a non-zero offset.
        # (This band has 2565 rows: frame 9's 300 rows do not fit into the 517 rows of the last block alone.)
        r8, r9 = np.nonzero(fl.frame_bit(sc.vis[band], 8))[0], np.nonzero(fl.frame_bit(sc.vis[band], 9))[0]
        margins(frame8_last_row=int(r8.max()), frame9_first_row=int(r9.min()), frame9_rows_in_last_block=int((r9 >= 2048 * ((len(band) - 1) // 2048)).sum()))
        assert r8.max() + 256 < r9.min() and r9.min() >= 256 and len(band) > 2048 and r9.max() >= 2048 > r9.min(), (r8.max(), r9.min(), r9.max(), len(band))


@pytest.mark.parametrize("mode", SOLVER_MODES)
@pytest.mark.parametrize("case", fl.STATE_CASES)
def test_fma_build_within_a_third_of_the_tolerances(margins, case, mode):
    sc, counts, (orc, fma) = oracles(case, mode)
    name = fl.model_of(case)
    for api in (orc, fma):
        api.init_albedo(); api.normalize_weights()
    ro, rf = orc.iterate(capi.ALL, 2), fma.iterate(capi.ALL, 2)
    band = orc.download_band()
    assert np.array_equal(band, fma.download_band())
    got = {"dist_vs": float(np.abs(orc.download_volume()["dist"][band] - fma.download_volume()["dist"][band]).max() / float(sc.voxel_size)),
           "pose": float(np.abs(orc.download_poses() - fma.download_poses()).max()),
           "light_rel": fl.relmax(fma.download_light(), orc.download_light()),
           "e_total_rel": max(abs(a["e_total"] - b["e_total"]) / abs(b["e_total"]) for a, b in zip(rf, ro))}
    tol = dict(fl.TOL, light_rel=fl.light_tol(name))
    margins(achieved=got, tolerance={k: v / 3 for k, v in tol.items()})
    assert all(np.isfinite(v) and v <= tol[k] / 3 for k, v in got.items()), (got, tol)


@pytest.mark.parametrize("mode", SOLVER_MODES)
@pytest.mark.parametrize("case", sorted(fl.CASES))
def test_empty_frames_keep_their_pose_and_light(case, mode):
    sc, counts, (orc,) = oracles(case, mode, fma_too=False)
    empty = [f for f, n in counts.items() if n == 0]
    assert empty
    orc.init_albedo(); orc.normalize_weights()
    P0, L0 = orc.download_poses().copy(), orc.download_light().copy()
    recs = orc.iterate(capi.ALL, 2)
    P1, L1 = orc.download_poses(), orc.download_light()
    assert all(np.isfinite(r["e_total"]) for r in recs) and np.isfinite(P1).all() and np.isfinite(L1).all()
    for f in empty:
        assert P0[f].tobytes() == P1[f].tobytes(), f
        if fl.model_of(case) != "LED":
            assert L0[f].tobytes() == L1[f].tobytes(), f
    assert not np.array_equal(P0, P1)      # (the other frames moved)


@pytest.mark.parametrize("mode", SOLVER_MODES)
@pytest.mark.parametrize("case", fl.OPTIMIZE_CASES)
def test_refinement_scene_is_off_the_divergence_edge(margins, case, mode):
    sc, counts, (orc, fma) = oracles(case, mode)
    P0, L0 = orc.download_poses().copy(), orc.download_light().copy()
    (ro, co), (rf, cf) = orc.optimize(capi.ALL), fma.optimize(capi.ALL)
    assert len(ro) == len(rf) and co == cf
    # the first scene ends before the refinement (see tests/_frame_lists.py CASES), the second runs one iteration behind it, on rebuilt lists
    assert sum(r["upsampled"] for r in ro) == (1 if case == "D-SH1-refined" else 0) and tuple(orc.info().dim) == ((48,) * 3 if case == "D-SH1-refined" else (24,) * 3)
    assert case != "D-SH1-refined" or (ro[5]["upsampled"] == 1 and len(ro) == 7)
    assert [(r["upsampled"], r["converged"], r["diverged"]) for r in ro] == [(r["upsampled"], r["converged"], r["diverged"]) for r in rf]
    assert orc.info().n_band == fma.info().n_band and np.array_equal(orc.download_band(), fma.download_band())
    e_rel = max(abs(a["e_total"] - b["e_total"]) / abs(b["e_total"]) for a, b in zip(rf, ro))
    margins(records=len(ro), upsampled=[r["upsampled"] for r in ro], e_total_rel=float(e_rel), tolerance={"e_total_rel": fl.TOL_D_E / 3})
    assert e_rel <= fl.TOL_D_E / 3
    assert P0[1].tobytes() == orc.download_poses()[1].tobytes() and L0[1].tobytes() == orc.download_light()[1].tobytes()
