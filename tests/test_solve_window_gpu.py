"""The windowed instance of the persistent distance solve (PSGSDF_PCG_WINDOW, pcg_solve.h k_cgp_solve<.., WIN>: every workgroup fetches the band rows its
rows reference once per pass into an LDS window instead of gathering 18 values per row and thread) must give the bits of the gathering instance:
the same products in the same order.  Every case runs the same scene in two fresh contexts, window on and off, and compares the raw bits of the band
distances, the CG pass counts and the energies; the tuning record must say which instance the last solve ran -- a band whose windows do not fit falls
back to the gathers and says so.

The partition of the persistent solve is shaped with PSGSDF_PCG_SOLVE_ROWS (rows per workgroup; PSGSDF_PCG_ROWS / PSGSDF_PCG_BLOCKS shape the per-pass
kernels only).  The 64^3 / 8-keyframe scene has about 21 000 band rows, about 470 per z plane; its default partition is 40 workgroups of 576 rows."""
import os

import numpy as np
import pytest

from psgradientsdf_amd import capi, synth

pytestmark = pytest.mark.gpu

_scenes = {}


def scene(N, F, model):
    key = (N, F, model)
    if key not in _scenes:
        _scenes[key] = synth.make_scene(N=N, F=F, W=160, H=120, model=model)
    return _scenes[key]


def run(sc, window, env=None, optimize=False, **settings):
    """one fresh context (the knobs are read when it is created): three iterations, or the whole loop"""
    env = dict(env or {}, PSGSDF_PCG_WINDOW=str(window))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id, **settings), 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        eng.load_scene(sc)
        if optimize:
            recs, _ = eng.optimize(capi.ALL)
        else:
            eng.init_albedo(); eng.normalize_weights()
            recs = eng.iterate(capi.ALL, 3)
        band = eng.download_band()
        dist = np.ascontiguousarray(eng.download_volume()["dist"][band], dtype=np.float32)
        eff = eng.get_tuning()["effective"]
        return dict(bits=dist.view(np.uint32), cg=[r["cg_iters"] for r in recs], e=[r["e_total"] for r in recs], up=[r["upsampled"] for r in recs],
                    band=band, knob=eff["pcg_window"], win=eff["solve_window"])
    finally:
        eng.close()


def same_bits(on, off):
    assert off["knob"] == 0 and off["win"]["last_solve_windowed"] == 0, off["win"]
    assert on["knob"] == 1
    assert np.array_equal(on["band"], off["band"])
    assert np.array_equal(on["bits"], off["bits"]), int((on["bits"] != off["bits"]).sum())
    assert on["cg"] == off["cg"] and min(on["cg"]) > 0, (on["cg"], off["cg"])
    assert on["e"] == off["e"], (on["e"], off["e"])


def pair(sc, env=None, **kw):
    on, off = run(sc, 1, env, **kw), run(sc, 0, env, **kw)
    print("solve_window:", on["win"], "cg", on["cg"])
    same_bits(on, off)
    return on


def windowed(on, rows_per_thread=None):
    w = on["win"]
    assert w["fits"] == 1 and w["fallback"] == "" and w["last_solve_windowed"] == 1 and 0 < w["window_doubles"] <= w["budget_doubles"], w
    if rows_per_thread:
        assert (w["rows_per_workgroup"] + 511) // 512 == rows_per_thread, w
    return w


def test_adjacent_workgroups(built):
    """default partition: z neighbours sit in the adjacent workgroups, the last workgroup is partial; three solves rotate the tags' epoch"""
    w = windowed(pair(scene(64, 8, "SH1")))
    assert w["rows_per_workgroup"] > 470 and w["workgroups"] * w["rows_per_workgroup"] > 20000


def test_neighbours_several_workgroups_away(built):
    """128 rows per workgroup: a z plane spans more than three workgroups, so the z segments lie wholly outside the neighbouring workgroups and the
    in-plane segment has halo on both sides"""
    w = windowed(pair(scene(64, 8, "SH1"), {"PSGSDF_PCG_SOLVE_ROWS": "128"}), 1)
    assert w["rows_per_workgroup"] == 128 and w["workgroups"] > 150
    assert w["window_doubles"] > 3 * 128      # (three separate ranges and the halo)


@pytest.mark.parametrize("rows,rpt", [(512, 1), (1024, 2), (1536, 3)])
def test_every_row_count_has_its_instance(built, rows, rpt):
    w = windowed(pair(scene(64, 8, "SH1"), {"PSGSDF_PCG_SOLVE_ROWS": str(rows)}), rpt)
    assert w["rows_per_workgroup"] == rows


def test_window_that_does_not_fit_falls_back_and_says_so(built):
    """Four rows per thread leave 160 KB - 4 x 38 KB - the static buffers = about 800 doubles, less than the 2048 own rows: the gathering instance
    runs, the record names the reason, the bits are the same.  (Sizes: "window_doubles" is the table's maximum over the workgroups, "budget_doubles"
    what the LDS holds next to the coefficients, both from the tuning record.  Between 1536 rows per workgroup -- three rows per thread, budget about
    5 700 doubles, need about 3 x 1536 + two z planes' halo -- and four rows per thread there is no partition whose window is just over the budget:
    the budget drops to a seventh at the step.)"""
    on = pair(scene(64, 8, "SH1"), {"PSGSDF_PCG_SOLVE_ROWS": "2048"})
    w = on["win"]
    assert w["rows_per_workgroup"] == 2048 and w["budget_doubles"] < 2048 < w["window_doubles"], w
    assert w["fits"] == 0 and w["fallback"] == "window does not fit" and w["last_solve_windowed"] == 0, w


def test_band_rebuilt_by_the_refinement(built):
    """psgsdf_optimize through the 2x refinement: the table is recomputed with the band (32^3 -> 64^3, 5 300 -> 21 000 rows; damping 10 keeps the loop
    alive up to the refinement at iteration 5, and one more iteration solves on the refined band)"""
    sc = scene(32, 6, "SH1")
    on = pair(sc, optimize=True, upsample=1, max_it=18, conv_threshold=0.0, damping=10.0)
    assert sum(on["up"]) == 1 and len(on["cg"]) > on["up"].index(1) + 1 and len(on["band"]) > 20000
    windowed(on)


@pytest.mark.parametrize("model", ["LED", "SH2"])
def test_other_models(built, model):
    windowed(pair(scene(48, 12, model)))
