"""The coefficients of the persistent distance solve as five 16-byte LDS words per row slot (pcg_solve.h SolveCoefs), and the row slots a wavefront
skips because none of its lanes has a row there: neither may change a bit.

Every partition below runs the 64^3 / 8-keyframe scene (160 x 120, 21 120 band rows) for three iterations in fresh contexts (the pattern of tests/test_solve_window_gpu.py)
-- windowed instance, gathering instance, and once the per-pass kernels -- and compares

* window on against off: the raw bits of the band distances, the pass counts and e_total;
* persistent against per-pass (PSGSDF_PCG_PERSIST=0, the classic float recurrences: DESIGN.md section 2, deviation 3): pass counts to +-1, distances
  within the parity tests' bound for every band voxel (tests/test_parity_gpu.py OPT_MAX_VS, in voxels);
* the tuning record's window budget against 160 KB - R x 40 960 B of coefficients - the kernel's static LDS.

Partitions (PSGSDF_PCG_SOLVE_ROWS = rows per workgroup; the engine rounds it up to a multiple of 64, so a PARTITION never ends inside a wavefront):
   128  R = 1
   576  R = 2, the second slot holds rows for tid < 64 only: wavefronts 1-7 skip it
  1344  R = 3, the third slot live for tid < 320: the headline's shape (256 workgroups x 1 344 rows), wavefronts 5-7 skip it
  1536  R = 3, every slot full
  1000  rounded to 1024 by the engine: R = 2, every slot full.  No value of the knob makes a slot's last live wavefront partial -- the rounding to 64
        rows is what the kernel relies on -- so a partial wavefront can only come from the END OF THE BAND.

The band ending inside a wavefront: the 64^3 / 8-keyframe band has 21 120 = 330 x 64 rows, so there it does NOT happen.  test_band_ends_inside_a_wavefront
therefore runs the 48^3 / 6-keyframe scene as well (11 896 rows = 185 x 64 + 56, asserted) at 1 344 rows per workgroup and at the default partition: the
last workgroup's last live wavefront has live and dead lanes in the same row slot and keeps the per-lane guards, the wavefronts behind it skip the slot."""
import numpy as np
import pytest

from psgradientsdf_amd import capi, synth
from test_parity_gpu import OPT_MAX_VS
from test_solve_window_gpu import run, same_bits, windowed

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 * 1024           # one CU
SLOT_BYTES = 5 * 16 * 512        # five 16-byte words for each of a workgroup's 512 threads
STATIC_LDS = 1552                # k_cgp_solve<R, false, WIN>: red 512 + red2 1024 + three abort words 12, rounded to 16 (the compiler's resource remarks)
WIN_LOADS = 12 * 512             # a thread fetches at most 12 window slots per pass

_scenes, _runs = {}, {}


def scene(model, N=64, F=8):
    if (model, N, F) not in _scenes:
        _scenes[model, N, F] = synth.make_scene(N=N, F=F, W=160, H=120, model=model)
    return _scenes[model, N, F]


def cached(model, rows, window, persist=1, N=64, F=8):
    """one run per (scene, partition, instance), shared by the tests and never modified"""
    key = (model, N, F, rows, window, persist)
    if key not in _runs:
        env = {"PSGSDF_PCG_PERSIST": str(persist)}
        if rows:
            env["PSGSDF_PCG_SOLVE_ROWS"] = str(rows)
        _runs[key] = run(scene(model, N, F), window, env)
    return _runs[key]


def against_per_pass(on, classic, vs):
    """the persistent solve against the per-pass kernels: pass counts to +-1, every band distance within the parity tests' bound"""
    assert classic["win"]["last_solve_windowed"] in (-1, 0) and np.array_equal(classic["band"], on["band"])
    dev = float(np.abs(on["bits"].view(np.float32).astype(np.float64) - classic["bits"].view(np.float32).astype(np.float64)).max() / vs)
    print("persistent against per-pass: cg", on["cg"], classic["cg"], "max |d| / vs", dev)
    assert all(abs(a - b) <= 1 for a, b in zip(on["cg"], classic["cg"])), (on["cg"], classic["cg"])
    assert dev <= OPT_MAX_VS, dev


# rows asked for, rows per workgroup the engine makes of it, row slots per thread, first wavefront without a row in the last slot (8: none)
PARTITIONS = [(128, 128, 1, 2), (576, 576, 2, 1), (1344, 1344, 3, 5), (1536, 1536, 3, 8), (1000, 1024, 2, 8)]


@pytest.mark.parametrize("ask,rows,rpt,first_dead", PARTITIONS)
def test_partition(built, ask, rows, rpt, first_dead):
    on, off = cached("SH1", ask, 1), cached("SH1", ask, 0)
    print("solve_window:", on["win"], "cg", on["cg"])
    same_bits(on, off)
    w = windowed(on, rpt)
    assert w["rows_per_workgroup"] == rows and w["workgroups"] == (len(on["band"]) + rows - 1) // rows, w
    live_last_slot = rows - (rpt - 1) * 512
    assert (live_last_slot + 63) // 64 == first_dead if first_dead < 8 else live_last_slot == 512      # whole wavefronts without a row in the last slot
    # the tuning record's budget
    assert w["budget_doubles"] == min((LDS_BYTES - rpt * SLOT_BYTES - STATIC_LDS) // 8, WIN_LOADS), w
    against_per_pass(on, cached("SH1", 0, 1, persist=0), float(scene("SH1").voxel_size))


@pytest.mark.parametrize("ask", [1344, 0])
def test_band_ends_inside_a_wavefront(built, ask):
    on, off = cached("SH1", ask, 1, N=48, F=6), cached("SH1", ask, 0, N=48, F=6)
    print("solve_window:", on["win"], "cg", on["cg"])
    same_bits(on, off)
    w = windowed(on, 3 if ask else None)
    n, rows = len(on["band"]), w["rows_per_workgroup"]
    last = n - (w["workgroups"] - 1) * rows      # rows of the last workgroup
    assert n % 64 != 0 and 0 < last <= rows and last % 64 != 0, (n, w)      # ... its last live wavefront is partial
    if ask:
        assert last > 1024 and (last - 1024 + 63) // 64 < 8      # in the third row slot, with whole wavefronts without a row behind it
    against_per_pass(on, cached("SH1", 0, 1, persist=0, N=48, F=6), float(scene("SH1", 48, 6).voxel_size))


def test_headline_budget_still_holds_the_headline_window(built):
    """R = 3 leaves 160 KB - 3 x 40 960 B - the static LDS, about 4 900 doubles; the 256^3 x 50 band's largest window is 4 318 doubles
    (profiles/r07_notes.md section 2) and must still run the windowed instance"""
    w = cached("SH1", 1344, 1)["win"]
    assert w["budget_doubles"] == (LDS_BYTES - 3 * SLOT_BYTES - STATIC_LDS) // 8 and w["budget_doubles"] >= 4318, w


@pytest.mark.parametrize("model", ["LED", "SH2"])
def test_other_models_at_the_default_partition(built, model):
    on, off = cached(model, 0, 1), cached(model, 0, 0)
    same_bits(on, off)
    windowed(on)
    against_per_pass(on, cached(model, 0, 1, persist=0), float(scene(model).voxel_size))
