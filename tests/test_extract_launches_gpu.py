"""The timed kernel launches of every mesh extraction call, pinned: which kernels one call launches, how often, and nothing else (the crop box and the
scans are not timed and do not appear).  The calls build on each other -- extract_mesh_components repeats the welded extraction, extract_mesh_lod
repeats both, the bake, the comparison and the alignment start from one of the three -- and a change to the host code between them must leave
these lists as they are."""
import numpy as np
import pytest

from psgradientsdf_amd import capi, synth
from test_fit_gpu import engine as fit_engine
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of

pytestmark = pytest.mark.gpu

MC = ["mc_count", "mc_emit"]
WMESH = ["wmesh_mark", "wmesh_faces", "wmesh_verts"]
MCOMP = ["mcomp_init", "mcomp_hook", "mcomp_flatten", "mcomp_edges", "mcomp_vstats", "mcomp_fstats", "mcomp_ecount"]
MCOMP_DROP = MCOMP + ["mcomp_keep", "mcomp_compact"]
MLOD = ["mlod_cluster", "mlod_ftable", "mlod_fkeep", "mlod_vflag", "mlod_emit"]
BAKE = ["k_render_bricks", "bake"]
GRID = ["compare_total", "compare_count", "compare_fill"]
ALIGN_1 = ["align_query_1", "align_rows_1"]
ALIGN_2 = ["align_query_2", "align_rows_2"]


def once(names):
    return {k: 1 for k in names}


def launches_of(eng, call):
    eng.reset_kernel_times()
    call()
    return {k: n for k, (ms, n) in eng.kernel_times().items()}


def test_every_call_launches_its_kernels_once_and_nothing_else(built):
    v, dim, vs = pieces_volume()
    eng = upload(v, dim, vs)      # (never initialised: no band, no band kernel)
    vs = vs_of(eng)
    before = eng.extract_mesh_indexed()      # warm-up
    eng.reset_kernel_times()
    eng.set_profiling(True)

    def refused():
        with pytest.raises(capi.PsgsdfError, match="rc=-3"):      # PSGSDF_ERR_UNSUPPORTED: cluster coordinates beyond 2^20
            eng.extract_mesh_lod(1e-7 * vs)

    for tag, call, names in (("mesh", eng.extract_mesh, MC),
                             ("indexed", eng.extract_mesh_indexed, WMESH),
                             ("components", eng.extract_mesh_components, WMESH + MCOMP),
                             ("components, keep_largest=1", lambda: eng.extract_mesh_components(keep_largest=1), WMESH + MCOMP_DROP),
                             ("lod", lambda: eng.extract_mesh_lod(2 * vs), WMESH + MLOD),
                             ("lod, keep_largest=1", lambda: eng.extract_mesh_lod(2 * vs, keep_largest=1), WMESH + MCOMP_DROP + MLOD),
                             ("lod, refused", refused, WMESH + ["mlod_cluster"])):
        got = launches_of(eng, call)
        print(tag, sorted(got.items()))
        assert got == {k: 1 for k in names}, (tag, got)
    after = eng.extract_mesh_indexed()
    eng.set_profiling(False)
    assert len(before[0]) == 3612 and len(before[3]) == 7204
    for a, b in zip(before[:4], after[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert before[4] == after[4]


def test_calls_that_start_from_a_mesh_launch_their_kernels_and_nothing_else(built):
    """the bakes, ambient occlusion, the comparison and the alignment on the same state; the reference is the engine's own welded mesh moved 0.3
    voxels along its normals, with the same faces (tools/time_compare.py's)"""
    v, dim, vs = pieces_volume()
    eng = upload(v, dim, vs)
    vs = vs_of(eng)
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    R = (xyz.astype(np.float64) + 0.3 * vs * nrm.astype(np.float64)).astype(np.float32)
    pts, up = xyz[:: len(xyz) // 5][:5], nrm[:: len(xyz) // 5][:5]
    twice = lambda names: {k: 2 for k in names}
    cases = (("bake", lambda: eng.bake_lod(2 * vs, 4), once(WMESH + MLOD + BAKE)),
             ("bake, keep_largest=1", lambda: eng.bake_lod(2 * vs, 4, keep_largest=1), once(WMESH + MCOMP_DROP + MLOD + BAKE)),
             ("bake with occlusion", lambda: eng.bake_lod_ao(2 * vs, 4), once(WMESH + MLOD + BAKE + ["occlusion"])),
             ("occlusion at points", lambda: eng.occlusion_points(pts, up), once(["k_render_bricks", "occlusion"])),
             ("compare", lambda: eng.compare_reference(R, faces), {**once(WMESH + ["compare_query_ref", "compare_query_rec"]), **twice(GRID + ["compare_stats"])}),
             ("compare, keep_largest=1", lambda: eng.compare_reference(R, faces, keep_largest=1),
              {**once(WMESH + MCOMP_DROP + ["compare_query_ref", "compare_query_rec"]), **twice(GRID + ["compare_stats"])}),
             ("align, both directions, no step", lambda: eng.align_reference(R, faces, directions=3, max_iters=0),
              {**once(WMESH + ALIGN_1 + ALIGN_2 + ["align_fold"]), **twice(GRID + ["align_move"])}),
             ("align, both directions, one step", lambda: eng.align_reference(R, faces, directions=3, max_iters=1),
              {**once(WMESH), **twice(GRID + ALIGN_1 + ALIGN_2 + ["align_fold"]), "align_move": 4}),
             ("align, reference to mesh, no step", lambda: eng.align_reference(R, faces, directions=1, max_iters=0),
              once(WMESH + GRID + ALIGN_1 + ["align_move", "align_fold"])))
    for tag, call, expected in cases:      # warm-up
        call()
    eng.set_profiling(True)
    for tag, call, expected in cases:
        got = launches_of(eng, call)
        print(tag, sorted(got.items()))
        assert got == expected, (tag, got)
    eng.set_profiling(False)


def test_the_fit_calls_launch_their_kernels_and_nothing_else(built):
    """the two calls that need a band, on the smallest initialised engine of tests/test_fit_gpu.py"""
    eng = fit_engine(synth.make_scene(N=24, F=3, W=64, H=48, model="SH1"))
    cases = (("band_fit", eng.band_fit, once(["band_fit"])), ("extract_mesh_fit", eng.extract_mesh_fit, once(WMESH + ["band_fit", "wmesh_fit"])))
    for tag, call, expected in cases:      # warm-up
        call()
    eng.set_profiling(True)
    for tag, call, expected in cases:
        got = launches_of(eng, call)
        print(tag, sorted(got.items()))
        assert got == expected, (tag, got)
    eng.set_profiling(False)
