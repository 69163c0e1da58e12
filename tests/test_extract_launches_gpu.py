"""The timed kernel launches of every mesh extraction call, pinned: which kernels one call launches, once each and nothing else (the crop box and the
scans are not timed and do not appear).  The calls build on each other -- extract_mesh_components repeats the welded extraction, extract_mesh_lod
repeats both -- and a change to the host code between them must leave these lists as they are."""
import numpy as np
import pytest

from psgradientsdf_amd import capi
from test_mesh_components_cpu import pieces_volume
from test_mesh_components_gpu import upload, vs_of

pytestmark = pytest.mark.gpu

MC = ["mc_count", "mc_emit"]
WMESH = ["wmesh_mark", "wmesh_faces", "wmesh_verts"]
MCOMP = ["mcomp_init", "mcomp_hook", "mcomp_flatten", "mcomp_edges", "mcomp_vstats", "mcomp_fstats", "mcomp_ecount"]
MCOMP_DROP = MCOMP + ["mcomp_keep", "mcomp_compact"]
MLOD = ["mlod_cluster", "mlod_ftable", "mlod_fkeep", "mlod_vflag", "mlod_emit"]


def test_every_call_launches_its_kernels_once_and_nothing_else(built):
    v, dim, vs = pieces_volume()
    eng = upload(v, dim, vs)      # (never initialised: no band, no band kernel)
    vs = vs_of(eng)
    before = eng.extract_mesh_indexed()      # warm-up
    eng.reset_kernel_times()
    eng.set_profiling(True)

    def launches(call):
        eng.reset_kernel_times()
        call()
        return {k: n for k, (ms, n) in eng.kernel_times().items()}

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
        got = launches(call)
        print(tag, sorted(got.items()))
        assert got == {k: 1 for k in names}, (tag, got)
    after = eng.extract_mesh_indexed()
    eng.set_profiling(False)
    assert len(before[0]) == 3612 and len(before[3]) == 7204
    for a, b in zip(before[:4], after[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert before[4] == after[4]
