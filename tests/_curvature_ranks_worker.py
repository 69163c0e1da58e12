"""worker of tests/test_curvature_gpu.py's refusal test: tests/_refused_ranks_worker.py with one more family, the three calls of
include/psgsdf_curvature.h.  Same command line, same result file.

    python _curvature_ranks_worker.py RANK WORLD SPEC.json OUT.json      (peer sockets: MESH_FDS, CU range: MESH_CU_MASKS)
"""
import json
import sys

import numpy as np

import _refused_ranks_worker as worker


def _curvature(eng, vs, N):
    lin = np.arange(N ** 3 // 2, N ** 3 // 2 + 5, dtype=np.int64)
    return [lambda: eng.curvature_voxels(lin), eng.extract_mesh_curvature, lambda: eng.bake_lod_curvature(2 * vs, 4), lambda: eng.bake_lod_curvature(2 * vs, 4, keep_largest=1)]


worker.FAMILIES["curvature"] = ((64, 48), _curvature)

if __name__ == "__main__":
    worker.main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
