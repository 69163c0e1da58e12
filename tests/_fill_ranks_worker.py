"""worker of tests/test_fill_gpu.py's refusal test: tests/_refused_ranks_worker.py with one more family, the two calls of include/psgsdf_fill.h.
Same command line, same result file.

    python _fill_ranks_worker.py RANK WORLD SPEC.json OUT.json      (peer sockets: MESH_FDS, CU range: MESH_CU_MASKS)
"""
import json
import sys

import _refused_ranks_worker as worker

worker.FAMILIES["fill"] = ((64, 48), lambda eng, vs, N: [lambda: eng.fill_voxels(2, 1), lambda: eng.extract_mesh_filled(2, 1)])

if __name__ == "__main__":
    worker.main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
