"""worker of tests/test_query_gpu.py: one rank of a world-N context (the engine's socket transport).  The three calls of include/psgsdf_query.h are
not collective: the ranks listed in spec["callers"] make them, the others do not, and nobody may wait for anybody.  Afterwards every rank takes part
in the collective psgsdf_extract_mesh_indexed, which must still work.  (The pattern of tests/_refused_ranks_worker.py.)

    python _query_ranks_worker.py RANK WORLD SPEC.json OUT.json      (started by tests/_ranks.py run_spec: peer sockets and CU range in its variables)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(rank, world, spec, out):
    import _ranks
    _ranks.arm(rank, spec)
    from psgradientsdf_amd import capi, synth
    sc = synth.make_scene(N=spec["N"], F=spec["F"], W=64, H=48, model="SH1")
    eng = _ranks.engine(sc, rank, world)
    eng.load_scene(sc)
    eng.init_albedo()
    errors = []
    if rank in spec["callers"]:
        pts = np.full((5, 3), 0.5 * spec["N"] * float(eng.info().voxel_size), np.float32); up = np.tile(np.float32([0, 0, 1]), (5, 1))
        for call in (lambda: eng.query_points(pts), lambda: eng.project_points(pts, "cell"), lambda: eng.cast_rays(pts, up)):
            try:
                call()
                errors.append("")
            except capi.PsgsdfError as e:
                errors.append(str(e))
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    json.dump({"errors": errors, "faces": int(len(faces)), "first": int(first)}, open(out, "w"))
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
