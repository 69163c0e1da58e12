"""worker of tests/_refused_ranks.py: one rank of a world-N context (the engine's socket transport).  The calls of family spec["family"] are not
collective: the ranks listed in spec["callers"] make them, the others do not, and nobody may wait for anybody.  Afterwards every rank takes part in
the collective psgsdf_extract_mesh_indexed, which must still work.

    python _refused_ranks_worker.py RANK WORLD SPEC.json OUT.json      (started by tests/_ranks.py run_spec: peer sockets and CU range in its variables)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _with_reference(name):
    """compare and align: three points as a cloud, with a face, and against the largest component"""
    def calls(eng, vs, N):
        pts = (np.float32([[0.5, 0.5, 0.5], [0.4, 0.5, 0.6], [0.6, 0.4, 0.5]]) * N * vs).astype(np.float32)
        call = getattr(eng, name)
        return [lambda: call(pts), lambda: call(pts, np.int32([[0, 1, 2]])), lambda: call(pts, keep_largest=1)]
    return calls


def _curvature(eng, vs, N):
    lin = np.arange(N ** 3 // 2, N ** 3 // 2 + 5, dtype=np.int64)
    return [lambda: eng.curvature_voxels(lin), eng.extract_mesh_curvature, lambda: eng.bake_lod_curvature(2 * vs, 4), lambda: eng.bake_lod_curvature(2 * vs, 4, keep_largest=1)]


def _occlusion(eng, vs, N):
    pts = np.full((5, 3), 0.5 * N * vs, np.float32); nrm = np.tile(np.float32([0, 0, 1]), (5, 1))
    return [lambda: eng.occlusion_points(pts, nrm), lambda: eng.bake_lod_ao(2 * vs, 4), lambda: eng.bake_lod_ao(2 * vs, 4, keep_largest=1)]


# family -> (the scene's image size, the calls a caller makes from eng, the voxel size vs and the scene's N)
FAMILIES = {
    "align": ((160, 120), _with_reference("align_reference")),
    "bake": ((160, 120), lambda eng, vs, N: [lambda: eng.bake_lod(2 * vs, 4), lambda: eng.bake_lod(2 * vs, 4, keep_largest=1)]),
    "compare": ((160, 120), _with_reference("compare_reference")),
    "curvature": ((64, 48), _curvature),
    "fill": ((64, 48), lambda eng, vs, N: [lambda: eng.fill_voxels(2, 1), lambda: eng.extract_mesh_filled(2, 1)]),
    "fit": ((64, 48), lambda eng, vs, N: [eng.band_fit, eng.extract_mesh_fit]),
    "mesh_components": ((160, 120), lambda eng, vs, N: [lambda: eng.extract_mesh_components(), lambda: eng.extract_mesh_components(keep_largest=1)]),
    "mesh_lod": ((160, 120), lambda eng, vs, N: [lambda: eng.extract_mesh_lod(2 * vs), lambda: eng.extract_mesh_lod(2 * vs, keep_largest=1)]),
    "occlusion": ((160, 120), _occlusion),
    "relight": ((160, 120), lambda eng, vs, N: [lambda: eng.relight([dict(kind="directional", vec=[0, 0, 1], samples=16, spread=0.1)], frame=0),
                                                lambda: eng.relight([dict(kind="sh", sh=[1, 0, 0, 0])], frame=0)]),
}


def main(rank, world, spec, out):
    import _ranks
    _ranks.arm(rank, spec)
    from psgradientsdf_amd import capi, synth
    (W, H), calls = FAMILIES[spec["family"]]
    sc = synth.make_scene(N=spec["N"], F=spec["F"], W=W, H=H, model="SH1")
    eng = _ranks.engine(sc, rank, world)
    eng.load_scene(sc)
    eng.init_albedo()
    errors = []
    if rank in spec["callers"]:
        for call in calls(eng, float(eng.info().voxel_size), spec["N"]):
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
