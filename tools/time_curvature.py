"""Cost of the surface curvature (include/psgsdf_curvature.h) on a synthetic SH1 scene on an N^3 grid, after one iteration: psgsdf_curvature_voxels over the
band (the list ascending, as psgsdf_download_band returns it), psgsdf_extract_mesh_curvature next to psgsdf_extract_mesh_indexed (it adds
k_wmesh_curv), psgsdf_bake_lod_curvature next to psgsdf_bake_lod at a cell of 4 voxels with 8 texels along an edge (it adds k_bake_curv).
Wall-clock per call (host clock; every call ends in a stream synchronise), then in a second pass the kernels' own event-timed ms per launch from
psgsdf_kernel_times:
    python tools/time_curvature.py N [reps]
For the kernel times of record run it under the tracer in a run of its own, with no counters in it:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_curvature.py 256
(kernel names: k_curv_voxels; k_wmesh_curv against k_wmesh_verts; k_bake_curv against k_bake)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psgradientsdf_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
sc = synth.make_scene(N=N, F=8, W=320, H=240, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
vs = float(np.float32(eng.info().voxel_size))
band = eng.download_band().astype(np.int64)
calls = (("curvature_voxels_band", lambda: eng.curvature_voxels(band)), ("extract_mesh_indexed", eng.extract_mesh_indexed), ("extract_mesh_curvature", eng.extract_mesh_curvature),
         ("bake_lod_4vs_R8", lambda: eng.bake_lod(4 * vs, 8)), ("bake_lod_curvature_4vs_R8", lambda: eng.bake_lod_curvature(4 * vs, 8)))
first = {name: call() for name, call in calls}      # (warm-up: code objects, allocations)
wall = {}
for name, call in calls:      # wall-clock first, without the event pair around every launch
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall[name + "_ms"] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
eng.reset_kernel_times()
eng.set_profiling(True)
for name, call in calls:
    for _ in range(reps):
        call()
kt = eng.kernel_times()
eng.set_profiling(False)
rows, mesh, bake = first["curvature_voxels_band"], first["extract_mesh_curvature"], first["bake_lod_curvature_4vs_R8"]
print(json.dumps({"grid": list(eng.info().dim), "reps": reps, **wall,
                  "kernel_ms_per_launch": {k: round(ms / max(n, 1), 4) for k, (ms, n) in kt.items() if k in ("curv_voxels", "wmesh_curv", "wmesh_verts", "bake_curv", "bake")},
                  "band": {"voxels": int(len(band)), "valid": int(rows["valid"].sum())},
                  "mesh": {"vertices": int(len(mesh["xyz"])), "faces": int(len(mesh["faces"])), "valid_end_voxels_0_1_2": np.bincount(mesh["valid"], minlength=3).tolist()},
                  "bake": {"width": bake["width"], "height": bake["height"], "texels": bake["n_texels"], "hits": bake["n_hits"], "valid": bake["n_valid"]}}))
