"""Cost of the field queries (include/psgsdf_query.h) on a synthetic SH1 scene on an N^3 grid, after one iteration: M points spread within 1.5
voxels of the welded mesh's vertices, and M rays towards them, through psgsdf_query_points, psgsdf_project_points (both models) and psgsdf_cast_rays.
Every call is timed twice: with the queries in a random order (what a caller's scan looks like to the grid) and sorted by the voxel they fall in,
which is what the caller's order costs -- the engine itself keeps the order it is given and does not sort.  Wall-clock per call (host clock; every
call ends in a stream synchronise, and uploads and downloads are part of it), then the kernels' own event-timed ms per launch from psgsdf_kernel_times.
    python tools/time_query.py N [M] [reps]
For the kernel times of record run it under the tracer in a run of its own, with no counters in it:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_query.py 256
(kernel names: k_query_points, k_query_project, k_query_rays)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psgradientsdf_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
sc = synth.make_scene(N=N, F=8, W=320, H=240, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
dim = [int(x) for x in eng.info().dim]
vs = float(np.float32(eng.info().voxel_size))
xyz, nrm, _, _, _ = eng.extract_mesh_indexed()
rng = np.random.default_rng(1)
pick = rng.integers(0, len(xyz), size=M)
pts = (xyz[pick].astype(np.float64) + rng.uniform(-1.5, 1.5, size=(M, 3)) * vs).astype(np.float32)
org = (xyz[pick].astype(np.float64) + 6 * vs * nrm[pick]).astype(np.float32)      # six voxels off the surface, looking back at it
dirs = (-nrm[pick]).astype(np.float32)
cell = np.floor(pts / vs + 0.5).astype(np.int64)
by_voxel = np.argsort((cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0], kind="stable")
orders = {"random": np.arange(M), "by_voxel": by_voxel}
out = {"grid": dim, "queries": M, "reps": reps, "mesh_vertices": int(len(xyz))}
for tag, o in orders.items():
    p, ro, rd = np.ascontiguousarray(pts[o]), np.ascontiguousarray(org[o]), np.ascontiguousarray(dirs[o])
    calls = [("query_points_cell", lambda: eng.query_points(p, "cell")), ("query_points_trilinear", lambda: eng.query_points(p, "trilinear")),
             ("project_points_cell", lambda: eng.project_points(p, "cell")), ("project_points_trilinear", lambda: eng.project_points(p, "trilinear")),
             ("cast_rays", lambda: eng.cast_rays(ro, rd))]
    first = {name: call() for name, call in calls}      # (warm-up: code objects, allocations)
    res = {}
    for name, call in calls:      # wall-clock first, without the event pair around every launch
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        res[name + "_ms"] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
    eng.set_profiling(True)
    eng.reset_kernel_times()
    for name, call in calls:
        eng.reset_kernel_times()
        for _ in range(reps):
            call()
        res[name + "_kernel_ms"] = {k: round(ms / max(n, 1), 4) for k, (ms, n) in eng.kernel_times().items() if k.startswith("k_query")}
    eng.set_profiling(False)
    res["counts"] = {name: first[name]["counts"] for name in first}
    res["mean_iterations"] = {m: round(float(first["project_points_" + m]["iterations"].mean()), 3) for m in ("cell", "trilinear")}
    out[tag] = res
print(json.dumps(out))
