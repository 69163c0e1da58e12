"""Cost of the comparison with a reference (include/psgsdf_compare.h, csrc/compare.hip): a synthetic SH1 scene on an N^3 grid with F keyframes, one
iteration, and its own welded mesh displaced by 0.3 voxels along the vertex normals (same faces) as the reference.  Per cell edge of the search grid
(voxels; PSGSDF_TIME_COMPARE_CELLS, default "1,2,4", 2 being the engine's choice): the kernels' event-timed ms per call -- grid build (k_cmp_total,
k_cmp_cells twice; both directions), the search each way (k_cmp_query), the statistics (k_cmp_stats; both directions) -- as median and range over
the repetitions, the whole call's wall time, and the mean number of candidate pairs a query evaluates each way (psgsdf_get_tuning "last_compare").
    python tools/time_compare.py N F [reps]
For the kernel times of record run it under the tracer in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_compare.py 256 50
(the scan between count and fill is extract.hip's k_cscan_*; the welded mesh in front is k_wmesh_*)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psgradientsdf_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 50
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
cells = [float(x) for x in os.environ.get("PSGSDF_TIME_COMPARE_CELLS", "1,2,4").split(",")]
say = lambda *a: print(*a, file=sys.stderr, flush=True)
say(f"scene {N}^3, {F} keyframes ...")
sc = synth.make_scene(N=N, F=F, W=320, H=240, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
vs = float(np.float32(eng.info().voxel_size))
xyz, nrm, rgb, faces, _ = eng.extract_mesh_indexed()
ref = (xyz.astype(np.float64) + 0.3 * vs * nrm.astype(np.float64)).astype(np.float32)
say(f"mesh: {len(xyz)} vertices, {len(faces)} faces")
eng.compare_reference(ref, faces)      # (warm-up: code objects, pinned slots)
t0 = time.perf_counter()
for _ in range(reps):
    eng.extract_mesh_indexed()
t_mesh = (time.perf_counter() - t0) / reps
GROUPS = {"grid_build": ("compare_total", "compare_count", "compare_fill"), "query_to_reference": ("compare_query_ref",), "query_to_reconstruction": ("compare_query_rec",),
          "statistics": ("compare_stats",)}
stat = lambda v: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
out = {}
eng.set_profiling(True)
for cell in cells:
    ms = {g: [] for g in GROUPS}; wall = []
    for _ in range(reps):
        before = eng.kernel_times()
        t0 = time.perf_counter()
        r = eng.compare_reference(ref, faces, grid_cell=cell * vs)
        wall.append(1e3 * (time.perf_counter() - t0))
        after = eng.kernel_times()
        for g, names in GROUPS.items():
            ms[g].append(sum(after.get(n, (0.0, 0))[0] - before.get(n, (0.0, 0))[0] for n in names))
    last = eng.get_tuning()["last_compare"]
    say(f"cells of {cell:g} vs done")
    out[f"{cell:g}vs"] = {"kernel_ms": {g: stat(v) for g, v in ms.items()}, "call_wall_ms_profiling": stat(wall),
                          "pairs_per_query": [round(p / max(q, 1), 1) for p, q in zip(last["pairs"], last["queries"])],
                          "mean_vs": [round(r[s]["mean"] / vs, 5) for s in ("to_reference", "to_reconstruction")], "fscore": r["fscore"]}
eng.set_profiling(False)
wall = []
for _ in range(reps):      # the whole call as a user sees it: no events between the launches
    t0 = time.perf_counter()
    eng.compare_reference(ref, faces)
    wall.append(1e3 * (time.perf_counter() - t0))
print(json.dumps({"grid": list(eng.info().dim), "keyframes": F, "vertices": len(xyz), "faces": len(faces), "extract_mesh_indexed_ms": round(1e3 * t_mesh, 3),
                  "compare_reference_ms": stat(wall), "per_cell": out}))
