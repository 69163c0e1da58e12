"""Cost of the alignment of a reference (include/psgsdf_align.h, csrc/align.hip): a synthetic SH1 scene on an N^3 grid with F keyframes, one
iteration, and its own welded mesh displaced by 0.3 voxels along the vertex normals (same faces), then rotated by 3 degrees about (0.3, -0.5, 0.8)
through the vertex mean and shifted by 1.5 voxels, as the reference.  Both directions.  Per repetition (default 5; median and range are printed):
the kernels' event-timed ms per call and per evaluation -- the grids (k_cmp_total, k_cmp_cells twice; built once per call), the moves (k_aln_move),
the search each way (k_cmp_query), the rows each way (k_aln_rows), the fold (k_aln_fold) -- then, without events between the launches, the whole
call's wall time and the wall time per evaluation, and the mean number of candidate pairs a query evaluates each way (psgsdf_get_tuning
"last_align").
    python tools/time_align.py N F [reps]
"""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
say = lambda *a: print(*a, file=sys.stderr, flush=True)
say(f"scene {N}^3, {F} keyframes ...")
sc = synth.make_scene(N=N, F=F, W=320, H=240, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
vs = float(np.float32(eng.info().voxel_size))
xyz, nrm, rgb, faces, _ = eng.extract_mesh_indexed()
say(f"mesh: {len(xyz)} vertices, {len(faces)} faces")


def rotation(axis, degrees):
    w = np.asarray(axis, np.float64); w = w / np.linalg.norm(w) * np.deg2rad(degrees)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


X = xyz.astype(np.float64) + 0.3 * vs * nrm.astype(np.float64)
c = xyz.astype(np.float64).mean(0)
ref = ((X - c) @ rotation((0.3, -0.5, 0.8), 3.0).T + c + 1.5 * vs * np.array([1.0, -2.0, 2.0]) / 3.0).astype(np.float32)
first = eng.align_reference(ref, faces)      # (warm-up: code objects, pinned slots)
say(f"status {first['status']} after {first['n_iters']} steps, rms {first['iters'][0]['rms'] / vs:.3f} -> {first['final']['rms'] / vs:.3f} vs")
GROUPS = {"grid_build": ("compare_total", "compare_count", "compare_fill"), "move": ("align_move",), "query_1": ("align_query_1",), "query_2": ("align_query_2",),
          "rows_1": ("align_rows_1",), "rows_2": ("align_rows_2",), "fold": ("align_fold",)}
stat = lambda v: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
ms = {g: [] for g in GROUPS}; wall_prof = []
eng.set_profiling(True)
for _ in range(reps):
    before = eng.kernel_times()
    t0 = time.perf_counter()
    r = eng.align_reference(ref, faces)
    wall_prof.append(1e3 * (time.perf_counter() - t0))
    after = eng.kernel_times()
    for g, names in GROUPS.items():
        ms[g].append(sum(after.get(n, (0.0, 0))[0] - before.get(n, (0.0, 0))[0] for n in names))
eng.set_profiling(False)
last = eng.get_tuning()["last_align"]
evals = last["evaluations"]
wall = []
for _ in range(reps):      # the whole call as a user sees it: no events between the launches
    t0 = time.perf_counter()
    eng.align_reference(ref, faces)
    wall.append(1e3 * (time.perf_counter() - t0))
t0 = time.perf_counter()
for _ in range(reps):
    eng.align_reference(ref, faces, max_iters=0)      # the mesh, the upload, the grids and ONE evaluation
t_one = 1e3 * (time.perf_counter() - t0) / reps
print(json.dumps({"grid": list(eng.info().dim), "keyframes": F, "vertices": len(xyz), "faces": len(faces), "status": r["status"], "iterations": r["n_iters"], "evaluations": evals,
                  "rms_vs": [round(it["rms"] / vs, 6) for it in r["iters"]] + [round(r["final"]["rms"] / vs, 6)],
                  "last_steps_rad_vs": [[float("%.3g" % np.linalg.norm(it["step"][:3])), float("%.3g" % (np.linalg.norm(it["step"][3:]) / vs))] for it in r["iters"][-3:]],
                  "kernel_ms_per_call": {g: stat(v) for g, v in ms.items()},
                  "kernel_ms_per_evaluation": {g: stat([x / evals for x in v]) for g, v in ms.items() if g != "grid_build"},
                  "pairs_per_query": [round(p / max(q, 1), 1) for p, q in zip(last["pairs"], last["queries"])],
                  "call_wall_ms": stat(wall), "call_wall_ms_profiling": stat(wall_prof), "one_evaluation_call_wall_ms": round(t_one, 3),
                  "wall_ms_per_evaluation": round((float(np.median(wall)) - t_one) / max(evals - 1, 1), 3)}))
