"""Cost of view rendering (include/psgsdf_render.h) on the headline scene: one keyframe view with every plane, and the per-keyframe report over all
keyframes.  Wall-clock per call (host clock around calls that end in a stream synchronise) and the kernels' own times from psgsdf_kernel_times:
    python tools/time_render.py [grid] [frames] [reps]
For the kernel times of record run it under the tracer in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_render.py 256 50
(kernel names: k_render_bricks, k_render<MODEL, IMG>, k_render_report<MODEL, IMG>, k_render_fold)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from psgradientsdf_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 50
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
sc = synth.make_scene(N=N, F=F, W=640, H=480, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.render(frame=0)
eng.render_report()                                         # (warm-up: code objects, allocations)
eng.reset_kernel_times()
eng.set_profiling(True)
t0 = time.perf_counter()
for _ in range(reps):
    r = eng.render(frame=0)
t_view = (time.perf_counter() - t0) / reps
t0 = time.perf_counter()
for _ in range(reps):
    rows = eng.render_report()
t_rep = (time.perf_counter() - t0) / reps
kt = eng.kernel_times()
eng.set_profiling(False)
st = r["stats"]
print(json.dumps({"grid": N, "keyframes": F, "size": [640, 480], "view_ms": round(1e3 * t_view, 3), "report_ms": round(1e3 * t_rep, 3),
                  "kernel_ms_per_launch": {k: round(ms / max(n, 1), 4) for k, (ms, n) in kt.items() if k.startswith("k_render")},
                  "hits_frame0": st["n_hits"], "off_band_frame0": st["n_hits_off_band"],
                  "mean_rmse": sum((sum(q["sum_r2"]) / max(3 * q["n_hits"], 1)) ** 0.5 for q in rows) / len(rows)}))
