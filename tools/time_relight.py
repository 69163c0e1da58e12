"""Cost of relighting (include/psgsdf_relight.h) on the headline scene: a 256^3 synthetic SH1 scene, keyframe 0's view at 640 x 480, under one
directional light with 1, 16 and 64 shadow rays per lit pixel and one point light with 16 (and the directional light turned away from every hit:
the cost of the idle lanes alone).  k_relight's event-timed ms per launch (one launch per
light and call) from psgsdf_kernel_times, as median and range over the repetitions, and rays per second, then the wall-clock of the whole call; next to it k_render's time per view on the
same context (the primary pass of every relight call is that kernel):
    python tools/time_relight.py [grid] [reps]
    python tools/time_relight.py render [grid] [reps]      k_render alone, for an A/B of two builds of the library (PSGSDF_ENGINE_LIB): alternate the runs
Compare the rays per second with k_occlusion's, the same walk (tools/time_mesh.py, "ambient_occlusion_4vs_R8"), measured in the same session.
For the kernel times of record run it under the tracer in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_relight.py 256
(kernel names: k_render_bricks, k_render<MODEL, IMG>, k_relight<KIND>)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from psgradientsdf_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
render_only = bool(args) and args[0] == "render"
if render_only:
    args = args[1:]
N = int(args[0]) if len(args) > 0 else 256
reps = int(args[1]) if len(args) > 1 else 5
sc = synth.make_scene(N=N, F=4, W=640, H=480, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
vs = float(np.float32(eng.info().voxel_size))


def stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(name, call):
    """the event-timed ms of the one launch of kernel `name` inside call()"""
    before = eng.kernel_times().get(name, (0.0, 0))
    out = call()
    after = eng.kernel_times()[name]
    assert after[1] == before[1] + 1, (name, before, after)
    return after[0] - before[0], out


eng.render(frame=0)                                          # (warm-up: code objects, allocations)
eng.set_profiling(True)
k_render = [timed("k_render", lambda: eng.render(frame=0))[0] for _ in range(max(reps, 5))]
res = {"grid": N, "size": [640, 480], "library": os.path.relpath(capi.ENGINE_LIB), "k_render_ms": stat(k_render)}
if not render_only:
    P0 = eng.download_poses()[0].reshape(4, 4).astype(np.float64)
    eye, fwd, right = P0[:3, 3], P0[:3, 2], P0[:3, 0]
    sun = [float(x) for x in (-fwd + 0.8 * right - 0.3 * P0[:3, 1])]
    lamp = [float(x) for x in (eye + 0.4 * np.linalg.norm(eye) * right)]
    cases = [("directional_K1", dict(kind="directional", vec=sun, samples=1)), ("directional_K16", dict(kind="directional", vec=sun, samples=16, spread=0.05)),
             ("directional_K64", dict(kind="directional", vec=sun, samples=64, spread=0.05)), ("point_K16", dict(kind="point", vec=lamp, samples=16, spread=2 * vs)),
             # every hit unlit: what the wavefronts of missed and unlit pixels cost (the launch has the lanes of K = 64, none of them walks)
             ("directional_K64_all_unlit", dict(kind="directional", vec=[float(x) for x in fwd], samples=64, spread=0.05))]
    for _, L in cases:
        eng.relight([L], frame=0)                            # (warm-up of every instance)
    ms = {name: [] for name, _ in cases}
    for _ in range(reps):
        for name, L in cases:                                # interleaved: every case sees the same clocks and cache state
            t, r = timed("k_relight", lambda: eng.relight([L], frame=0))
            ms[name].append(t)
            ms.setdefault(name + "_counts", r["counts"][0])
    res["relight"] = {}
    for name, _ in cases:
        cn = ms[name + "_counts"]
        med = float(np.median(ms[name]))
        res["relight"][name] = {"k_relight_ms": stat(ms[name]), **cn, "rays_per_s": round(cn["n_rays"] / (1e-3 * med))}
    res["hit_share"] = round(cn["n_hits"] / (640 * 480), 4)
    res["kernel_ms_per_launch"] = {k: round(t / max(n, 1), 4) for k, (t, n) in eng.kernel_times().items() if k.startswith(("k_relight", "k_render"))}
    eng.set_profiling(False)
    # wall-clock of the whole call (host clock; the call ends in a stream synchronise): brick map, primary pass, list, one light, downloads
    for name, L in cases:
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.relight([L], frame=0)
            wall.append(1e3 * (time.perf_counter() - t0))
        res["relight"][name]["call_ms"] = stat(wall)
    t0 = time.perf_counter()
    eng.relight([L for _, L in cases[:4]], frame=0)
    res["call_4_lights_ms"] = round(1e3 * (time.perf_counter() - t0), 4)
eng.set_profiling(False)
print(json.dumps(res))
