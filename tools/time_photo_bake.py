"""Cost of the albedo texture solved from the keyframes (include/psgsdf_photo.h) on the bench scene: a 256^3 synthetic SH1 scene with 50 keyframes of
640 x 480, level-of-detail cell 4 voxels, 8 texels along an edge.  k_photo_pairs' and k_photo_solve's event-timed ms per call from psgsdf_kernel_times,
as median and range over the repetitions, the (texel, keyframe) pairs per second of the pair kernel -- all of them, and those that reach the ray
(used + occluded + dark: the others end at the projection or the angle) -- and the wall-clock of the whole call next to psgsdf_bake_lod's.
Next to it, on the same context, relight's rays per second for one point light with one shadow ray per lit pixel (keyframe 0's view; k_relight: the
same walk without the projection and the shading), the figure the pair rate is read against:
    python tools/time_photo_bake.py [grid] [keyframes] [reps]
For the kernel times of record run it under the tracer in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_photo_bake.py 256
(kernel names: k_photo_pairs<MODEL>, k_photo_solve<MODEL, IMG>, k_relight<KIND>)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from psgradientsdf_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
N = int(args[0]) if len(args) > 0 else 256
F = int(args[1]) if len(args) > 1 else 50
reps = int(args[2]) if len(args) > 2 else 5
CELL, R = 4, 8
sc = synth.make_scene(N=N, F=F, W=640, H=480, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
vs = float(np.float32(eng.info().voxel_size))


def stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(names, call):
    """the event-timed ms of the launches of the kernels `names` inside call()"""
    before = eng.kernel_times()
    out = call()
    after = eng.kernel_times()
    return [after[k][0] - before.get(k, (0.0, 0))[0] for k in names], out


photo = lambda: eng.bake_lod_photo(CELL * vs, R)
P0 = eng.download_poses()[0].reshape(4, 4).astype(np.float64)
lamp = dict(kind="point", vec=[float(x) for x in (P0[:3, 3] + 0.4 * np.linalg.norm(P0[:3, 3]) * P0[:3, 0])], samples=1)
photo(); eng.relight([lamp], frame=0)                        # (warm-up: code objects, allocations)
eng.set_profiling(True)
pairs_ms, solve_ms, relight_ms = [], [], []
for _ in range(reps):                                        # interleaved: both see the same clocks and cache state
    (tp, ts), got = timed(("k_photo_pairs", "k_photo_solve"), photo)
    (tr,), lit = timed(("k_relight",), lambda: eng.relight([lamp], frame=0))
    pairs_ms.append(tp); solve_ms.append(ts); relight_ms.append(tr)
eng.set_profiling(False)
k, rl = got["counts"], lit["counts"][0]
walked = k["n_used"] + k["n_occluded"] + k["n_dark"]
med_p, med_r = float(np.median(pairs_ms)), float(np.median(relight_ms))
res = {"grid": N, "keyframes": F, "cell_voxels": CELL, "R": R, "library": os.path.relpath(capi.ENGINE_LIB), "atlas": [got["width"], got["height"]], "faces": len(got["faces"]),
       "counts": k, "k_photo_pairs_ms": stat(pairs_ms), "k_photo_solve_ms": stat(solve_ms),
       "pairs_per_s": round(k["n_pairs"] / (1e-3 * med_p)), "walked_pairs": walked, "walked_pairs_per_s": round(walked / (1e-3 * med_p)),
       "pairs_per_s_both_kernels": round(k["n_pairs"] / (1e-3 * (med_p + float(np.median(solve_ms))))),
       "relight_point_K1": {"k_relight_ms": stat(relight_ms), **rl, "rays_per_s": round(rl["n_rays"] / (1e-3 * med_r))}}
# wall-clock of the whole calls (host clock; each ends in a stream synchronise): welded mesh, clusters, bake, downloads -- and the photo map on top
for name, call in (("bake_lod_wall_ms", lambda: eng.bake_lod(CELL * vs, R)), ("bake_lod_photo_wall_ms", photo)):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); wall.append(1e3 * (time.perf_counter() - t0))
    res[name] = stat(wall)
print(json.dumps(res))
