"""Cost of the hole filling (include/psgsdf_fill.h) on a synthetic SH1 scene on an N^3 grid, after one iteration: psgsdf_fill_voxels and
psgsdf_extract_mesh_filled for a few (rounds, sweeps), next to psgsdf_extract_mesh_components on the same state.  Wall-clock per call (host clock; every
call ends in a stream synchronise), then in a second pass the kernels' own event-timed ms per launch from psgsdf_kernel_times, and from them the
bytes per second the sweep kernel achieves: per filled voxel and sweep it reads 6 neighbour codes and 7 floats per known neighbour and writes 7 floats.
    python tools/time_fill.py N [reps]
For the kernel times of record run it under the tracer in a run of its own, with no counters in it:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_fill.py 256
(kernel names: k_fill_box_part, k_fill_round, k_fill_flags, k_fill_list, k_fill_sweep, k_fill_pack, k_fill_scatter, k_wmesh_filled)."""
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
CASES = ((2, 0), (2, 4), (6, 16), (16, 64))
sc = synth.make_scene(N=N, F=8, W=320, H=240, model="SH1")
eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
dim = [int(x) for x in eng.info().dim]
calls = [("extract_mesh_components", eng.extract_mesh_components)]
for R, K in CASES:
    calls.append((f"fill_voxels_R{R}_K{K}", lambda R=R, K=K: eng.fill_voxels(R, K)))
    calls.append((f"extract_mesh_filled_R{R}_K{K}", lambda R=R, K=K: eng.extract_mesh_filled(R, K)))
first = {name: call() for name, call in calls}      # (warm-up: code objects, allocations)
wall = {}
for name, call in calls:      # wall-clock first, without the event pair around every launch
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall[name + "_ms"] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
kernels, sweep = {}, {}
eng.set_profiling(True)
for R, K in CASES:      # one case at a time: the launches of a case are averaged among themselves
    eng.reset_kernel_times()
    for _ in range(reps):
        eng.extract_mesh_filled(R, K)
    kt = eng.kernel_times()
    kernels[f"R{R}_K{K}"] = {k: round(ms / max(n, 1), 4) for k, (ms, n) in kt.items() if k.startswith("fill_") or k in ("wmesh_filled", "wmesh_mark", "wmesh_verts", "wmesh_faces")}
    if K:
        # the bytes of one sweep: per list entry 6 codes and 7 floats out, per known neighbour 7 floats in
        lin = first[f"fill_voxels_R{R}_K{K}"]["lin"]
        known = np.zeros(dim[0] * dim[1] * dim[2], bool); known[lin] = True
        known |= eng.download_volume()["weight"] > 0
        i, j, k = lin % dim[0], (lin // dim[0]) % dim[1], lin // (dim[0] * dim[1])
        nb = 0
        for a, (p, n, stride) in enumerate(((i, dim[0], 1), (j, dim[1], dim[0]), (k, dim[2], dim[0] * dim[1]))):
            nb += int(known[(lin - stride)[p > 0]].sum()) + int(known[(lin + stride)[p < n - 1]].sum())
        nbytes = len(lin) * (6 * 4 + 7 * 4) + nb * 7 * 4
        ms = kt["fill_sweep"][0] / max(kt["fill_sweep"][1], 1)
        sweep[f"R{R}_K{K}"] = {"filled": int(len(lin)), "known_neighbours": nb, "bytes": nbytes, "ms": round(ms, 4), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
eng.set_profiling(False)
mesh = {name: {"vertices": int(len(first[name]["xyz"])), "faces": int(len(first[name]["faces"])), "boundary_edges": int(first[name]["components"]["n_boundary_edges"].sum())}
        for name in first if name.startswith("extract_mesh")}
print(json.dumps({"grid": dim, "reps": reps, **wall, "kernel_ms_per_launch": kernels, "sweep": sweep, "mesh": mesh,
                  "filled_voxels": {name: int(len(first[name]["lin"])) for name in first if name.startswith("fill_voxels")}}))
