"""Cost of the welded mesh (include/psgsdf_mesh.h) against the non-indexed one (psgsdf_extract_mesh) on the same state, the sizes of both, and the cost of
the welded mesh with its connected components labelled and filtered (psgsdf_extract_mesh_components; it repeats the welded extraction), and the cost
and sizes of the level-of-detail mesh at cells of 2 and 4 voxels, without and with keep_largest = 1 (psgsdf_extract_mesh_lod; it repeats both).
Then the photometric fit (include/psgsdf_fit.h): psgsdf_band_fit next to psgsdf_energy (the same gathers and arithmetic: k_band_fit stores 24 B per row
where k_energy reduces) and psgsdf_extract_mesh_fit next to psgsdf_extract_mesh_indexed (it adds k_band_fit and k_wmesh_fit).
Then the detail maps (include/psgsdf_bake.h): psgsdf_bake_lod at the same cells with 8 texels along an edge (it repeats the level-of-detail call and adds
k_render_bricks and k_bake), its atlas sizes and counts.
Then ambient occlusion (include/psgsdf_occlusion.h): psgsdf_bake_lod_ao at a cell of 4 voxels, 8 texels along an edge, 16 and 64 rays per texel, radius 8
voxels, bias 1 voxel: k_occlusion's event-timed ms per launch and rays per second, with the walk cut at the radius and -- alternating in the same run,
on a second context created under PSGSDF_AO_CUT=0 and brought to the same state -- without the cut (the same bits), each as median and range over the
repetitions (synthetic scenes only).
Wall-clock per call (host clock; both calls end in a stream synchronise) and the kernels' own times from psgsdf_kernel_times:
    python tools/time_mesh.py sokrates [reps]      the sokrates fixture fused at its poses (128^3 at 4 mm), one iteration
    python tools/time_mesh.py N [reps]             a synthetic SH1 scene on an N^3 grid
For the kernel times of record run it under the tracer in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_mesh.py 256
(kernel names: k_wmesh_mark, k_wmesh_faces, k_wmesh_verts, k_wmesh_or (multi-rank only) against k_mc_count, k_mc_emit; both share k_box_*, k_cscan_*;
the components: k_mcomp_init, _hook, _flatten, _edges, _vstats, _fstats, _ecount, and with a filter that drops something _keep, _compact;
the level of detail: k_mlod_cluster, _ftable, _fkeep, _vflag, _emit -- one launch of each per call, so their averages mix the two cell sizes:
PSGSDF_TIME_MESH_LOD=2 or =4 restricts the run to one of them (k_bake's average likewise); the fit: k_band_fit against k_energy, k_wmesh_fit against k_wmesh_verts)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from psgradientsdf_amd import capi, synth  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "256"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
if what == "sokrates":
    from test_render_gpu import _load_multiview
    K, color, depth, poses = _load_multiview(os.path.join(ROOT, "tests", "golden", "sokrates_small"))
    F, vs = len(poses), 0.004
    ys, xs = np.nonzero(depth[0] > 0)
    z = depth[0][ys, xs].astype(np.float64)
    pc = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], 1)
    centre = (pc @ poses[0][:3, :3].T.astype(np.float64) + poses[0][:3, 3]).mean(0)
    g = capi.GridDesc(); g.dim[:] = [128, 128, 128]; g.voxel_size = vs; g.shift[:] = [float(x) for x in centre]; g.truncation = 5 * vs
    eng = capi.load_engine(g, K.reshape(-1), capi.default_settings(capi.SH1), 0)
    eng.volume_init(F)
    for f in range(F):
        eng.integrate_frame(color[f], depth[f], eng.estimate_normals(depth[f]), poses[f], f, z_min=0.5, z_max=3.5)
    eng.set_keyframes(np.arange(F, dtype=np.int32), np.stack(color), np.stack(poses).reshape(F, 16))
    eng.init()
else:
    N = int(what)
    sc = synth.make_scene(N=N, F=8, W=320, H=240, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.load_scene(sc)
eng.init_albedo()
eng.iterate(capi.ALL, 1)
xn, _ = eng.extract_mesh()
xyz, nrm, rgb, faces, _ = eng.extract_mesh_indexed()                   # (warm-up: code objects, allocations)
comps = eng.extract_mesh_components(keep_largest=1)["components"]
vs = float(np.float32(eng.info().voxel_size))
lod_cells = [int(x) for x in os.environ.get("PSGSDF_TIME_MESH_LOD", "2,4").split(",")]
lod_sizes = {}
for s in lod_cells:
    for name, flt in (("all", {}), ("keep_largest_1", {"keep_largest": 1})):
        m = eng.extract_mesh_lod(s * vs, **flt)
        lod_sizes[f"{s}vs_{name}"] = {"vertices_in": m["n_vertices_in"], "faces_in": m["n_faces_in"], "vertices": len(m["xyz"]), "faces": len(m["faces"]),
                                      "ply_body_bytes": 27 * len(m["xyz"]) + 13 * len(m["faces"])}
bake_sizes = {}
for s in lod_cells:
    b = eng.bake_lod(s * vs, 8)
    bake_sizes[f"{s}vs"] = {"faces": len(b["faces"]), "width": b["width"], "height": b["height"], **{k: b[k] for k in ("n_texels", "n_hits", "n_hits_off_band", "n_buried", "n_misses")}}
eng.energy(); eng.band_fit(); fit = eng.extract_mesh_fit()
eng.reset_kernel_times()
eng.set_profiling(True)
t0 = time.perf_counter()
for _ in range(reps):
    eng.extract_mesh()
t_plain = (time.perf_counter() - t0) / reps
t0 = time.perf_counter()
for _ in range(reps):
    eng.extract_mesh_indexed()
t_idx = (time.perf_counter() - t0) / reps
t_cc = {}
for name, flt in (("all", {}), ("keep_largest_1", {"keep_largest": 1})):      # everything kept: no compaction; one kept: k_mcomp_keep, two scans, k_mcomp_compact
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.extract_mesh_components(**flt)
    t_cc[name] = (time.perf_counter() - t0) / reps
t_lod = {}
for s in lod_cells:
    for name, flt in (("all", {}), ("keep_largest_1", {"keep_largest": 1})):
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.extract_mesh_lod(s * vs, **flt)
        t_lod[f"{s}vs_{name}"] = (time.perf_counter() - t0) / reps
t_bake = {}
for s in lod_cells:
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.bake_lod(s * vs, 8)
    t_bake[f"{s}vs"] = (time.perf_counter() - t0) / reps
t_fit = {}
for name, call in (("energy_ms", eng.energy), ("band_fit_ms", eng.band_fit), ("extract_mesh_fit_ms", eng.extract_mesh_fit)):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    t_fit[name] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
kt = eng.kernel_times()
ao = {}
if what != "sokrates":
    os.environ["PSGSDF_AO_CUT"] = "0"      # (read when a context is created)
    uncut = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    del os.environ["PSGSDF_AO_CUT"]
    uncut.load_scene(sc); uncut.init_albedo(); uncut.iterate(capi.ALL, 1)
    uncut.bake_lod_ao(4 * vs, 8, None, 16, 8 * vs, vs)      # (warm-up)
    uncut.set_profiling(True)
    for K in (16, 64):
        ms = {"cut": [], "no_cut": []}
        for _ in range(reps):
            for name, e in (("cut", eng), ("no_cut", uncut)):      # alternating: both see the same clocks and cache state
                before = e.kernel_times().get("occlusion", (0.0, 0))
                b = e.bake_lod_ao(4 * vs, 8, None, K, 8 * vs, vs)
                after = e.kernel_times()["occlusion"]
                assert after[1] == before[1] + 1
                ms[name].append(after[0] - before[0])
        cn = b["counts"]
        ao[f"K{K}"] = {"texels": cn["n_samples"], "rays": cn["n_rays"], "occluded": cn["n_occluded"], "buried": cn["n_buried"],
                       **{f"k_occlusion_ms_{n}": {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()},
                       **{f"rays_per_s_{n}": round(cn["n_rays"] / (1e-3 * float(np.median(v)))) for n, v in ms.items()}}
    uncut.set_profiling(False)
eng.set_profiling(False)
V, Fc = len(xyz), len(faces)
print(json.dumps({"state": what, "grid": list(eng.info().dim), "extract_mesh_ms": round(1e3 * t_plain, 3), "extract_mesh_indexed_ms": round(1e3 * t_idx, 3),
                  "extract_mesh_components_ms": {k: round(1e3 * v, 3) for k, v in t_cc.items()},
                  "extract_mesh_lod_ms": {k: round(1e3 * v, 3) for k, v in t_lod.items()}, "lod": lod_sizes,
                  "bake_lod_ms": {k: round(1e3 * v, 3) for k, v in t_bake.items()}, "bake": bake_sizes, "ambient_occlusion_4vs_R8": ao,
                  "kernel_ms_per_launch": {k: round(ms / max(n, 1), 4) for k, (ms, n) in kt.items() if k.startswith(("mc_", "wmesh_", "mcomp_", "mlod_")) or k in ("band_fit", "energy", "bake", "k_render_bricks")},
                  **t_fit, "fit": {"n_band": int(eng.info().n_band), "vertex_observations": int(fit["n_obs"].sum()), "vertices_observed": int((fit["n_obs"] > 0).sum())},
                  "faces": Fc, "components": len(comps), "largest_component_faces": int(comps["n_faces"].max()) if len(comps) else 0, "vertices_indexed": V, "vertices_non_indexed": len(xn),
                  "indexed_ply_body_bytes": 27 * V + 13 * Fc}))
