#!/usr/bin/env python3
"""bench.py — Gauss-Newton iterations/sec of the full photometric-stereo sweep (BASELINE.json metric).

One "step" = one body of the alternation loop (albedo, light, distance, pose blocks, the four PS-energy
evaluations and the convergence / divergence test; PsOptimizer.cpp:303-384) on the synthetic 256^3 x 50-keyframe
scene, inputs resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

`value` is the PRODUCT loop, psgsdf_optimize -- what voxelPS calls: the host takes the stop decision after every iteration
(VERDICT r02 item 5).  The K timed steps are iterations W+1 .. W+K of one psgsdf_optimize call, bracketed through its per-iteration
callback (device drained + barrier on both sides).

A plain run does what `value` needs and nothing else: it synthesises the scene, warms up, times the K steps (one repetition unless --reps
says otherwise), writes the outputs if asked to and prints the line.  `--full` adds everything else the benchmark measures: the same scene
through psgsdf_iterate (no stop decision, nothing to wait for: `iterate_ms_per_step`), five repetitions by default, the kernel breakdown,
the roofline of the dominant kernel (with live rocprofv3 counter passes), the CPU baseline, and the LED (configs[3]) / SH2 workloads and the
others as `extra`; on N > 1 ranks the full-size check and the weak-scaling and configs[4] runs.  What a plain run spends outside its steps grows
with K: the loop ends itself after ~18 iterations, so every ~15 timed steps take a fresh context (~20 ms at 256^3 x 50 keyframes: allocation, upload, set-up).

`--dump-outputs DIR` writes what the timed loop hands its caller after the last timed step, as DIR/<name>.npy: `dist`, `grad` (3 x S) and
`albedo` (3 x S) at the band voxels (float32), `band_index` (their linear voxel indices, float64), `poses` (F x 16) and `light` (float32), and
`records` (float64, one row per timed step: the REC_FIELDS below, then e_after[0..3]).  The inputs are seeded: the same arguments give the same
inputs in every run.  More than 64 MB in all: a fixed, seeded sample of the band voxels.  On N > 1 ranks every rank writes its own slab's
arrays as <name>_rank<r>.npy.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--reps R] [--grid 256] [--frames 50] [--model SH1] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` without a launcher (WORLD_SIZE unset) starts the N ranks itself, one process per device; with fewer than N devices visible it exits
non-zero (PSGSDF_BENCH_SHARE_GPU=1: all ranks on GPU 0 over the gloo test transport -- a functional check, not a measurement).  The line never
reports an n_gpus other than --gpus.  `value` is the MEDIAN over R repetitions of the K-step bracket (fresh contexts each; R = --reps, default 1, 5 with --full), `spread` their min / max.

N > 1: `value` = STRONG scaling of the metric's own problem -- the ONE 256^3 volume with its 50 keyframes cut into N z-slabs of equal
band count, one process per GPU, every rank synthesising and uploading only its own planes -- it/s of that one job (`scaling: "strong"`).  With
--full the line carries, as `extra`, the weak-scaling run (`extra.weak`: N copies of the scene stacked along z, 50*N keyframes, N x it/s -- round 4's
default, `--weak` makes it `value` again) and BASELINE configs[4] (`extra.configs4_strong`: 512^3, SH2, 100 keyframes cut into N slabs; `--strong`
alone makes it `value`), each with its own pre-timing self-check and `degraded` flag.  The engine's C++ host runs the slab loop natively; Python only
launches the ranks, hands the RCCL id around and takes the time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from psgradientsdf_amd import capi, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md


PMC_NAMES = {"k_cgf_solve": "pcg_solve", "k_cgp_solve": "pcg_solve", "k_cgf_pass": "pcg_pass", "k_cgf_init": "pcg_init", "k_sweep_dist": "sweep_dist", "k_sweep_pose": "sweep_pose",
             "k_sweep_light": "sweep_light", "k_sweep_albedo": "sweep_albedo", "k_energy": "energy", "k_assemble": "assemble", "k_derive": "derive",
             "k_frames_eigen": "solve_frames_eigen"}


def live_traffic(args):
    """HBM-side bytes per launch of the bench kernels, measured IN THIS RUN: two short child runs of this very command under
    `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes, counters only -- no tracing domain next to them), 4 iterations each, corrected as
    /opt/skills/guides/MI355X_MICROARCH.md prescribes (both counters in KiB; gfx950 tallies a 128-byte fetch as 64: FETCH_SIZE x 2).  None where rocprofv3
    is missing, the run is itself being profiled, or PSGSDF_BENCH_LIVE_PMC=0 -- the line then falls back to the archived summary under its own label."""
    import csv, re, shutil, subprocess, tempfile
    from collections import defaultdict
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if (not exe or os.environ.get("PSGSDF_BENCH_LIVE_PMC") == "0" or os.environ.get("PSGSDF_BENCH_CHILD") == "1"
            or "rocprof" in os.environ.get("LD_PRELOAD", "") or os.environ.get("ROCPROFILER_LIBRARY_CTOR") or os.environ.get("ROCP_TOOL_LIBRARIES")):
        return None
    t0 = time.perf_counter()
    res = {}
    tmp = tempfile.mkdtemp(prefix="psgsdf_pmc_", dir="/tmp")
    env = dict(os.environ, PSGSDF_BENCH_CHILD="1", PSGSDF_BENCH_NO_SOLVE_MODEL="1", TMPDIR="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "-d", d, "-o", "pmc", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--steps", "4", "--warmup", "1", "--reps", "1", "--full",
                   "--no-cpu-baseline", "--no-breakdown", "--no-extra", "--grid", str(args.grid), "--frames", str(args.frames), "--width", str(args.width), "--height", str(args.height), "--model", args.model]
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=float(os.environ.get("PSGSDF_BENCH_PMC_TIMEOUT_S", "240")))
            path = next((os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("counter_collection.csv")), None)
            if r.returncode != 0 or not path:
                return {"error": f"rocprofv3 --pmc {counter}: rc {r.returncode}, {r.stderr.decode(errors='replace')[-200:]}"}
            acc = defaultdict(list)
            with open(path) as f:
                for row in csv.DictReader(f):
                    mm = re.search(r"psg::(k_[a-z0-9_]+)", row.get("Kernel_Name", ""))
                    if row.get("Counter_Name") == counter and mm and mm.group(1) in PMC_NAMES:
                        acc[PMC_NAMES[mm.group(1)]].append(float(row["Counter_Value"]))
            res[counter] = {k: (sum(v) / len(v), len(v)) for k, v in acc.items() if v}
    except Exception as ex:      # (a side measurement: never takes the line down)
        return {"error": repr(ex)[:300]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for k in sorted(set(res.get("FETCH_SIZE", {})) | set(res.get("WRITE_SIZE", {}))):
        f, nf = res["FETCH_SIZE"].get(k, (0.0, 0)); w, _ = res["WRITE_SIZE"].get(k, (0.0, 0))
        kernels[k] = {"hbm_bytes_per_launch": (2.0 * f + w) * 1024.0, "launches": nf, "fetch_size_kib_raw": f, "write_size_kib_raw": w}
    return {"kernels": kernels, "seconds": round(time.perf_counter() - t0, 1),
            "how": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (two passes, counters only) around 4 iterations of this command, spawned by this run; FETCH_SIZE x2 (gfx950), KiB -> bytes; Infinity-Cache hits are counted"}


def algorithmic_bytes(kernel, S, n_obs, W, H, F, laplacian=False, pcg_passes=1.0):
    """Algorithmic HBM bytes of ONE launch: per band voxel B_v = 60 B of state
    (dist 4, grad 12, rgb 12, vis 8, 3 stencil-neighbour dists 12, 3 row lookups 12; +12 with the Laplacian),
    image taps U_img = min(48 B * n_obs, 12 B * W*H*F) and the kernel's per-voxel output."""
    B_v = 60 + (12 if laplacian else 0) + (8 if F > 64 else 0)
    U = min(48 * n_obs, 12 * W * H * F)
    table = {
        "sweep_albedo": S * B_v + U + 24 * S,
        "sweep_light": S * B_v + U,
        "sweep_pose": S * B_v + U,
        "sweep_dist": S * B_v + U + 56 * S,
        "energy": S * B_v + U,
        "pcg_solve": 124 * S * pcg_passes,   # the persistent solve: ONE launch runs all passes of a solve (B_cg = 124 B per band voxel per PCG iteration)
        "pcg_pass": 124 * S,    # B_cg = 124 B per band voxel per PCG iteration (block 40 + 3 nbr rows 12 + gather p 16 + scatter Ap 16 + 5 vector streams 40)
        "assemble": (56 + 80 + 12) * S,
        "derive": (4 + 12 + 24 + 36 + 12) * S,
    }
    return table.get(kernel)


def timed_optimize(make_engine, torch, dist, steps, warmup, reps=1, before_timed=None, after_call=None, on_last=None):
    """`reps` repetitions of: K = `steps` iterations of the product loop psgsdf_optimize, bracketed by device synchronisation (+ barrier over the
    ranks) on both sides.  The loop leaves on its own when the energy stops falling (the reference's divergence exit, PsOptimizer.cpp:377-384; ~18
    iterations on the headline scene), so: one UNTIMED call first (the warm-up: >= `warmup` iterations, and it tells how many iterations a call
    survives), then as many timed calls as needed, each on a FRESH context (psgsdf_optimize normalises the regulariser weights in place), each
    skipping its first iteration and ending ITSELF after its share of the K steps, before the divergence exit would.  The brackets are taken in a
    passive record observer (psgsdf_set_record_observer), so the loop being timed is the callback-free one with its speculative start of the next
    iteration.  on_last(engine, records of the repetition's timed iterations) sees the context of the last timed call before it is closed.
    Returns (list of elapsed seconds per repetition -- None if the loop does not survive 3 iterations --, records of the timed iterations
    of the first repetition, calls)."""
    import time as _t

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    eng = make_engine()
    recs0, _ = eng.optimize(capi.ALL, cap=warmup + steps + 8)
    sync()
    eng.close()
    survive = len(recs0) - 1                      # records a call delivers before it ends on its own (the terminating iteration is not reported)
    calls = 1
    if survive < 3:
        return None, recs0, calls
    elapsed_reps, first_recs = [], []
    for rep in range(reps):
        elapsed, timed = 0.0, []
        while len(timed) < steps:
            need = min(steps - len(timed), survive - 1)
            seg = {"t0": None, "t1": None, "recs": []}
            eng = make_engine()

            def on_record(done, rec, seg=seg, need=need, eng=eng, first=(rep == 0 and not timed)):
                if done == 1:
                    if before_timed and first:
                        before_timed(eng)
                    sync(); seg["t0"] = _t.perf_counter()
                    return False
                seg["recs"].append(rec)
                if done == 1 + need:
                    sync(); seg["t1"] = _t.perf_counter()
                    return True                   # end the loop here: this call's share of the K timed steps is done
                return False

            eng.set_record_observer(on_record)      # passive: psgsdf_optimize keeps its speculative start of the next iteration (no on_iter callback)
            eng.optimize(capi.ALL, cap=warmup + steps + 8)
            sync()
            if after_call:
                after_call(eng, calls - 1)
            if on_last and seg["t1"] is not None and rep == reps - 1 and len(timed) + len(seg["recs"]) >= steps:
                on_last(eng, timed + seg["recs"])
            eng.close()
            calls += 1
            if seg["t1"] is None:                   # the loop ended earlier than the untimed call did (cannot happen: same scene, same bits)
                return None, timed, calls
            elapsed += seg["t1"] - seg["t0"]; timed += seg["recs"]
        elapsed_reps.append(elapsed)
        if rep == 0:
            first_recs = timed
    return elapsed_reps, first_recs, calls


def attach_comm(eng, dist, rank, world, share):
    """attach a context to its rank: the engine's own RCCL communicator (the id travels through torch's process group), or -- all ranks sharing
    GPU 0 -- the caller-supplied gloo transport of the tests (RCCL refuses two ranks per device)"""
    if share:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _gloo_transport import GlooTransport
        eng._transport = GlooTransport(dist)
        eng.comm_init_ext(eng._transport.ops, rank, world)
    else:
        ident = [capi.comm_unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(ident, src=0)
        eng.comm_init(rank, world, ident[0])


def self_check(dist, rank, world, device, share, model="SH1", F=8):
    """Before anything is timed on N > 1 ranks: the N-rank slab run against a single-context run of the same small scene (64^3, two iterations;
    SH1 with 8 keyframes for the 256^3 workloads, SH2 with 70 keyframes -- two visibility words per voxel -- for configs[4]) on this rank's own
    device -- e_total to 1e-5 relative (SH2: 2e-4, the float32 9x9 light blocks).  A wrong exchange shows here, not as a fast wrong number."""
    sc = synth.make_scene(N=64, F=F, W=160 if F <= 16 else 96, H=120 if F <= 16 else 72, model=model)
    st = capi.default_settings(synth.MODELS[model])
    tol = 2e-4 if model == "SH2" else 1e-5
    eng = capi.load_engine(sc, sc.K, st, device)
    attach_comm(eng, dist, rank, world, share)
    eng.load_scene_slab(sc, rank, world)
    eng.init_albedo(); eng.normalize_weights()
    e_n = [float(r["e_total"]) for r in eng.iterate(capi.ALL, 2)]
    eng.close()
    ref = capi.load_engine(sc, sc.K, st, device)
    ref.load_scene(sc); ref.init_albedo(); ref.normalize_weights()
    e_1 = [float(r["e_total"]) for r in ref.iterate(capi.ALL, 2)]
    ref.close()
    rel = max(abs(a - b) / abs(b) for a, b in zip(e_n, e_1))
    worst = [None] * world
    dist.all_gather_object(worst, rel)
    rel = max(worst)
    return {"scene": f"64^3 x {F} keyframes, {model}, 2 iterations", "e_total_ranks": e_n, "e_total_single": e_1, "rel_diff": rel, "tol": tol, "ok": bool(rel <= tol)}


STATE_STATS = ("cross_rank_ready", "cross_rank_mem_kind")      # states, not counters: never summed over contexts

# --dump-outputs: the columns of records.npy (then e_after[0..3]) and the size cap of all arrays together
REC_FIELDS = ("e_total", "e_r", "e_n", "e_l", "e_n_in", "e_l_in", "rel_diff", "reg_weight_n", "reg_weight_l", "cg_iters", "converged", "diverged", "upsampled")
DUMP_CAP_BYTES = 64 << 20


def collect_outputs(eng, recs, slab, cap_bytes):
    """what a caller of the timed loop receives after its last step: the band's distances, gradients and albedo, the poses, the light and the
    records of the timed iterations.  A slab rank returns its own band voxels.  Beyond cap_bytes: a fixed, seeded sample of the band voxels."""
    n = None
    if slab:
        mi = eng.mg_info()
        n = int(mi["row1"] - mi["row0"])
    band = eng.download_band(n)
    vol = eng.download_volume()
    small = {"poses": eng.download_poses(), "light": eng.download_light(),
             "records": np.array([[float(r[k]) for k in REC_FIELDS] + [float(x) for x in r["e_after"]] for r in recs], np.float64)}
    per_voxel = 4 * (1 + 3 + 3) + 8                                   # dist, grad, albedo (float32) + band_index (float64)
    room = max(cap_bytes - sum(a.nbytes for a in small.values()), 0) // per_voxel
    rows = np.arange(len(band))
    if len(band) > room:
        rows = np.sort(np.random.default_rng(0).choice(len(band), size=room, replace=False))
    vox = band[rows]
    return dict(small, band_index=vox.astype(np.float64), dist=vol["dist"][vox], grad=np.ascontiguousarray(vol["grad"][:, vox]),
                albedo=np.ascontiguousarray(vol["rgb"][:, vox]))


def write_outputs(folder, outputs, rank, world):
    for name, a in outputs.items():
        np.save(os.path.join(folder, f"{name}.npy" if world == 1 else f"{name}_rank{rank}.npy"), a)


def measure(args, model, torch, dist, rank, world, device, slab, share, headline, collect=None):
    """one workload: scene, contexts, the timed loop; returns the fields of the JSON line for it.  A plain run times the loop `value` is about and
    nothing else; the psgsdf_iterate context (kernel breakdown, iterate_ms_per_step, the solve model) runs with --full, when it IS the timed loop
    (--loop iterate), or when psgsdf_optimize does not survive 3 iterations.  collect(engine, records): what the timed loop hands its caller,
    taken from the context of its last timed step (res["outputs"])."""
    full = args.full
    reps = max(1, args.reps)
    planes_of = None
    t_gen = time.time()
    use_u8 = args.u8_images
    scene_kw = dict(N=args.grid, F=args.frames, W=args.width, H=args.height, model=model, u8=use_u8 or getattr(args, "u8_scene", False))      # (u8_scene: keyframes quantised to 8 bits but handed over as FLOATS, as the reference's loader does)
    if args.strong:
        # ONE volume for all ranks; a rank renders the keyframes (every rank needs all of them) and synthesises only the planes it is asked for:
        # first its share of the planes for the cut negotiation, then its own slab + halo planes (capi.load_scene_slab)
        nz = args.grid
        sc = synth.make_scene(z_planes=(rank * nz // world, (rank + 1) * nz // world), **scene_kw)

        def planes_of(zlo, zhi):
            part = sc if tuple(sc.z_planes) == (zlo, zhi) else synth.make_scene(z_planes=(zlo, zhi), reuse=sc, **scene_kw)
            return dict(dist=part.dist, grad=part.grad, weight=part.weight, rgb=part.rgb, vis=part.vis)
    else:
        sc = synth.make_scene(**scene_kw)
    t_gen = time.time() - t_gen
    model_id = synth.MODELS[model]
    st = capi.default_settings(model_id)
    if model == "LED":   # config_basket_LED.json
        st.reg_weight_n, st.reg_weight_l, st.damping = 0.1, 5.0, 3.0
    if world > 1 and not args.strong:
        # weak scaling: `world` copies of the scene stacked along z, every rank building only the planes it is asked for (never the n-fold volume)
        sc, planes_of = synth.tile_scene_lazy(sc, world)

    def context(settings):
        eng = capi.load_engine(sc, sc.K, settings, device)
        if slab:
            attach_comm(eng, dist, rank, world, share)
        if args.strong or world > 1:
            eng.load_scene_slab(sc, rank, world, planes=planes_of, u8=use_u8)
        else:
            eng.load_scene(sc, u8=use_u8)
        return eng

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def band_rows(eng):
        if not slab:
            return None
        mi = eng.mg_info()
        return int(mi["row1"] - mi["row0"])

    timing_iterate = args.loop == "iterate"
    use_watch = headline and full and os.environ.get("PSGSDF_NO_WATCH") != "1"
    it = {"t_iter": None, "recs": None, "kernels": {}, "dom": "sweep_dist", "watched": (0.0, 0), "kernels_per_rank": None, "solve_model": None,
          "collectives_per_step": None, "n_obs": None, "outputs": None}

    def iterate_context(want_outputs):
        # ---- context 1: psgsdf_iterate (no stop decision): kernel breakdown, the dominant kernel, the round-2 figure
        eng = context(st)
        eng.init_albedo()
        eng.normalize_weights()
        it["S"] = eng.info().n_band // world              # per-slab band size (weak: every slab holds one copy of the scene; strong: the mean)
        it["n_obs"] = eng.step(capi.ALBEDO)["n_obs"] // world
        it["own_rows"] = band_rows(eng)
        eng.iterate(capi.ALL, args.warmup)
        kernels, dom = {}, "sweep_dist"
        nprof = 0
        if headline and full and not args.no_breakdown:
            # the dominant kernel (largest total time per iteration) from a short synchronous-event pass; THAT kernel is then timed inside the
            # timed region with HIP events recorded on the launch stream (no host sync)
            eng.set_profiling(True)
            eng.reset_kernel_times()
            nprof = 3
            eng.iterate(capi.ALL, nprof)
            kt = eng.kernel_times()
            eng.set_profiling(False)
            kernels = {k: {"ms_per_iter": v[0] / nprof, "launches_per_iter": v[1] / nprof} for k, v in kt.items()}
            dom = max(kernels, key=lambda k: kernels[k]["ms_per_iter"] if algorithmic_bytes(k, 1, 1, 1, 1, 1) else -1)
        if dist is not None and headline and full and not args.no_breakdown:      # every rank's own breakdown: a measured N-GPU curve can be attributed kernel by kernel
            it["kernels_per_rank"] = [None] * world
            dist.all_gather_object(it["kernels_per_rank"], {k: round(1e3 * v["ms_per_iter"], 1) for k, v in kernels.items()})
        it["kernels"], it["dom"] = kernels, dom
        it["watch"] = dom + ("/16" if dom == "pcg_pass" else "/4")   # HIP events around every 16th (4th) launch (each pair breaks the back-to-back dispatch: ~6 us of stream time)
        eng.reset_kernel_times()
        if use_watch and timing_iterate:
            eng.watch_kernel(it["watch"])
        barrier()
        coll0 = eng.comm_stats()
        t0 = time.perf_counter()
        it["recs"] = eng.iterate(capi.ALL, args.steps)
        torch.cuda.synchronize()
        it["t_iter"] = time.perf_counter() - t0
        coll1 = eng.comm_stats()
        barrier()
        it["collectives_per_step"] = (coll1 - coll0) / max(args.steps, 1)
        if use_watch and timing_iterate:
            it["watched"] = eng.kernel_times().get(dom, (0.0, 0))
        eng.watch_kernel("")
        it["sync_stats"] = eng.debug_sync_stats()
        if collect and want_outputs:
            it["outputs"] = collect(eng, it["recs"])
        if headline and full and dom == "pcg_solve" and not slab and os.environ.get("PSGSDF_BENCH_NO_SOLVE_MODEL") != "1":      # (off under the kernel trace of tools/profile_round.sh: the forced-pass launches would sit in the solve's statistics)
            # what the dominant kernel's time is made of, measured live: the same launch forced to 16 and to 48 passes (stop rule off) -> time per pass
            # and the fixed part (assembly of the system from the sweep's voxel blocks, first records, distance update, launch ramp)
            try:
                t16 = min(eng.debug_time_pcg_solve(passes=16, reps=4)[0] for _ in range(3)); t48 = min(eng.debug_time_pcg_solve(passes=48, reps=4)[0] for _ in range(3))
                per = (t48 - t16) / 32.0
                it["solve_model"] = {"us_per_pass": 1e3 * per, "fixed_us": 1e3 * (t16 - 16.0 * per), "solve_16_passes_us": 1e3 * t16, "solve_48_passes_us": 1e3 * t48}
            except capi.PsgsdfError:
                it["solve_model"] = None
        it["tuning"] = eng.get_tuning()
        eng.close()

    if full or timing_iterate:
        iterate_context(timing_iterate)
    sync_stats, tuning = it.get("sync_stats"), it.get("tuning")

    # ---- context 2: psgsdf_optimize, the loop voxelPS runs (initAlbedo + weight normalisation + iterations with the stop decision)
    t_reps, recs_opt, opt_calls, opt = None, None, 1, {"outputs": None, "S": None, "own_rows": None}
    watched_opt = [(0.0, 0)]
    if full or not timing_iterate:
        st2 = capi.default_settings(model_id)
        st2.reg_weight_n, st2.reg_weight_l, st2.damping = st.reg_weight_n, st.reg_weight_l, st.damping
        st2.max_it, st2.conv_threshold, st2.upsample = args.warmup + args.steps + 4, 0.0, 0

        def before_timed(e):
            if use_watch and not timing_iterate:
                e.reset_kernel_times()
                e.watch_kernel(it["watch"])

        def after_call(e, call):
            nonlocal sync_stats, tuning
            if call == 0 and use_watch and not timing_iterate:
                watched_opt[0] = e.kernel_times().get(it["dom"], (0.0, 0))
                e.watch_kernel("")
            if call == 0 and opt["S"] is None:
                opt["S"], opt["own_rows"] = e.info().n_band // world, band_rows(e)
            if tuning is None:
                tuning = e.get_tuning()
            s2 = e.debug_sync_stats()
            if sync_stats is None:
                sync_stats = s2
                return
            for k in sync_stats:
                sync_stats[k] = max(sync_stats[k], s2[k]) if k in STATE_STATS else sync_stats[k] + s2[k]

        def on_last(e, recs):
            opt["outputs"] = collect(e, recs)
        t_reps, recs_opt, opt_calls = timed_optimize(lambda: context(st2), torch, dist, args.steps, args.warmup, reps if headline else 1, before_timed, after_call,
                                                     on_last if (collect and not timing_iterate) else None)
        if use_watch and not timing_iterate:
            it["watched"] = watched_opt[0]
        if t_reps is None and (it["t_iter"] is None or (collect and it["outputs"] is None)):      # (psgsdf_optimize does not survive 3 iterations on this scene: the line falls back to psgsdf_iterate)
            iterate_context(True)
            sync_stats, tuning = it["sync_stats"], it["tuning"]

    S = it.get("S", opt["S"])
    own_rows = it.get("own_rows", opt["own_rows"])
    if slab and dist is not None:
        gathered = [None] * world
        dist.all_gather_object(gathered, own_rows)
        own_rows = [int(x) for x in gathered]
    elif slab:
        own_rows = [own_rows]
    t_iter = it["t_iter"]

    def over_ranks(x):      # MAX over the ranks (the contract's clock: the slowest rank)
        if dist is None or x is None:
            return x
        if share:           # (gloo group: CPU tensors)
            tt = torch.tensor(list(x) if isinstance(x, (list, tuple)) else [x], dtype=torch.float64)
        else:
            tt = torch.tensor(list(x) if isinstance(x, (list, tuple)) else [x], dtype=torch.float64, device=f"cuda:{device}")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return [float(v) for v in tt.tolist()] if isinstance(x, (list, tuple)) else float(tt.item())
    t_iter, t_reps = over_ranks(t_iter), over_ranks(t_reps)
    t_opt = float(np.median(t_reps)) if t_reps else None
    if dist is not None:      # hand-off statistics of every rank: a fallback anywhere shows in the line
        gathered = [None] * world
        dist.all_gather_object(gathered, sync_stats)
        for k in sync_stats:
            sync_stats[k] = max(g[k] for g in gathered) if (k in STATE_STATS or k == "persist_fallbacks") else sync_stats[k]

    n_reps = reps if headline else 1
    loop = f"psgsdf_optimize ({opt_calls - 1} timed call{'s' if opt_calls != 2 else ''} on fresh contexts after one untimed, {n_reps} repetition{'s' if n_reps != 1 else ''} of the {args.steps}-step bracket)"
    if timing_iterate or t_opt is None:
        elapsed, recs, outputs = t_iter, it["recs"], it["outputs"]
        loop = "psgsdf_iterate" + ("" if timing_iterate else " (psgsdf_optimize does not survive 3 iterations on this scene)")
    else:
        elapsed, recs, outputs = t_opt, recs_opt, opt["outputs"]
    cg_iters = float(np.mean([r["cg_iters"] for r in recs]))
    mult = 1 if args.strong else world
    spread = None
    if t_reps and not (timing_iterate or t_opt is None):
        vals = [mult * args.steps / t for t in t_reps]
        spread = {"reps": len(vals), "min": min(vals), "max": max(vals), "values": [round(v, 1) for v in vals], "statistic": "value = median over the repetitions of the K-step bracket (fresh contexts each)"}
    res = dict(model=model, value=mult * args.steps / elapsed, ms_per_step=1e3 * elapsed / args.steps, spread=spread, loop=loop, S=int(S),
               n_obs=None if it["n_obs"] is None else int(it["n_obs"]), cg_iters=cg_iters,
               iterate_ms_per_step=None if t_iter is None else 1e3 * t_iter / args.steps, optimize_ms_per_step=(1e3 * t_opt / args.steps) if t_opt else None,
               kernels=it["kernels"], dom=it["dom"], watched=it["watched"], t_gen=t_gen, st=st, sc=sc, sync_stats=sync_stats,
               collectives_per_step=it["collectives_per_step"], use_u8=use_u8, own_rows=own_rows, outputs=outputs,
               scene_kw=scene_kw, solve_model=it["solve_model"], tuning=tuning, make_context=lambda: context(st), kernels_per_rank=it["kernels_per_rank"])
    return res


def full_size_check(make_context, m, args, model, torch, dist, rank, world, device):
    """The N-rank engine against ONE context on the MEASURED scene at its full size: the first three Gauss-Newton iterations from the same start (N ranks on
    their slabs; rank 0 synthesises the whole volume and runs it on one context on its own device), every e_total within 1e-5.  Three iterations, not the
    whole timed run: this algorithm amplifies rounding tenfold per iteration or two from about the tenth on (profiles/r05_notes.md section 2 -- the oracle
    differs from its own FMA build by 1e-2 after 16), so a slab run and a single context, which sum in different orders, legitimately drift apart later."""
    n_it = 3
    eng = make_context()
    eng.init_albedo(); eng.normalize_weights()
    e_n = [float(r["e_total"]) for r in eng.iterate(capi.ALL, n_it)]
    eng.close()
    res = [None]
    if rank == 0:
        sc = synth.make_scene(**m["scene_kw"])
        ref = capi.load_engine(sc, sc.K, m["st"], device)
        ref.load_scene(sc, u8=m["use_u8"])
        ref.init_albedo(); ref.normalize_weights()
        e_1 = [float(r["e_total"]) for r in ref.iterate(capi.ALL, n_it)]
        ref.close()
        rel = max(abs(a - b) / abs(b) for a, b in zip(e_n, e_1))
        res = [{"scene": f"the measured one ({args.grid}^3 x {args.frames} keyframes, {model}), e_total of the first {n_it} iterations, {world} ranks vs one context on rank 0's device",
                "rel_diff": rel, "tol": 1e-5, "ok": bool(rel <= 1e-5), "e_total_ranks": e_n, "e_total_single": e_1}]
    dist.broadcast_object_list(res, src=0)
    return res[0]


def multi_gpu_block(m, check, world, share):
    """the multi-GPU fields of one workload + its `degraded` flag (the cross-rank persistent solve is off or fell back, or a self-check failed)"""
    ss = m["sync_stats"]
    kinds = {-1: "not probed", 0: "none (cross-rank solve off)", 1: "fine-grained", 2: "uncached", 3: "coarse (pinned)"}
    blk = {"ranks": world, "transport": "gloo test transport, all ranks on GPU 0 (functional check only)" if share else "rccl", "rccl_ranks": 0 if share else world,
           "cross_rank_ready": int(ss["cross_rank_ready"]), "cross_rank_solves": int(ss["cross_rank_solves"]), "persist_fallbacks": int(ss["persist_fallbacks"]),
           "hand_off_memory": kinds.get(int(ss["cross_rank_mem_kind"]), "?"), "probe_stale_records": int(ss["probe_stale"]), "probe_timeouts": int(ss["probe_timeouts"]),
           "collectives_per_step": m["collectives_per_step"], "halo_exchanges_by_push_kernels": int(ss.get("halo_pushes", 0)),
           "band_rows_per_rank": m["own_rows"],
           "exchange": "inside the kernels through IPC-mapped peer memory (distance solve, per-frame rows, scalar folds, halo rows); collectives_per_step counts what still went through the communicator",
           "self_check": check}
    if m.get("kernels_per_rank"):
        # per rank, microseconds per iteration from the synchronous-event pass (each launch bracketed by events and a host wait: ~4 us above rocprofv3's
        # durations per launch; it ranks and attributes, it does not add up to ms_per_step).  The distance solve's launch / (passes + 1 prologue round) bounds
        # the cross-rank pass from above (it still contains the assembly and the update: ~30 us on one GPU at the headline band).
        blk["per_rank_kernels_us_per_iteration_sync_pass"] = m["kernels_per_rank"]
        passes = m["cg_iters"] + 2.0
        blk["cross_rank_solve"] = {"passes_per_solve": passes, "us_per_launch_per_rank": [k.get("pcg_solve", k.get("pcg_pass")) for k in m["kernels_per_rank"]],
                                   "us_per_pass_upper_bound_per_rank": [round((k.get("pcg_solve") or 0.0) / passes, 2) if k.get("pcg_solve") else None for k in m["kernels_per_rank"]],
                                   "one_gpu_reference": "7.0 us per pass + 30 us fixed on one MI355X at the 256^3 band (roofline.us_per_pass / fixed_us of the N = 1 line); DESIGN.md section 7.5 has the predicted curve"}
    checks_ok = all(c["ok"] for c in (check if isinstance(check, list) else [check]) if c)
    return blk, bool(not ss["cross_rank_ready"] or ss["persist_fallbacks"] > 0 or not checks_ok)


def voxelps_e2e():
    import subprocess, tempfile
    exe = os.path.join(ROOT, "psgradientsdf_amd", "host", "voxelPS"); data = os.path.join(ROOT, "tests", "golden", "sokrates_21")
    if not (os.path.exists(exe) and os.path.isdir(data)):
        return {"skipped": "voxelPS or tests/golden/sokrates_21 not present"}
    res = {"workload": "voxelPS --config_file: config_skorates.json settings (128^3 at 4 mm, SH1, max iter 100, 5e-3) on the reference's demo frames 0-20 (sub-sampled 3x: 380 x 570), 21 keyframes, run to convergence; whole process"}
    for label, flags in (("round5", []), ("round4_path", ["--host-writers"])):
        best = None
        for _ in range(2):
            with tempfile.TemporaryDirectory() as td:
                out = td + "/"
                cfg = {"input": data + "/", "output": out, "pose filename": "pose.txt", "datatype": "multiview", "first": 0, "last": 20, "voxel size": 0.004, "truncation factor": 5, "zmin": 0.5, "zmax": 3.5,
                       "sharpness threshold": 0.0, "model type": "SH1", "loss function": "cauchy", "reg albedo": 0.0, "reg norm": 10.0, "reg laplacian": 0.0, "max iter": 100, "damping": 1.0,
                       "converge threshold": 5e-3, "lambda": 0.2, "upsample": False, "--light": True, "--albedo": True, "--distance": True, "--pose": True}
                json.dump(cfg, open(out + "config.json", "w"))
                r = subprocess.run([exe, "--config_file", out + "config.json", "--timing", out + "timing.json"] + flags, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    return {"error": (r.stdout[-200:] + r.stderr[-200:])}
                t = json.load(open(out + "timing.json"))
                t["iterations"] = r.stdout.count("relative diff"); t["output_bytes"] = sum(os.path.getsize(out + f) for f in os.listdir(out) if f.endswith((".ply", ".sdf", ".txt")))
                if best is None or t["total_s"] < best["total_s"]:
                    best = t
        st = best["stages_s"]; grp = lambda pre: round(sum(v for k, v in st.items() if k.startswith(pre)), 4)
        res[label] = {"total_s": round(best["total_s"], 4), "gauss_newton_iterations": best["iterations"], "output_MB": round(best["output_bytes"] / 1e6, 1),
                      "stages_s": {"decode (main thread)": grp("decode:"), "fusion": grp("fuse:"), "focus measure": grp("keyframe selection"), "dumps (main thread)": grp("dump:"),
                                   "background writer (overlapped)": grp("background:"), "waiting for the writer": grp("wait for the background"), "alternatingOptimize incl. its dumps": grp("alternatingOptimize")}}
    res["speedup"] = round(res["round4_path"]["total_s"] / res["round5"]["total_s"], 2)
    return res


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per device, LOCAL_RANK = device; RANK / WORLD_SIZE / MASTER_* as
    torch.distributed.run would set them), rank 0 inherits stdout and prints the ONE line.  Fewer than N devices -> non-zero exit, unless
    PSGSDF_BENCH_SHARE_GPU=1 (all ranks on GPU 0 through the gloo test transport: a functional check of the code path, not a measurement)."""
    import socket
    import subprocess
    import torch
    share = os.environ.get("PSGSDF_BENCH_SHARE_GPU") == "1"
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if ndev < n and not share:
        print(f"bench.py: --gpus {n} needs {n} devices, {ndev} visible (PSGSDF_BENCH_SHARE_GPU=1 runs the ranks on one device as a functional check; it measures nothing)", file=sys.stderr)
        return 3
    if share and ndev < 1:
        print("bench.py: no GPU visible", file=sys.stderr)
        return 3
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while any(p.poll() is None for p in procs):
            time.sleep(0.2)
            bad = [p for p in procs if p.poll() not in (None, 0)]
            if bad:                      # a rank died: the others would wait for it in a collective
                rc = bad[0].returncode
                break
    finally:
        for p in procs:                  # (exactly the processes started here, by PID)
            if p.poll() is None:
                if rc == 0:
                    p.wait()
                else:
                    p.terminate()
        for p in procs:
            try:
                p.wait(timeout=20)
            except Exception:
                p.kill()
    return rc or max((p.returncode or 0) for p in procs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the K-step bracket (fresh contexts each): value = their median, spread = min / max (default 1; 5 with --full)")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--model", default="SH1", choices=["SH1", "SH2", "LED"])
    ap.add_argument("--u8-images", action="store_true", help="keyframes quantised to 8 bits and handed over as 8-bit RGB (psgsdf_set_keyframes_u8) instead of float RGB")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--force-slab", action="store_true", help="attach the single rank to a one-rank RCCL communicator (overhead of the multi-rank code path)")
    ap.add_argument("--no-extra", action="store_true", help="skip the LED / SH2 lines")
    ap.add_argument("--strong", action="store_true", help="strong scaling: ONE volume (default BASELINE configs[4]: 512^3, SH2, 100 keyframes) cut into --gpus z-slabs; every rank synthesises and uploads only its own planes")
    ap.add_argument("--weak", action="store_true", help="N > 1: `value` = the weak-scaling run (N copies of the scene stacked along z, N x it/s: round 4's default) instead of the strong scaling of the one scene")
    ap.add_argument("--configs4", default="512:100", help="grid:keyframes of the BASELINE configs[4] extra of the N > 1 line (SH2; tests pass a small one)")
    ap.add_argument("--probe-only", action="store_true", help="no measurement: the first-contact probe of a multi-GPU node (tools/first_contact.py: communicator, one collective, the in-kernel hand-off forms per memory kind between every neighbour pair, two iterations with every in-kernel exchange against one context), one JSON line, every phase under a wall-clock bound")
    ap.add_argument("--loop", default="optimize", choices=["optimize", "iterate"], help="which loop `value` times (iterate: the round-2 figure, no stop decision)")
    ap.add_argument("--full", action="store_true", help="everything else the benchmark measures next to `value`: the psgsdf_iterate figure, the kernel breakdown and roofline (with live counter passes), the CPU baseline, "
                    "the other models / solvers / workloads as `extra`, and on N > 1 ranks the full-size check and the weak-scaling and configs[4] runs")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed loop computed in its last step as DIR/<name>.npy (see the module docstring)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.full else 1
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
    if args.probe_only:
        import subprocess
        sys.exit(subprocess.call([sys.executable, os.path.join(ROOT, "tools", "first_contact.py"), "--gpus", str(max(args.gpus, 2))]))
    c4 = [int(x) for x in args.configs4.split(":")]
    if args.strong and (args.grid, args.frames, args.model) == (256, 50, "SH1"):      # --strong and nothing chosen explicitly: BASELINE configs[4] is `value`
        args.grid, args.frames, args.model = c4[0], c4[1], "SH2"
    explicit_strong = args.strong
    if args.gpus > 1 and not args.weak:      # the N > 1 line is the strong scaling of the metric's own problem
        args.strong = True

    # ---- N ranks.  Under a launcher (torch.distributed.run: WORLD_SIZE set) this process IS one of the N ranks; without one, --gpus N > 1
    # starts the N ranks here.  Either way the line reports --gpus ranks or nothing.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ.get('WORLD_SIZE')} ranks: refusing to print a line whose n_gpus differs from --gpus", file=sys.stderr)
        sys.exit(2)

    if os.environ.get("PSGSDF_FAULT_DUMP"):   # diagnostics: dump every thread's Python stack after N seconds and exit
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["PSGSDF_FAULT_DUMP"]), exit=True)
    # RCCL / HIP runtime banners go to the C-level stdout: keep the real stdout for the ONE JSON line only
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    import torch
    slab = world > 1 or args.force_slab
    share = False
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        # PSGSDF_BENCH_SHARE_GPU=1: every rank on GPU 0 and the exchanges through the gloo test transport (RCCL refuses two ranks per
        # device) -- a functional check of this code path on a one-GPU box (tests/test_bench_gpu.py), not a measurement
        share = os.environ.get("PSGSDF_BENCH_SHARE_GPU") == "1"
        if share:
            local_rank = 0
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            # the ranks' persistent solve kernels wait for each other: on ONE device they are only resident together if each rank keeps to its
            # own share of the CUs (PSGSDF_CU_MASK: the context's stream is created with that mask)
            ncu = torch.cuda.get_device_properties(0).multi_processor_count
            os.environ.setdefault("PSGSDF_CU_MASK", f"{rank * (ncu // world)}:{(rank + 1) * (ncu // world)}")
        torch.cuda.set_device(local_rank)
        if share:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:      # torch's process group only carries the RCCL id, the barriers and the MAX of the elapsed time
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
    device = local_rank if world > 1 else 0

    check, fallback = None, None
    if world > 1:
        # A first lease on a multi-GPU node must measure, not debug: the 64^3 self-check runs every in-kernel exchange between the real devices.  If it
        # raises on any rank (a bounded wait expired: the engine names the exchange) or disagrees with the single context, ALL ranks fall back to the
        # communicator paths (PSGSDF_XR=0: one RCCL all-reduce per PCG pass, rows / sums / halos over RCCL) and the line says so: `degraded`, `fallback`.
        # A watchdog ends a rank that is stuck in a collective behind a failed peer (stack dump, non-zero exit) instead of hanging the lease.
        import faulthandler
        if not os.environ.get("PSGSDF_FAULT_DUMP"):
            faulthandler.dump_traceback_later(int(os.environ.get("PSGSDF_BENCH_WATCHDOG_S", "1500")), exit=True)
        if os.environ.get("PSGSDF_BENCH_FAULT"):      # test hook "rank:VAR=value": an environment variable for ONE rank (tests/test_bench_gpu.py: fault injection, development library)
            r_, kv = os.environ["PSGSDF_BENCH_FAULT"].split(":", 1)
            if int(r_) == rank:
                os.environ.update(dict([kv.split("=", 1)]))
        sc_args = ("SH2", 70) if args.model == "SH2" else ("SH1", 8)

        def guarded():
            err, chk = None, None
            try:
                chk = self_check(dist, rank, world, device, share, *sc_args)
            except capi.PsgsdfError as ex:
                err = str(ex)[-300:]
            votes = [None] * world
            dist.all_gather_object(votes, (bool(err is None and chk and chk["ok"]), err))
            return chk, votes
        check, votes = guarded()
        if not all(v[0] for v in votes):
            reason = next((f"rank {i}: {v[1]}" for i, v in enumerate(votes) if v[1]), "the N-rank result differs from the single context's")
            if rank == 0:
                print(f"bench.py: the self-check with the in-kernel exchanges failed ({reason}); falling back to the communicator paths (PSGSDF_XR=0)", file=sys.stderr)
            os.environ["PSGSDF_XR"] = "0"
            for k in ("PSGSDF_FAULT_HALO", "PSGSDF_FAULT_SOLVE"):
                os.environ.pop(k, None)
            fallback = {"reason": reason, "exchanges": "RCCL collectives on every rank (PSGSDF_XR=0): one all-reduce per PCG pass, per-frame rows, scalar sums and halo rows over the communicator"}
            check, votes = guarded()
            if not all(v[0] for v in votes):
                if rank == 0:
                    print("bench.py: the self-check fails on the communicator paths too: " + "; ".join(f"rank {i}: {v[1]}" for i, v in enumerate(votes) if v[1]), file=sys.stderr)
                sys.exit(4)
    collect = (lambda eng, recs: collect_outputs(eng, recs, slab, DUMP_CAP_BYTES // world)) if args.dump_outputs else None
    m = measure(args, args.model, torch, dist, rank, world, device, slab, share, headline=True, collect=collect)
    if args.dump_outputs:
        write_outputs(args.dump_outputs, m.pop("outputs"), rank, world)
    if world > 1 and args.full and args.strong and os.environ.get("PSGSDF_BENCH_NO_FULL_CHECK") != "1":
        check = [check, full_size_check(m["make_context"], m, args, args.model, torch, dist, rank, world, device)]
    S, n_obs, cg_iters, kernels, dom, watched, st, sc = m["S"], m["n_obs"], m["cg_iters"], m["kernels"], m["dom"], m["watched"], m["st"], m["sc"]
    use_u8 = m["use_u8"]
    out = {
        "metric": "Gauss-Newton iterations/sec (full PS sweep), 256^3 grid x 50 frames" if (args.grid, args.frames) == (256, 50)
        else f"Gauss-Newton iterations/sec (full PS sweep), {args.grid}^3 grid x {args.frames} frames",
        "value": m["value"], "unit": "it/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        # (one GPU: the strong and the weak run are the same run; the N > 1 line is the strong scaling of this scene unless --weak)
        "ms_per_step": m["ms_per_step"], "higher_is_better": True, "scaling": "weak" if args.weak else "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic (8-bit RGB keyframes)" if use_u8 else "synthetic",
        "config": {"workload": f"synthetic {args.width}x{args.height} RGB-D bumpy sphere, {args.grid}^3 grid, {args.model}, {args.frames} keyframes, "
                               "albedo+light+distance+pose blocks, Cauchy IRLS, Eikonal reg (config_skorates.json settings)",
                   "loop": m["loop"] + ": stop decision (convergence / divergence test on the host) after every iteration; each timed call ends itself before the loop's own divergence exit would",
                   "band_voxels": int(S), "observations": None if n_obs is None else int(n_obs), "pcg_iters_per_step": cg_iters,
                   "parallelism": "single GPU" if world == 1 else
                   (f"strong scaling: ONE {args.grid}^3 volume with {args.frames} keyframes cut into {world} z-slabs of equal band count (one per GPU; every rank synthesises and uploads only its own planes), native slab loop of the C++ host; exchanges inside the kernels over IPC-mapped peer memory, RCCL for set-up and as the fallback" if args.strong else
                    f"{world} z-slabs (one per GPU), grid {args.grid}x{args.grid}x{args.grid * world}, {args.frames * world} keyframes, native slab loop of the C++ host; exchanges inside the kernels over IPC-mapped peer memory, RCCL for set-up and as the fallback")},
        "optimize_ms_per_step": m["optimize_ms_per_step"],
        "spread": m["spread"],
    }
    if m["iterate_ms_per_step"] is not None:      # psgsdf_iterate: the same iterations without a stop decision (round-2 `value`; --full or --loop iterate)
        out["iterate_ms_per_step"] = m["iterate_ms_per_step"]
        out["iterate_value"] = (1 if args.strong else world) * 1e3 / m["iterate_ms_per_step"]
    if world > 1:
        # degraded: the line is not the design's N-GPU figure -- the cross-rank persistent solve is off or fell back, or the N-rank result is wrong
        out["multi_gpu"], out["degraded"] = multi_gpu_block(m, check, world, share)
        if fallback:
            out["multi_gpu"]["fallback"] = fallback; out["degraded"] = True

    if rank == 0:
        if slab:
            out["config"]["collectives_per_step"] = m["collectives_per_step"]
            out["config"]["band_rows_per_rank"] = m["own_rows"]
        out["config"]["frame_solver"] = m["tuning"]["effective"].get("frame_solve", "ldlt") + (
            " (light / pose blocks: every frame's block solved directly, LDL^T in double, inside the sweep; the reference's own solver -- ONE global float Jacobi-PCG, PSGSDF_FRAME_SOLVE=eigen -- is measured under extra.reference_frame_solver)"
            if m["tuning"]["effective"].get("frame_solve", "ldlt") == "ldlt" else " (the reference's solver of the light / pose blocks: one global float Jacobi-PCG over all frames, csrc/frame_solve.hip)")
        out["sync_stats"] = m["sync_stats"]      # scalar read-backs validated / found late / persistent-solve fallbacks in this run (include/psgsdf.h)
        out["tuning"] = {"build": m["tuning"]["build"], "env": m["tuning"]["env"], "ignored_dev_only": m["tuning"]["ignored_dev_only"]}      # psgsdf_get_tuning: every PSGSDF_* knob that was in force
        out["setup_s"] = {"scene_generation": round(m["t_gen"], 1)}

    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel, timed live with HIP events inside the timed region
        lap = st.reg_weight_l != 0.0
        # event pairs recorded on the launch stream around every 16th launch: the pair also reads the dispatch latency, so this is
        # ~2.5 us above the kernel duration rocprofv3 --kernel-trace reports (profiles/): the roofline fraction errs low
        avg_ms = watched[0] / max(watched[1], 1) if watched[1] else float("nan")
        nbytes = algorithmic_bytes(dom, S, n_obs, args.width, args.height, args.frames, lap, pcg_passes=cg_iters + 1.0)   # per GPU (one slab); a solve of n iterations runs n + 1 passes
        # the solve enqueues the previous solve's pass count + 2: the surplus kernels return at once (no-op launches, ~4.7 us) and are part
        # of the sampled average; `avg_working_launch_ms` removes them with the measured ratio passes / launches
        launches_per_step = kernels.get(dom, {}).get("launches_per_iter") if kernels else None
        working_frac = min(1.0, (cg_iters + 1.0) / launches_per_step) if (dom == "pcg_pass" and launches_per_step) else 1.0
        noop_ms = 0.0047
        avg_work_ms = (avg_ms - (1.0 - working_frac) * noop_ms) / working_frac if working_frac > 0 else avg_ms
        achieved = nbytes / (avg_ms * 1e-3) / 1e9
        traffic, traffic_src, pj = None, None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
        # (the archived rocprofv3 summaries carry the hash of the engine sources they were collected on: the line says whether the sources have changed since)
        try:
            src_hash = open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", ".build_hash")).read().strip()[:12]
        except OSError:
            src_hash = None
        stale = lambda j: None if not (j and j.get("source_hash") and src_hash) else bool(j["source_hash"] != src_hash)
        live = live_traffic(args) if (world == 1 and not slab and not args.no_breakdown) else None
        if live and live.get("kernels", {}).get(dom):
            pj = dict(live["kernels"])
            traffic = pj[dom]["hbm_bytes_per_launch"]
            traffic_src = f"live: {live['how']} ({live['seconds']} s, {pj[dom]['launches']} launches of {dom})"
            out["pmc_live"] = live
        elif os.path.exists(pmc) and (args.grid, args.frames, args.model, world) == (256, 50, "SH1", 1):   # the counters were collected on this configuration
            try:
                pj = json.load(open(pmc))
                traffic = (pj.get(dom) or {}).get("hbm_bytes_per_launch")
                traffic_src = (f"static: profiles/pmc_summary.json @{pj.get('commit', '?')} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, FETCH_SIZE x2 (gfx950), KiB -> bytes); "
                               f"not re-measured in this run ({(live or {}).get('error') or 'rocprofv3 not available / live pass switched off'}); engine sources changed since it was collected: {stale(pj)}")
            except Exception:
                traffic = None
        out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "bytes_per_launch": nbytes, "avg_launch_ms": avg_ms,
                           "traffic_over_algorithmic": (traffic / nbytes) if (traffic and nbytes) else None,      # < 1: the kernel keeps data on chip (pcg_solve: the matrix lives in LDS); it is then NOT bandwidth-bound and `frac` overstates how close to a limit it runs
                           "launches_timed": int(watched[1]), "avg_working_launch_ms": avg_work_ms, "working_launch_fraction": working_frac,
                           "bytes_per_unit": "SURVEY 8d algorithmic figure (PCG: 124 B per band voxel per pass; pcg_solve runs cg_iters + 1 passes per launch and keeps the matrix on chip: its HBM-side traffic is far below the algorithmic bytes; the launch also assembles the distance system from the sweep's voxel blocks, which is NOT counted here)",
                           "storage_bytes_per_launch": 152 * S if dom in ("pcg_pass", "pcg_solve") else None,
                           # the pcg_solve launch also assembles the system (reads the sweep's 14-float voxel blocks + 3 neighbour rows: 68 B per band voxel)
                           # and applies the distance update (8 B): the same fraction with those algorithmic bytes counted, for reference only
                           "frac_with_fused_steps": ((nbytes + 76 * S) / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if dom == "pcg_solve" else None,
                           "traffic_source": traffic_src}
        if dom == "pcg_solve":
            # SURVEY 8d prices this kernel against HBM (`bound`, `frac` above: the contract's figure), but HBM is not what bounds it: the matrix lives in LDS
            # and the counters see 0.13-0.24 x the algorithmic bytes.  A pass is a chain of device-wide hand-offs (tag wait -> gathers of the neighbours' values
            # -> publish); the floor below is that chain at its shortest, the decomposition next to it is measured in this run.
            sm = m.get("solve_model")
            passes = cg_iters + 2.0                                      # cg_iters + 1 passes, + the prologue's gather round w_0 = A u_0
            hand_off_us = 3.0                                            # one device-wide hand-off through memory on MI355X (profiles/r04_notes.md section 4, tools/mapped_visibility.hip)
            fixed_floor_us = 76.0 * S / (HBM_PEAK_GBS * 1e3) + 2.0       # the fused assembly + update stream 76 B per band voxel once; + the launch ramp
            floor_us = fixed_floor_us + passes * hand_off_us
            out["roofline"].update({
                "bound_observed": "device-wide hand-off latency (per PCG pass: the neighbours' values back from beyond the L2 -- self-validating since round 5: no tag wait, acquire or drain in front of them -- two gather batches, the all-gather of the sums, across 256 workgroups; the matrix is LDS-resident, HBM-side traffic is %s x the algorithmic bytes)" % (("%.2f" % out["roofline"]["traffic_over_algorithmic"]) if out["roofline"].get("traffic_over_algorithmic") else "a fraction of"),
                "passes": passes, "us_per_pass": sm["us_per_pass"] if sm else None, "fixed_us": sm["fixed_us"] if sm else None,
                "floor_model": {"formula": "fixed_floor + passes x hand_off", "hand_off_us": hand_off_us, "fixed_floor_us": fixed_floor_us, "floor_us": floor_us,
                                "measured_us": 1e3 * avg_ms, "frac_of_floor": floor_us / (1e3 * avg_ms) if avg_ms == avg_ms else None,
                                "measured_decomposition_us": ({"fixed (assembly, first records, update, launch)": sm["fixed_us"], "passes": passes * sm["us_per_pass"]} if sm else None),
                                "note": "a pass costs 2.3 hand-offs' worth (round 4: 2.7): the exchanged values carry their own tags, so the chain is store -> gather (re-issued until the tag is the pass's) -> sums; 18 gathers per row in two batches (profiles/r04_notes.md section 4, r05_notes.md sections 9-10)"}})
        # whole-iteration algorithmic bytes (SURVEY.md §8d formula) for reference
        U = min(48 * n_obs, 12 * args.width * args.height * args.frames)
        B_iter = 4 * (S * 60 + U) + 120 * S + 124 * cg_iters * S   # SURVEY §8d per-pass figure kept (the fused pass moves 144 B/row)
        out["iteration"] = {"algorithmic_bytes": B_iter, "achieved_GBs": B_iter * (m["value"] / world) / 1e9,
                            "frac_of_hbm_peak": B_iter * (m["value"] / world) / 1e9 / HBM_PEAK_GBS}
        if pj:      # the same fraction from the COUNTERS (archived passes): what really crosses the HBM interface per iteration -- nothing on this path is bandwidth-bound
            per_iter = ("pcg_solve", "sweep_dist", "sweep_pose", "sweep_light", "sweep_albedo", "derive")
            cb = sum((pj.get(k) or {}).get("hbm_bytes_per_launch", 0.0) for k in per_iter)
            out["iteration"].update({"counter_bytes": cb, "counter_frac_of_hbm_peak": cb * (m["value"] / world) / 1e9 / HBM_PEAK_GBS,
                                     "counter_source": (f"live (pmc_live), kernels {', '.join(per_iter)}" if "pmc_live" in out else f"static: profiles/pmc_summary.json @{pj.get('commit', '?')}, kernels {', '.join(per_iter)}; sources changed since: {stale(pj)}")})
        if kernels:
            # A SYNCHRONOUS-event pass over psgsdf_iterate (every launch bracketed by an event pair and a host wait: ~4 us of overhead per launch, and
            # `energy`, which the product loop folds into the next sweep, runs as a kernel of its own here): it ranks the kernels, it does not add
            # up to ms_per_step.  The table that does is rocprofv3's (kernels_rocprof).
            out["kernels_sync_pass"] = {k: round(v["ms_per_iter"], 4) for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_iter"])}
            ks = os.path.join(ROOT, "profiles", "kernel_stats_summary.json")
            if os.path.exists(ks) and (args.grid, args.frames, args.model, world) == (256, 50, "SH1", 1):
                try:
                    out["kernels_rocprof"] = json.load(open(ks))      # static: rocprofv3 --kernel-trace --stats of this command at the stamped commit (us per iteration, sums to the iteration)
                    out["kernels_rocprof"]["engine_sources_changed_since"] = stale(out["kernels_rocprof"])
                except Exception:
                    pass
            # per-kernel roofline fractions from the same synchronous-event pass (events add ~4 us per launch: fractions err low)
            out["kernel_roofline_frac"] = {k: round(algorithmic_bytes(k, S, n_obs, args.width, args.height, args.frames, lap, pcg_passes=cg_iters + 1.0) / (v["ms_per_iter"] / max(v["launches_per_iter"], 1e-9) * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)
                                           for k, v in kernels.items() if algorithmic_bytes(k, 1, 1, 1, 1, 1) and v["ms_per_iter"] > 0}

        # ---- CPU baseline: the oracle (a port of the reference's arithmetic) on the host cores, bounded sample
        if world == 1 and not slab and not args.no_cpu_baseline and not args.strong:
            from oracle import oracle
            orc = oracle.Oracle(sc, sc.K, st, threads=1)
            orc.load_scene(sc)
            orc.init_albedo()
            orc.normalize_weights()
            tc = time.perf_counter()
            orc.iterate(capi.ALL, 1)
            tc = time.perf_counter() - tc
            out["cpu_baseline"] = {"value": 1.0 / tc, "unit": "it/s", "cores": 1, "kind": "port",
                                   "sample": f"1 full Gauss-Newton iteration of the same {args.grid}^3 x {args.frames} scene "
                                             f"(4 blocks + 4 energy evaluations), single-threaded C oracle with indexed band lookup, {tc:.1f} s"}
            orc.close()
            # SURVEY 8d(i) "faithful mode": the reference tests band membership with std::find over the band list (Optimizer.cpp:470 and eight more
            # sites), O(S) per test.  Measured on a 64^3 crop (8 keyframes, 320x240) with the oracle's look-ups switched to that linear scan, the
            # excess over the indexed run extrapolated by its law: excess ~ (membership tests ~ N_obs) x (scan length ~ S).
            scf = synth.make_scene(N=64, F=8, W=320, H=240, model=args.model)
            tf = []
            for faithful in (False, True):
                orc = oracle.Oracle(scf, scf.K, st, threads=1)
                orc.load_scene(scf); orc.init_albedo(); orc.normalize_weights()
                orc.set_faithful(faithful)
                t0 = time.perf_counter(); orc.iterate(capi.ALL, 1); tf.append(time.perf_counter() - t0)
                if not faithful:
                    Sf, nof = int(orc.info().n_band), int(orc.step(capi.ALBEDO)["n_obs"])
                orc.close()
            excess = max(tf[1] - tf[0], 0.0) * (float(n_obs) * float(S)) / (float(nof) * float(Sf))
            out["cpu_baseline"]["faithful"] = {"value": 1.0 / (tc + excess), "unit": "it/s", "cores": 1, "kind": "port, std::find membership (extrapolated)",
                                               "sample": f"64^3 x 8-keyframe crop (band {Sf}, {nof} observations): 1 iteration indexed {tf[0]:.2f} s, with linear std::find-style membership {tf[1]:.2f} s; "
                                                         f"the excess scaled by (N_obs x S) = ({n_obs} x {S}) / ({nof} x {Sf}) and added to the indexed full-size iteration ({tc:.1f} s): {tc + excess:.0f} s per iteration -- an EXTRAPOLATION, not a measurement at full size"}
            del scf
            # the same port with its sweeps spread over the host's cores (OpenMP): informative only, `value` stays the one-core figure
            nthr = min(64, os.cpu_count() or 1)
            if nthr > 1:
                orc = oracle.Oracle(sc, sc.K, st, threads=nthr)
                orc.load_scene(sc); orc.init_albedo(); orc.normalize_weights()
                tc = time.perf_counter(); orc.iterate(capi.ALL, 1); tc = time.perf_counter() - tc
                out["cpu_baseline"]["multithreaded"] = {"value": 1.0 / tc, "unit": "it/s", "cores": nthr}
                orc.close()
    m.pop("make_context", None)
    del m, sc
    # ---- the other shading models on the same grid / keyframe shape (BASELINE configs[3] = LED; SH2 = configs[4]'s model at the headline size)
    if args.full and world == 1 and not slab and not args.no_extra and not args.strong and (args.grid, args.frames, args.model) == (256, 50, "SH1"):
        extra = {}
        for mod in ("LED", "SH2"):
            e = measure(args, mod, torch, dist, rank, world, device, slab, share, headline=False)
            extra[mod] = {"value": e["value"], "unit": "it/s", "ms_per_step": e["ms_per_step"], "loop": e["loop"], "iterate_ms_per_step": e["iterate_ms_per_step"],
                          "band_voxels": e["S"], "observations": e["n_obs"], "pcg_iters_per_step": e["cg_iters"],
                          "settings": "config_basket_LED.json (damping 3, reg 0.1 / 5)" if mod == "LED" else "config_skorates.json"}
            del e
        # the headline scene with keyframes that are 8-bit data handed over as floats -- what the reference's main() gives its optimiser after
        # imread + convertTo(CV_32FC3, 1/255): the engine recognises them and samples RGBA8 words (same floats, half the tap instructions)
        args.u8_scene = True
        e = measure(args, "SH1", torch, dist, rank, world, device, slab, share, headline=False)
        args.u8_scene = False
        extra["SH1_png_like_float_keyframes"] = {"value": e["value"], "unit": "it/s", "ms_per_step": e["ms_per_step"],
                                                 "note": "keyframes quantised to 8 bits, passed through psgsdf_set_keyframes (float); held as RGBA8 words (PSGSDF_IMG_COMPACT)"}
        del e
        # ---- the same three workloads with the REFERENCE's solver of the light / pose blocks (PSGSDF_FRAME_SOLVE=eigen: one global float Jacobi-PCG over all
        # frames' blocks in a kernel of its own behind the sweep, csrc/frame_solve.hip) -- what exact solver fidelity costs
        if os.environ.get("PSGSDF_FRAME_SOLVE") is None:
            import copy
            fs = {}
            a3 = copy.copy(args); a3.reps = min(args.reps, 3)
            os.environ["PSGSDF_FRAME_SOLVE"] = "eigen"
            try:
                for mod in ("SH1", "LED", "SH2"):
                    e = measure(a3, mod, torch, dist, rank, world, device, slab, share, headline=False)
                    assert e["tuning"]["effective"].get("frame_solve") == "eigen"
                    base = out["value"] if mod == "SH1" else extra[mod]["value"]
                    fs[mod] = {"value": e["value"], "unit": "it/s", "ms_per_step": e["ms_per_step"], "vs_default_solver": e["value"] / base}
                    del e
            finally:
                del os.environ["PSGSDF_FRAME_SOLVE"]
            fs["note"] = ("Eigen's iteration counts on these scenes: light 42 (SH1) / 250-370 (SH2) / 0 (LED: a diagonal 3 x 3), pose 14; one workgroup, 3 barriers per pass. "
                          "The default (direct block solves inside the sweeps) stays: the reference's solver costs more than 3 % on every model; parity against it is measured either way (tests/test_frame_solver_gpu.py, profiles/r06_parity_margins.json)")
            extra["reference_frame_solver"] = fs
        # ---- the drop-in end to end: `voxelPS --config_file` with config_skorates.json's settings on the reference's demo frames
        # (tests/golden/sokrates_21), wall-clock of the whole process and its stages; "round4_path" = the same binary with --host-writers (dense
        # downloads, host marching cubes, iostream text, serial PNG decode): the files are byte for byte the same (tests/test_extract_gpu.py)
        try:
            extra["voxelps_e2e"] = voxelps_e2e()
        except Exception as ex:      # (never let the side measurement take the line down)
            extra["voxelps_e2e"] = {"error": repr(ex)[:300]}
        if rank == 0:
            out["extra"] = extra
    if args.full and world > 1 and not args.no_extra and not explicit_strong and not args.weak:
        # ---- the other two N-rank workloads ride along, each with its own self-check and `degraded`
        import copy
        extra = {}
        wk = copy.copy(args); wk.strong = False; wk.weak = True
        e = measure(wk, args.model, torch, dist, rank, world, device, slab, share, headline=False)
        blk, deg = multi_gpu_block(e, check[0] if isinstance(check, list) else check, world, share)
        extra["weak"] = {"value": e["value"], "unit": "it/s", "ms_per_step": e["ms_per_step"], "scaling": "weak",
                         "workload": f"{world} copies of the {args.grid}^3 scene stacked along z (grid {args.grid}x{args.grid}x{args.grid * world}), {args.frames * world} keyframes, one slab per GPU; value = {world} x it/s of the whole job ({args.grid}^3 x {args.frames}-frame equivalents per second)",
                         "loop": e["loop"], "band_voxels_per_rank": e["S"], "pcg_iters_per_step": e["cg_iters"], "multi_gpu": blk, "degraded": deg}
        del e
        c4a = copy.copy(args); c4a.strong = True; c4a.grid, c4a.frames = c4[0], c4[1]
        if (c4a.width, c4a.height) == (640, 480) and c4[0] < 256:      # (a small stand-in of the tests: small images too)
            c4a.width, c4a.height = 96, 72
        chk4 = self_check(dist, rank, world, device, share, "SH2", 70)
        e = measure(c4a, "SH2", torch, dist, rank, world, device, slab, share, headline=False)
        blk, deg = multi_gpu_block(e, chk4, world, share)
        extra["configs4_strong"] = {"value": e["value"], "unit": "it/s", "ms_per_step": e["ms_per_step"], "scaling": "strong",
                                    "workload": f"BASELINE configs[4]: ONE {c4[0]}^3 volume, SH2, {c4[1]} keyframes ({(c4[1] + 63) // 64} visibility word{'s' if c4[1] > 64 else ''} per voxel) cut into {world} z-slabs of equal band count",
                                    "loop": e["loop"], "band_voxels_per_rank": e["S"], "pcg_iters_per_step": e["cg_iters"], "multi_gpu": blk, "degraded": deg}
        del e
        if rank == 0:
            out["extra"] = extra
    if rank == 0:
        print(json.dumps(out), file=real_stdout, flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
