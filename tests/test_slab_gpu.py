"""The engine's native multi-rank path on real hardware: psgsdf_iterate / psgsdf_optimize on contexts attached to ranks, the
exchanges issued by the C++ host itself.  (a) one rank with the engine's own RCCL communicator (dlopen, ncclCommInitRank, all-reduces
enqueued on the engine's stream); (b) two and three ranks sharing the one GPU through the caller-supplied transport (RCCL refuses two
ranks per device): real halo exchanges, all-reduces and the all-gather between engine contexts.  All must reproduce the plain
single-context engine, which the parity tests pin to the oracle."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _ranks
from _ranks import stitch
from psgradientsdf_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def run_ranks(tmp_path, model, world, transport, mode, N, n_iters, extra_env=None, timeout=150):
    """the slab worker keeps its own command line and variable names (tools/soak_slab.py and the cases below name them); CU ranges are the caller's (extra_env)"""
    port = free_port(); out = str(tmp_path / "slab")
    _ranks.run_ranks("_slab_worker_gpu.py", [[r, world, port, model, out, n_iters, N, transport, mode] for r in range(world)], world, timeout,
                     env={"SLAB_WORKER_TIMEOUT": str(timeout - 40), **(extra_env or {})}, mesh=transport == "sockets", split=False, names=("SLAB_FDS", "SLAB_CU_MASKS"))
    return [np.load(out + f".rank{r}.npz") for r in range(world)]


@pytest.mark.parametrize("model,world,transport", [("SH1", 1, "rccl"), ("SH1", 1, "rccl-perpass"), ("SH1", 2, "gloo"), ("SH1", 2, "gloo-xr0"), ("SH1", 3, "gloo-xf0"), ("LED", 2, "gloo-xs0"), ("SH1", 3, "gloo-xh0"), ("LED", 2, "gloo"), ("SH1", 3, "gloo"), ("SH1", 4, "gloo"), ("SH2", 2, "gloo"),
                                                   ("SH1+reg", 2, "gloo")])
def test_native_slab_loop_matches_single_context(built, margins, tmp_path, model, world, transport):
    N, n_iters = 40, 2
    # "rccl-perpass": the PCG as the multi-rank path runs it (one kernel, one fold and one RCCL all-reduce of 7 doubles per pass) -- a one-rank
    # communicator would otherwise use the persistent single-kernel solve, which needs no exchange
    # "gloo-xr0": the multi-rank PCG of round 2 (per-pass kernels, one all-reduce of 7 doubles and one halo exchange per pass); without it the ranks
    # run the CROSS-RANK PERSISTENT solve (pcg_solve.h k_cgp_solve<.., MR>: halo records pushed into the neighbour's band through IPC mappings, rank-level
    # sums through every rank's mailbox region) -- here between two / three processes sharing the one GPU
    # "gloo-xf0": the per-frame light / pose rows through an all-reduce and the solve kernels (round 3); without it they meet inside the sweeps
    extra = {"PSGSDF_PCG_PERSIST": "0"} if transport == "rccl-perpass" else {"PSGSDF_XR": "0"} if transport == "gloo-xr0" else {"PSGSDF_XF": "0"} if transport == "gloo-xf0" else {"PSGSDF_XS": "0"} if transport == "gloo-xs0" else {"PSGSDF_XH": "0"} if transport == "gloo-xh0" else None      # "gloo-xs0": scalar read-backs staged and all-reduced (round 3) instead of exchanged by the folding thread
    res = run_ranks(tmp_path, model, world, transport.split("-")[0], "iterate", N, n_iters, extra)
    # "+reg": with the albedo regulariser -- the matrix-free CG over 3S unknowns whose Jr / Jr^T stencils cross the cut (halo exchanges
    # of J, res, p and t; every dot product an all-reduce)
    model, _, opt = model.partition("+")
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model=model)
    st = capi.default_settings(sc.model_id, **({"reg_weight_rho": 0.02} if opt == "reg" else {}))
    ref = capi.load_engine(sc, sc.K, st, 0); ref.load_scene(sc)
    ref.init_albedo(); e0 = ref.normalize_weights()
    recs = ref.iterate(capi.ALL, n_iters)
    band = ref.download_band(); v = ref.download_volume(); vs = float(sc.voxel_size)
    for r, got in enumerate(res):      # every rank reports the same global energies, iteration counts, poses
        assert abs(float(got["e0"]) - e0) <= 1e-6 * abs(e0)
        assert np.allclose(got["e_total"], [x["e_total"] for x in recs], rtol=2e-4 if model == "SH2" else 5e-6)
        assert np.all(np.abs(got["cg"] - np.array([x["cg_iters"] for x in recs])) <= 1)
        assert np.abs(got["poses"] - ref.download_poses()).max() <= (2e-5 if model == "SH2" else 1e-6)
        row0, row1, halo, S, need_lo, need_hi, z0, z1, rows = got["info"]
        assert S == len(band) == int(got["n_band"]) and list(got["dim"]) == [N, N, N]
        assert rows == need_lo + (row1 - row0) + need_hi and rows <= S
        if world > 1:
            assert halo > 0 and (need_lo > 0 or need_hi > 0)        # the sphere is cut through: stencils cross the cut, halos really move
            assert rows < 0.8 * S                                     # a rank holds its slab (+ halo planes), not the whole band
            xr_ready, xr_solves, fallbacks, mem_kind, probe_stale, probe_to = (int(x) for x in got["xr"])
            # the hand-off probe ran between the real neighbours (here: processes sharing one GPU) and chose the memory kind of the record planes
            assert (mem_kind == 0 if transport == "gloo-xr0" else mem_kind == 1) and probe_stale == 0 and probe_to == 0
            if transport == "gloo-xr0":
                assert xr_ready == 0 and xr_solves == 0 and got["ncoll"] > 40     # ~2 exchanges per PCG pass
            else:
                # the distance solves ran as ONE kernel per rank (a rank that cannot wait any longer for the others -- a badly loaded host -- makes
                # ALL ranks fall back to the per-pass kernels together; that is correct behaviour too, so it is tolerated here and counted)
                assert xr_ready == 1 and xr_solves >= 1 and fallbacks <= 1
                # (frame rows, scalar folds and halo rows all travel through the mapped regions: what is left for the communicator is set-up traffic;
                #  "gloo-xf0/xs0/xh0" switch one of the three back to it)
                assert got["ncoll"] > (4 if transport in ("gloo-xf0", "gloo-xs0", "gloo-xh0") else 0) and int(got["halo_pushes"]) > (0 if transport != "gloo-xh0" else -1)
                if transport == "gloo-xh0":
                    assert int(got["halo_pushes"]) == 0
                if opt != "reg" and fallbacks == 0:
                    assert xr_solves == n_iters and got["ncoll"] < 40               # ... and the per-pass collectives are gone
            held = ~np.isnan(got["dist"])
            assert held.sum() == (z1 - z0) * N * N and held[z0 * N * N:(z1 * N * N)].all()      # exactly its own planes came back
        else:
            assert got["ncoll"] > (30 if transport == "rccl-perpass" else 3)   # RCCL all-reduces of a one-rank communicator (the per-frame rows need none: solved inside the sweeps)
    # the slabs tile the volume and the band: stitched together they are the single-context result (the slabs sum their dot products in a
    # different order than one context does)
    assert np.array_equal(np.concatenate([g["band"] for g in res]), band)
    d = stitch(res, "dist"); rgb = stitch(res, "rgb")
    margins(slab_vs_single={"dist_max_vs": float(np.abs(d[band] - v["dist"][band]).max() / vs), "rgb_max": float(np.abs(rgb[:, band] - v["rgb"][:, band]).max()),
                            "e_total_rel": float(max(np.abs(np.array(g["e_total"]) / np.array([x["e_total"] for x in recs]) - 1).max() for g in res)),
                            "pose_max": float(max(np.abs(g["poses"] - ref.download_poses()).max() for g in res))},
            tolerance={"dist_max_vs": 1e-4, "rgb_max": 1e-2 if model == "SH2" else 2e-4, "e_total_rel": 2e-4 if model == "SH2" else 5e-6, "pose_max": 2e-5 if model == "SH2" else 1e-6})
    assert np.abs(d[band] - v["dist"][band]).max() <= 1e-4 * vs      # (SH2 too: 2.6e-5 achieved, profiles/r04_parity_margins.json)
    assert np.abs(rgb[:, band] - v["rgb"][:, band]).max() <= (1e-2 if model == "SH2" else 2e-4)   # SH2: float32 9x9 light blocks of cond ~2e4 (tests/test_parity_gpu.py LIGHT_RTOL) amplify the all-reduce's summation order
    off = ~np.isin(np.arange(len(d)), band)
    assert np.array_equal(d[off], v["dist"][off])                     # voxels outside the band are untouched
    if world > 1:
        cuts = sorted((int(g["info"][6]), int(g["info"][7])) for g in res)
        assert cuts[0][0] == 0 and cuts[-1][1] == N and all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
        own = [int(g["info"][1] - g["info"][0]) for g in res]
        assert max(own) <= 1.35 * min(own)                            # cut by band count (plane granularity), not by height


def test_native_slab_refinement(built, tmp_path):
    """two ranks through the 2x refinement (PsOptimizer.cpp:386-409): halo planes refreshed, every slab refines the planes it holds, keeps the
    inner refined halo plane, rebuilds its band -- then another iteration -- against the single-context run of the same calls"""
    res = run_ranks(tmp_path, "SH1", 2, "gloo", "refine", 24, 2)
    sc = synth.make_scene(N=24, F=6, W=160, H=120, model="SH1")
    st = capi.default_settings(capi.SH1)
    ref = capi.load_engine(sc, sc.K, st, 0); ref.load_scene(sc)
    ref.init_albedo(); ref.normalize_weights()
    recs = ref.iterate(capi.ALL, 2); ref.upsample2x(); recs += ref.iterate(capi.ALL, 1)
    band = ref.download_band(); v = ref.download_volume(); vs = float(ref.info().voxel_size)
    assert list(ref.info().dim) == [48, 48, 48]
    for got in res:
        assert list(got["dim"]) == [48, 48, 48] and int(got["n_band"]) == len(band)
        assert np.allclose(got["e_total"], [x["e_total"] for x in recs], rtol=1e-5)
    assert np.array_equal(np.concatenate([g["band"] for g in res]), band)      # the refined slabs tile the refined band
    d = stitch(res, "dist")
    assert np.abs(d[band] - v["dist"][band]).max() <= 1e-4 * vs
    assert res[0]["info"][7] == res[1]["info"][6] == 2 * (res[0]["info"][7] // 2)     # the cut doubled with the grid


@pytest.mark.parametrize("model,world", [("SH1", 2), ("LED", 3)])
def test_slab_optimize_with_speculative_start(built, tmp_path, model, world):
    """psgsdf_optimize on slabs: the stop decision of every iteration is taken while the next iteration's albedo / light sweeps already run (the
    closing energy is all-reduced right behind the first of them; the window closes at the same program point on every rank) -- bit for bit what the
    loop that decides first produces (PSGSDF_SPECULATE_MR=0), and the single context's result to the slab tolerances, through the 2x refinement."""
    N, cap = 24, 18
    res = run_ranks(tmp_path, model, world, "gloo", "optimize", N, cap)
    (tmp_path / "decide_first").mkdir()
    res0 = run_ranks(tmp_path / "decide_first", model, world, "gloo", "optimize", N, cap, {"PSGSDF_SPECULATE_MR": "0"})
    for a, b in zip(res, res0):
        assert int(a["spec"][0]) >= 3 and int(b["spec"][0]) == 0                 # windows were opened / none
        for key in ("dist", "rgb", "poses", "light", "e_total", "cg", "upsampled"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    sc = synth.make_scene(N=N, F=5, W=160, H=120, model=model)
    st = capi.default_settings(sc.model_id, upsample=1, max_it=cap, conv_threshold=0.0, damping=10.0, **({"reg_weight_n": 0.1, "reg_weight_l": 5.0} if model == "LED" else {}))
    ref = capi.load_engine(sc, sc.K, st, 0); ref.load_scene(sc)
    ref.init_albedo(); ref.normalize_weights()
    recs, conv = ref.optimize(capi.ALL)
    band = ref.download_band(); v = ref.download_volume(); vs = float(ref.info().voxel_size)
    for got in res:
        assert len(got["e_total"]) == len(recs) and int(got["conv"]) == int(conv)
        assert list(got["upsampled"]) == [int(r["upsampled"]) for r in recs] and sum(got["upsampled"]) == 1      # the refinement after iteration 5 happened on the slabs too
        assert np.allclose(got["e_total"], [x["e_total"] for x in recs], rtol=2e-5)
    assert np.array_equal(np.concatenate([g["band"] for g in res]), band)
    d = stitch(res, "dist")
    assert np.abs(d[band] - v["dist"][band]).max() <= 1e-4 * vs


def test_a_lost_halo_push_is_an_error_not_a_hang(built, tmp_path):
    """Every wait inside a kernel for another rank is bounded.  Rank 1 of 2 skips its third halo push (PSGSDF_FAULT_HALO; the bound shortened to 2^16
    polls): rank 0's pull gives up, fills the halo rows with NaN and says so in a host-mapped word (the NaN alone is not enough: a CG over NaN sums
    never reports Success, and the reference's rule then skips the update); the other rank meets the failure in its next exchange with rank 0.
    Both report PSGSDF_ERR_DEVICE -- no rank hangs, no rank returns a result."""
    port = free_port(); out = str(tmp_path / "slab")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PSGSDF_XWAIT_LOG2="16", SLAB_FAULT_HALO="3")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_slab_worker_gpu.py"), str(r), "2", str(port), "SH1", out, "3", "40", "gloo", "iterate"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=150)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode not in (0, None) for p in procs), [p.returncode for p in procs]
    # (whichever check sees it first: the distance solve's "published NaN" or the read-back's "NaN came back from an exchange")
    assert all(("NaN came back from an exchange" in o or "published NaN" in o or "gave up" in o) and "PsgsdfError" in o for o in outs), [o[-600:] for o in outs]
    assert any("halo pull 3 gave up" in o for o in outs), [o[-600:] for o in outs]      # the rank whose pull expired names the exchange
    assert not os.path.exists(out + ".rank0.npz") and not os.path.exists(out + ".rank1.npz")


@pytest.mark.parametrize("world,mode", [(2, "fuse"), (3, "fuse_rebalance")])
def test_slab_parallel_front_end(built, tmp_path, world, mode):
    """SURVEY 8f row 1 "trivially z-slab parallel" (VERDICT r03 item 7): psgsdf_volume_init / psgsdf_integrate_frame / psgsdf_track on contexts attached
    to ranks.  Every rank fuses the six frames into the z-planes it holds (cut by height: the band does not exist yet) -- weights, visibility words,
    distances, gradients and colours of the stitched slabs equal the single context's BIT FOR BIT; the tracker's 6x6 system is summed over the
    ranks (each counts the pixels whose nearest voxel it owns) and every rank obtains the single context's pose; psgsdf_rebalance_slabs re-cuts
    the fused volume into slabs of equal band count and moves the planes; then keyframes, init and two Gauss-Newton iterations as usual."""
    N, n_iters = 40, 2
    res = run_ranks(tmp_path, "SH1", world, "gloo", mode, N, n_iters)
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model="SH1")
    ref = capi.load_engine(sc, sc.K, capi.default_settings(capi.SH1), 0)
    ref.volume_init(sc.F)
    for f in range(sc.F):
        ref.integrate_frame(sc.images[f], sc.depth[f], ref.estimate_normals(sc.depth[f]), sc.poses_gt[f], f, z_min=0.05, z_max=10.0)
    P, iters, conv = ref.track(sc.depth[1], sc.poses_gt[0], z_min=0.05, z_max=10.0, num_iterations=3)
    fused = ref.download_volume(); fvis = ref.download_vis_seq(1)
    ref.set_keyframes(np.arange(sc.F, dtype=np.int32), sc.images, sc.poses); ref.init()
    ref.init_albedo(); e0 = ref.normalize_weights()
    recs = ref.iterate(capi.ALL, n_iters)
    band = ref.download_band(); v = ref.download_volume(); vs = float(sc.voxel_size)
    # ---- fusion: the stitched slabs are the single context's volume, bit for bit
    assert np.array_equal(stitch(res, "fused_weight"), fused["weight"]) and np.array_equal(stitch(res, "fused_dist"), fused["dist"])
    own_vis = np.zeros_like(fvis)
    for g in res:
        z0, z1 = int(g["info"][6]), int(g["info"][7])
        own_vis[z0 * N * N:z1 * N * N] = g["fused_vis"][z0 * N * N:z1 * N * N]
    assert np.array_equal(own_vis, fvis) and fvis.any()
    # ---- tracker: the same pose on every rank, the single context's to rounding (per-thread float sums over different pixel subsets)
    for g in res:
        assert np.abs(g["track"][:16].reshape(4, 4) - P).max() <= 2e-6 and int(g["track"][16]) == iters and bool(g["track"][17]) == conv
        assert np.array_equal(g["track"], res[0]["track"])
    # ---- the cut: by height after volume_init; by band count after psgsdf_rebalance_slabs
    uniform = [(r * N // world, (r + 1) * N // world) for r in range(world)]
    assert [tuple(int(x) for x in g["cut_before"]) for g in res] == uniform
    cuts = [(int(g["info"][6]), int(g["info"][7])) for g in res]
    own = [int(g["info"][1] - g["info"][0]) for g in res]
    if mode == "fuse_rebalance":
        assert cuts != uniform and max(own) <= 1.35 * min(own)      # (three equal-height slabs of a sphere hold very different band counts)
    else:
        assert cuts == uniform
    assert cuts[0][0] == 0 and cuts[-1][1] == N and all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
    # ---- and the optimisation on the slab-fused volume is the single context's
    for g in res:
        assert abs(float(g["e0"]) - e0) <= 1e-6 * abs(e0) and np.allclose(g["e_total"], [x["e_total"] for x in recs], rtol=5e-6)
    assert np.array_equal(np.concatenate([g["band"] for g in res]), band)
    d = stitch(res, "dist")
    assert np.abs(d[band] - v["dist"][band]).max() <= 1e-4 * vs


@pytest.mark.parametrize("world", [2, 3])
def test_slab_local_upload(built, tmp_path, world):
    """psgsdf_plan_slab + psgsdf_upload_volume_slab (no rank hands over -- or ever looks at -- more than its own z-planes and one halo plane per
    inner side; the cut negotiation is one all-reduce of a per-plane histogram that the ranks fill in turns): the same cuts, the same band rows and
    the same bits as the whole-volume upload of psgsdf_upload_volume on every rank."""
    res = run_ranks(tmp_path, "SH1", world, "gloo", "iterate_slab", 40, 2)
    (tmp_path / "w").mkdir()
    ref = run_ranks(tmp_path / "w", "SH1", world, "gloo", "iterate", 40, 2)
    for a, b in zip(res, ref):
        assert list(a["info"]) == list(b["info"])                       # same cuts, same row ranges, same halos
        assert np.array_equal(a["band"], b["band"]) and np.array_equal(a["e_total"], b["e_total"]) and np.array_equal(a["cg"], b["cg"])
        assert np.array_equal(a["dist"], b["dist"], equal_nan=True) and np.array_equal(a["rgb"], b["rgb"], equal_nan=True) and np.array_equal(a["poses"], b["poses"])


def test_rccl_path_with_two_ranks_on_one_device_fails_cleanly(built, tmp_path):
    """A dry run of the RCCL transport at N = 2 on the one-GPU box: both ranks load librccl, exchange the unique id and
    call ncclCommInitRank for the SAME device.  RCCL refuses that; what matters here is that the bootstrap of two ranks completes and that the
    refusal comes back through the C ABI as PSGSDF_ERR_COMM with RCCL's message on BOTH ranks within seconds -- no hang, no crash."""
    import time
    port = free_port(); out = str(tmp_path / "dup")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_SOCKET_IFNAME="lo")
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_slab_worker_gpu.py"), str(r), "2", str(port), "SH1", out, "1", "24", "rccldup", "iterate"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=150)
            outs.append((p.returncode, o))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert time.time() - t0 < 150
    for rc, o in outs:
        assert rc == 3 and "COMM_ERROR" in o and "ncclCommInitRank" in o and "rc=-5" in o, o[-1500:]


@pytest.mark.parametrize("masks,memkind", [("0:128,128:256", None), ("0:64,64:128,128:192,192:256", None), ("0:128,128:256", "uncached")])
def test_cross_rank_persistent_solve_on_disjoint_cu_halves(built, tmp_path, masks, memkind):
    """the persistent distance solve ACROSS ranks, developed on the one-GPU box by giving each of two ranks half the CUs
    (PSGSDF_CU_MASK -> hipExtStreamCreateWithCUMask), so that both persistent kernels are resident while they exchange halo records and rank sums
    through IPC-mapped memory: 96^3, two iterations, against the single-context engine to 1e-4 voxel.  Four ranks on CU quarters: a
    rank's granules reach ranks that are not its neighbours, possibly before those have even started their solve -- the epoch tags make that harmless.
    "uncached": the record planes in hipDeviceMallocUncached memory (what the probe falls back to if fine-grained memory does not carry the
    hand-offs between two real devices)."""
    N, n_iters = 96, 2
    world = masks.count(",") + 1
    env = {"SLAB_CU_MASKS": masks}
    if memkind:
        env["PSGSDF_XR_MEM"] = memkind
    res = run_ranks(tmp_path, "SH1", world, "gloo", "iterate", N, n_iters, env)
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model="SH1")
    ref = capi.load_engine(sc, sc.K, capi.default_settings(capi.SH1), 0); ref.load_scene(sc)
    ref.init_albedo(); ref.normalize_weights()
    recs = ref.iterate(capi.ALL, n_iters)
    band = ref.download_band(); v = ref.download_volume(); vs = float(sc.voxel_size)
    for got in res:
        assert int(got["xr"][0]) == 1 and int(got["xr"][1]) >= 1 and int(got["xr"][2]) <= 1      # (a fallback under host load is tolerated, see above)
        assert int(got["xr"][3]) == (2 if memkind == "uncached" else 1) and int(got["xr"][4]) == 0 and int(got["xr"][5]) == 0
        assert np.allclose(got["e_total"], [x["e_total"] for x in recs], rtol=5e-6)
        assert np.all(np.abs(got["cg"] - np.array([x["cg_iters"] for x in recs])) <= 1)
    d = stitch(res, "dist")
    assert np.abs(d[band] - v["dist"][band]).max() <= 1e-4 * vs


EIGHTHS = ",".join(f"{32 * i}:{32 * i + 32}" for i in range(8))


@pytest.mark.parametrize("model,N,frames,mode", [("SH1", 96, None, "iterate"), ("SH2", 64, "70:96:72", "iterate"), ("LED", 64, None, "iterate"), ("SH1", 24, None, "iterate"), ("SH1", 16, None, "iterate"), ("SH1", 24, None, "optimize")])
def test_eight_ranks_on_cu_eighths(built, margins, tmp_path, model, N, frames, mode):
    """WORLD SIZE 8 -- the machine BASELINE.json names -- rehearsed on the one-GPU box: eight processes, each confined to an eighth
    of the CUs (PSGSDF_CU_MASK=0:32, 32:64, ...), so that the eight persistent solve kernels are resident together while they exchange halo records,
    rank granules, frame rows and scalar folds through IPC-mapped memory.  Seven inner cut planes, band-count cuts over eight slabs, rank-order sums
    over eight granules, the hand-off probe over seven neighbour pairs.  SH2 with 70 keyframes: TWO visibility words per voxel in slab mode
    (configs[4]'s layout); N = 24: slabs of one or two planes -- thinner than the three planes a stencil spans, a rank's two halo planes belong to
    ranks that are its neighbours' neighbours' neighbours in the band; "optimize": the product loop through the 2x refinement with the speculative
    start.  All against the single context: every band voxel within 1e-4 voxel, cross-rank solves on every rank, NO fallback."""
    n_iters = 18 if mode == "optimize" else 2
    env = {"SLAB_CU_MASKS": EIGHTHS}
    if frames:
        env["SLAB_FRAMES"] = frames
    res = run_ranks(tmp_path, model, 8, "gloo", mode, N, n_iters, env, timeout=280)
    fr = [int(x) for x in frames.split(":")] if frames else []
    sc = synth.make_scene(N=N, F=fr[0] if fr else (5 if mode == "optimize" else 6), W=fr[1] if fr else 160, H=fr[2] if fr else 120, model=model)
    kw = dict(upsample=1, max_it=n_iters, conv_threshold=0.0, damping=10.0) if mode == "optimize" else {}
    st = capi.default_settings(sc.model_id, **kw)
    ref = capi.load_engine(sc, sc.K, st, 0); ref.load_scene(sc)
    ref.init_albedo(); e0 = ref.normalize_weights()
    if mode == "optimize":
        recs, conv = ref.optimize(capi.ALL)
    else:
        recs = ref.iterate(capi.ALL, n_iters)
    band = ref.download_band(); v = ref.download_volume(); vs = float(ref.info().voxel_size)
    if frames:
        assert sc.vis_words == 2
    planes = []
    for got in res:
        xr_ready, xr_solves, fallbacks, mem_kind, probe_stale, probe_to = (int(x) for x in got["xr"])
        assert xr_ready == 1 and xr_solves >= 1 and fallbacks == 0, (xr_ready, xr_solves, fallbacks)
        assert mem_kind == 1 and probe_stale == 0 and probe_to == 0
        assert len(got["e_total"]) == len(recs)
        assert np.allclose(got["e_total"], [x["e_total"] for x in recs], rtol=2e-4 if model == "SH2" else 2e-5 if mode == "optimize" else 5e-6)
        assert np.all(np.abs(got["cg"] - np.array([x["cg_iters"] for x in recs])) <= 1)
        assert np.abs(got["poses"] - ref.download_poses()).max() <= (2e-5 if model == "SH2" else 2e-6)
        planes.append(int(got["info"][7]) - int(got["info"][6]))
    cuts = [(int(g["info"][6]), int(g["info"][7])) for g in res]
    nz = int(ref.info().dim[2])
    assert cuts[0][0] == 0 and cuts[-1][1] == nz and all(cuts[i][1] == cuts[i + 1][0] for i in range(7)) and min(planes) >= 1
    if N <= 24 and mode == "iterate":
        assert min(planes) <= (1 if N == 16 else 2), planes              # slabs thinner than a stencil (N = 16: ONE plane -- both halo planes of its neighbours are this rank's only plane)
    assert np.array_equal(np.concatenate([g["band"] for g in res]), band)
    d = stitch(res, "dist"); rgb = stitch(res, "rgb")
    m = {"dist_max_vs": float(np.abs(d[band] - v["dist"][band]).max() / vs), "rgb_max": float(np.abs(rgb[:, band] - v["rgb"][:, band]).max()), "planes_per_rank": planes,
         "band_rows_per_rank": [int(g["info"][1] - g["info"][0]) for g in res], "cross_rank_solves": [int(g["xr"][1]) for g in res]}
    margins(eight_ranks_vs_single=m, tolerance={"dist_max_vs": 1e-4})
    assert m["dist_max_vs"] <= 1e-4
    assert m["rgb_max"] <= (1e-2 if model == "SH2" else 2e-4)
