"""N ranks of a worker script on the one GPU: the launcher of the multi-rank tests and the workers' side of it.  These tests start several GPU
processes on a machine others use too, so how they are started, bounded and reaped is written here once.

The test's side: run_ranks (any worker), run_spec (the workers with the command line RANK WORLD SPEC.json OUT), stitch.
The worker's side: arm before the context exists, engine to create it and attach it to its peers."""
import faulthandler
import json
import os
import socket
import subprocess
import sys

import numpy as np

NCU = 256      # MI355X
FDS, CU_MASKS = "RANKS_FDS", "RANKS_CU_MASKS"      # a rank's peer sockets "fd,fd,..." (-1: itself); every rank's CU range "a:b,a:b,..."
TESTS = os.path.dirname(os.path.abspath(__file__))


def socket_mesh(world):
    """one connected stream-socket pair per pair of ranks: mesh[r][q] = rank r's end of its connection to rank q (psgsdf_comm_init_sockets)"""
    mesh = [[-1] * world for _ in range(world)]
    for r in range(world):
        for q in range(r + 1, world):
            a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
            mesh[r][q], mesh[q][r] = a.detach(), b.detach()
    return mesh


def run_ranks(worker, argv, world, timeout, env=None, mesh=True, split=True, names=(FDS, CU_MASKS)):
    """`world` processes of tests/<worker>, rank r with the arguments argv[r], all of which must exit with status 0 within `timeout` seconds each
    (waited for in rank order); the caller loads what they wrote.  mesh: a socket pair per pair of ranks, rank r inheriting its own ends only, named
    in the variable names[0]; split: rank r confined to the r-th of `world` equal CU ranges, all of them named in names[1].  One rank gets neither.
    env: more environment.  No rank outlives the call."""
    assert world <= 16, "at most 16 processes may hold the GPU at a time"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {}))
    if split and world > 1:
        env[names[1]] = ",".join(f"{r * NCU // world}:{(r + 1) * NCU // world}" for r in range(world))
    fds = socket_mesh(world) if mesh and world > 1 else [[] for _ in range(world)]
    procs = []
    try:
        try:
            for r in range(world):
                procs.append(subprocess.Popen([sys.executable, os.path.join(TESTS, worker)] + [str(a) for a in argv[r]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                              env=dict(env, **{names[0]: ",".join(str(f) for f in fds[r])}) if fds[r] else env, pass_fds=[f for f in fds[r] if f >= 0]))
        finally:
            for f in (f for row in fds for f in row if f >= 0):      # the parent's copies: a rank's death must reach its peers as a closed connection
                os.close(f)
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, o[-3000:]
    finally:
        for p in procs:      # a rank that is still alive here would keep the GPU (and the next test) busy
            if p.poll() is None:
                p.kill()


def run_spec(worker, tmp_path, tag, ext, world, timeout, spec):
    """run_ranks for the workers with the command line RANK WORLD SPEC.json OUT; spec["timeout"], the worker's own limit, defaults to 20 s less than the
    launcher's.  Returns the ranks' result files."""
    spec.setdefault("timeout", timeout - 20)
    sp = str(tmp_path / f"{tag}.json"); json.dump(spec, open(sp, "w"))
    outs = [str(tmp_path / f"{tag}.rank{r}.{ext}") for r in range(world)]
    run_ranks(worker, [[r, world, sp, outs[r]] for r in range(world)], world, timeout)
    return outs


def stitch(res, key):
    """the slabs tile the volume: every rank filled the z-planes it owns, NaN elsewhere"""
    out = np.full_like(res[0][key], np.nan)
    for got in res:
        m = ~np.isnan(got[key]); assert not (m & ~np.isnan(out)).any(); out[m] = got[key][m]
    assert not np.isnan(out).any()
    return out


# ---- the worker's side
def arm(rank, spec):
    """first thing in a worker: its own time limit (a traceback, then exit) and, for ranks sharing the one GPU, its CU range -- before the context is created"""
    faulthandler.dump_traceback_later(int(spec.get("timeout", 100)), exit=True)
    if os.environ.get(CU_MASKS):
        os.environ["PSGSDF_CU_MASK"] = os.environ[CU_MASKS].split(",")[rank]


def engine(sc, rank, world):
    """the scene's context with default settings, attached to its peers over the launcher's sockets (world 1: a plain single-rank context)"""
    from psgradientsdf_amd import capi
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    if world > 1:
        eng.comm_init_sockets([int(x) for x in os.environ[FDS].split(",")], rank, world)
    return eng
