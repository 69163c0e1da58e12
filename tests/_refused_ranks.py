"""driver of the test_ranks_are_refused_before_any_exchange tests: the calls of one family (tests/_refused_ranks_worker.py FAMILIES) made by rank 1
alone of a two-rank context.  A refusal that had become collective would leave rank 1 waiting for rank 0 until the worker's own limit."""
import json
import os
import subprocess
import sys

from test_mesh_indexed_gpu import NCU, _socket_mesh


def refused_ranks(tmp_path, family, N=40, F=4):
    """both ranks' results: {"errors": one text per call made ("" if it succeeded), "faces", "first": of the collective mesh afterwards}"""
    world, timeout = 2, 150
    sp = str(tmp_path / "spec.json"); json.dump({"family": family, "N": N, "F": F, "callers": [1], "timeout": timeout - 20}, open(sp, "w"))
    mesh = _socket_mesh(world)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MESH_CU_MASKS=",".join(f"{r * NCU // world}:{(r + 1) * NCU // world}" for r in range(world)))
    outs = [str(tmp_path / f"rank{r}.json") for r in range(world)]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_refused_ranks_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), sp, outs[r]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(env, MESH_FDS=",".join(str(f) for f in mesh[r])), pass_fds=[f for f in mesh[r] if f >= 0]) for r in range(world)]
    for row in mesh:
        for f in row:
            if f >= 0:
                os.close(f)
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, o[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [json.load(open(o)) for o in outs]
