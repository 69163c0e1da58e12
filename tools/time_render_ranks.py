"""Cost of view rendering on a multi-rank context (include/psgsdf_render.h, DESIGN.md 9, "Multi-rank contexts"): N ranks share the one GPU on disjoint CU ranges and
meet through the engine's socket transport -- a rehearsal of the collective calls, not a scaling measurement.  Wall-clock per call of one keyframe
view with every plane and of the report over all keyframes, and the bytes each rank puts into the all-reduces:
    python tools/time_render_ranks.py [ranks] [grid] [frames] [reps]"""
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NCU = 256      # MI355X


def rank_main(rank, world, N, F, reps):
    os.environ["PSGSDF_CU_MASK"] = f"{rank * NCU // world}:{(rank + 1) * NCU // world}"
    from psgradientsdf_amd import capi, synth
    sc = synth.make_scene(N=N, F=F, W=640, H=480, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.comm_init_sockets([int(x) for x in os.environ["RENDER_FDS"].split(",")], rank, world)
    eng.load_scene(sc)
    eng.render(frame=0)
    eng.render_report()                                     # (warm-up: code objects, allocations)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = eng.render(frame=0)
    t_view = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.render_report()
    t_rep = (time.perf_counter() - t0) / reps
    i = eng.info()
    bricks = 1
    for d in i.dim:
        bricks *= (int(d) + 7) // 8
    first = 8 * (bricks + 2 * world)                        # brick marks, every rank's z0 and call checksum
    px = 640 * 480
    if rank == 0:
        print(json.dumps({"ranks": world, "grid": N, "keyframes": F, "size": [640, 480], "view_ms": round(1e3 * t_view, 3), "report_ms": round(1e3 * t_rep, 3),
                          "bytes_view_all_planes": first + 8 * px * (1 + 13), "bytes_report": first + 8 * px * F * (1 + 4), "hits_frame0": r["stats"]["n_hits"]}), flush=True)
    eng.close()


def main():
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    F = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    mesh = [[-1] * world for _ in range(world)]
    for r in range(world):
        for q in range(r + 1, world):
            a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_STREAM)
            mesh[r][q], mesh[q][r] = a.detach(), b.detach()
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), str(world), str(N), str(F), str(reps)],
                              env=dict(os.environ, RENDER_FDS=",".join(str(f) for f in mesh[r])), pass_fds=[f for f in mesh[r] if f >= 0]) for r in range(world)]
    for row in mesh:
        for f in row:
            if f >= 0:
                os.close(f)
    rc = 0
    for p in procs:
        rc |= p.wait()
    sys.exit(rc)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--rank":
        rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        main()
