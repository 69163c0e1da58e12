"""worker of tests/test_render_ranks_gpu.py: one rank of a world-N context (the engine's socket transport; N = 1: a plain single-rank context) that
loads a synthetic scene -- or a stitched state -- and records what the collective render calls return, or runs a few iterations and records the state.

    python _render_ranks_worker.py RANK WORLD SPEC.json OUT.npz      (started by tests/_ranks.py run_spec: peer sockets and CU range in its variables)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats_row(st):
    return np.array([st["n_pixels"], st["n_hits"], st["n_hits_off_band"], *st["sum_r2"], *st["sum_abs_r"], st["robust"]], np.float64)


def cameras(eng, world):
    """caller cameras of the tests: down the z axis, up it, a horizontal one whose pixel row through cy has rays parallel to the slab planes,
    one inside the volume (in the second slab along z, a middle one from three ranks on), and a narrow one down onto the top of the object"""
    import _render_ref as ref
    i = eng.info()
    vs, dim, org = float(i.voxel_size), np.array(i.dim[:], np.float64), np.array(i.origin[:], np.float64)
    ext, c = vs * dim, org + vs * (dim - 1) / 2
    if world > 1:      # the z-planes of every rank's slab, in z order
        mi = eng.mg_info()
        cut = np.zeros(2 * world); cut[2 * mi["rank"]], cut[2 * mi["rank"] + 1] = mi["z0"], mi["z1"]
        cut = sorted(eng.comm_allreduce_host(cut).reshape(world, 2).tolist())
        zmid = org[2] + vs * 0.5 * (cut[1][0] + cut[1][1])
    else:
        zmid = c[2]

    def pose(x, y, z, eye):
        P = np.eye(4); P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
        return P
    W, H = 64, 48
    K = [56.0, 56.0, 31.5, 24.0]        # cy on a pixel row: dc[1] == 0 exactly there
    cams = [dict(name="down", pose=pose([1, 0, 0], [0, -1, 0], [0, 0, -1], c + [0, 0, 1.1 * ext[2]]), K=K, size=(W, H)),
            dict(name="up", pose=pose([1, 0, 0], [0, 1, 0], [0, 0, 1], c - [0, 0, 1.1 * ext[2]]), K=K, size=(W, H)),
            dict(name="level", pose=pose([1, 0, 0], [0, 0, -1], [0, 1, 0], c - [0, 1.1 * ext[1], 0]), K=K, size=(W, H)),
            dict(name="inside", pose=ref.look_at([org[0] + 0.08 * ext[0], c[1] + 0.05 * ext[1], zmid], [c[0], c[1], zmid - 0.1 * ext[2]]), K=K, size=(W, H)),
            dict(name="narrow", pose=pose([1, 0, 0], [0, -1, 0], [0, 0, -1], c + [0, 0, 1.1 * ext[2]]), K=[400.0, 400.0, 7.5, 7.5], size=(16, 16))]
    for k in cams:
        k["pose"] = np.asarray(k["pose"], np.float32).reshape(16).tolist()
    return cams


def main(rank, world, spec, out):
    import _ranks
    _ranks.arm(rank, spec)
    from psgradientsdf_amd import capi, synth
    model = spec["model"]
    sc = synth.make_scene(N=spec["N"], F=spec["F"], W=spec["W"], H=spec["H"], model=model, u8=spec["u8"])
    if spec.get("empty"):      # nothing observed with weight: the band (and so the partition) stays, no cell can hold a hit
        sc.weight = np.zeros_like(sc.weight)
    light = None
    if spec.get("state"):      # a stitched state of an earlier run: volume, poses, light
        z = np.load(spec["state"])
        sc.dist, sc.grad, sc.weight, sc.rgb = (np.ascontiguousarray(z[k]).reshape(np.shape(getattr(sc, k))) for k in ("dist", "grad", "weight", "rgb"))
        sc.poses = np.ascontiguousarray(z["poses"]); light = z["light"]
    eng = _ranks.engine(sc, rank, world)
    eng.load_scene(sc, u8=spec["u8"])
    if light is None:      # the light is loaded (the scene's own: LED [3], SH [F][nb]), not initialised from the (rank-order) sums of the volume
        light = sc.light_gt
    eng.upload_light(np.ascontiguousarray(light, np.float32))
    res = {}
    if spec["phase"] == "iterate":
        eng.init_albedo()
        eng.normalize_weights()
        eng.iterate(capi.ALL, spec["iters"])
    v = eng.download_volume()
    mi = eng.mg_info() if world > 1 else {"z0": 0, "z1": int(eng.info().dim[2]), "row0": 0, "row1": int(eng.info().n_band)}
    res.update(dist=v["dist"], grad=v["grad"], weight=v["weight"], rgb=v["rgb"], poses=eng.download_poses(), light=eng.download_light(),
               band=eng.download_band(mi["row1"] - mi["row0"]), cut=[mi["z0"], mi["z1"]], dim=list(eng.info().dim))
    if spec["phase"] == "render":
        cams = spec.get("cams") or cameras(eng, world)
        res["cams"] = json.dumps(cams)
        for f in range(sc.F):
            r = eng.render(frame=f)
            for k, a in r.items():
                res[f"kf{f}_{k}"] = stats_row(a) if k == "stats" else a
        for j, k in enumerate(cams):
            r = eng.render(pose=k["pose"], K=k["K"], size=k["size"], light_frame=j % sc.F)
            for q, a in r.items():
                res[f"cam{j}_{q}"] = stats_row(a) if q == "stats" else a
        res["report"] = np.stack([stats_row(s) for s in eng.render_report()])
    elif spec["phase"] == "mismatch":      # rank r asks for its own view: every rank must get PSGSDF_ERR_ARG
        k = cameras(eng, world)[0]
        p = np.array(k["pose"], np.float32); p[3] += np.float32(0.001 * rank)
        try:
            eng.render(pose=p, K=k["K"], size=k["size"])
            res["error"] = ""
        except capi.PsgsdfError as ex:
            res["error"] = str(ex)
        res["after"] = stats_row(eng.render(frame=0)["stats"])      # the context is still usable (and the ranks still in step)
    np.savez(out, **res)
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
