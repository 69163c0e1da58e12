"""worker of tests/test_mesh_indexed_gpu.py: one rank of a world-N context (the engine's socket transport) that brings a synthetic scene to a state
and records its share of the welded mesh (psgsdf_extract_mesh_indexed, a collective call) and its planes of the volume.

    python _mesh_ranks_worker.py RANK WORLD SPEC.json OUT.npz      (started by tests/_ranks.py run_spec: peer sockets and CU range in its variables)
spec: model, N, F, mode = iterate (2 iterations) | refine (2 iterations, the 2x refinement, 1 more) | fuse_rebalance (slab-parallel fusion, re-cut, 1 iteration)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(rank, world, spec, out):
    import _ranks
    _ranks.arm(rank, spec)
    from psgradientsdf_amd import capi, synth
    sc = synth.make_scene(N=spec["N"], F=spec["F"], W=160, H=120, model=spec["model"])
    eng = _ranks.engine(sc, rank, world)
    mode = spec["mode"]
    if mode == "fuse_rebalance":      # every rank fuses every frame into the planes it holds, then the slabs are re-cut
        eng.volume_init(sc.F)
        for f in range(sc.F):
            eng.integrate_frame(sc.images[f], sc.depth[f], eng.estimate_normals(sc.depth[f]), sc.poses_gt[f], f, z_min=0.05, z_max=10.0)
        eng.rebalance_slabs()
        eng.set_keyframes(np.arange(sc.F, dtype=np.int32), sc.images, sc.poses); eng.init()
    else:
        eng.load_scene(sc)
    eng.init_albedo()
    eng.normalize_weights()
    eng.iterate(capi.ALL, 1 if mode == "fuse_rebalance" else 2)
    if mode == "refine":
        eng.upsample2x()
        eng.iterate(capi.ALL, 1)
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    again = eng.extract_mesh_indexed()
    v = eng.download_volume()
    mi = eng.mg_info()
    i = eng.info()
    np.savez(out, xyz=xyz, nrm=nrm, rgb=rgb, faces=faces, first=first, same_again=all(np.array_equal(a, b) for a, b in zip((xyz, nrm, rgb, faces, first), again)),
             dist=v["dist"], grad=v["grad"], weight=v["weight"], rgb_vol=v["rgb"], cut=[mi["z0"], mi["z1"]], dim=list(i.dim), vs=i.voxel_size)
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
