"""worker of tests/test_relight_gpu.py: one rank of a world-N context (the engine's socket transport).  psgsdf_relight is not a collective call: the
ranks listed in spec["callers"] call it, the others do not, and nobody may wait for anybody.  Afterwards every rank takes part in the collective
psgsdf_extract_mesh_indexed, which must still work.

    python _relight_ranks_worker.py RANK WORLD SPEC.json OUT.json      (peer sockets: MESH_FDS, CU range: MESH_CU_MASKS)
"""
import faulthandler
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(rank, world, spec, out):
    faulthandler.dump_traceback_later(int(spec.get("timeout", 100)), exit=True)
    if os.environ.get("MESH_CU_MASKS"):      # ranks sharing the one GPU on disjoint CU ranges
        os.environ["PSGSDF_CU_MASK"] = os.environ["MESH_CU_MASKS"].split(",")[rank]
    from psgradientsdf_amd import capi, synth
    sc = synth.make_scene(N=spec["N"], F=spec["F"], W=160, H=120, model="SH1")
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.comm_init_sockets([int(x) for x in os.environ["MESH_FDS"].split(",")], rank, world)
    eng.load_scene(sc)
    eng.init_albedo()
    errors = []
    if rank in spec["callers"]:
        for lights in ([dict(kind="directional", vec=[0, 0, 1], samples=16, spread=0.1)], [dict(kind="sh", sh=[1, 0, 0, 0])]):
            try:
                eng.relight(lights, frame=0)
                errors.append("")
            except capi.PsgsdfError as e:
                errors.append(str(e))
    xyz, nrm, rgb, faces, first = eng.extract_mesh_indexed()
    json.dump({"errors": errors, "faces": int(len(faces)), "first": int(first)}, open(out, "w"))
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), json.load(open(sys.argv[3])), sys.argv[4])
