"""View rendering and the keyframe report on multi-rank (z-slab) contexts (include/psgsdf_render.h, DESIGN.md 9, "Multi-rank contexts"): two to four ranks share the one
GPU on disjoint CU ranges and meet through the engine's socket transport.  Every rank must return the planes and stats a single-rank context holding
the same state returns, bit for bit (planes compared as uint32, stats as float64 bits), while each rank holds only its slab."""
import json
import os
import subprocess

import numpy as np
import pytest

from _ranks import NCU, run_spec, stitch

pytestmark = pytest.mark.gpu


def run(tmp_path, tag, world, timeout=120, **spec):
    """world ranks of the worker (1: a plain single-rank context); returns every rank's npz"""
    return [dict(np.load(o)) for o in run_spec("_render_ranks_worker.py", tmp_path, tag, "npz", world, timeout, spec)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_same_state(ranks, one):
    """the N-rank contexts and the single-rank one hold the same volume, band, poses and light, bit for bit"""
    for k in ("dist", "grad", "weight", "rgb"):
        assert same(stitch(ranks, k), one[k]), k
    order = sorted(range(len(ranks)), key=lambda r: int(ranks[r]["cut"][0]))
    assert same(np.concatenate([ranks[r]["band"] for r in order]), one["band"])
    for got in ranks:
        assert same(got["poses"], one["poses"]) and same(got["light"], one["light"])


def render_keys(d):
    return sorted(k for k in d if k.startswith(("kf", "cam")) and k != "cams" or k == "report")


def assert_same_renders(ranks, one):
    keys = render_keys(one)
    assert keys and all(render_keys(got) == keys for got in ranks)
    for got in ranks:                      # every rank returns the single-rank planes and stats
        for k in keys:
            assert same(got[k], one[k]), k


def cuts(ranks):
    return sorted(int(got["cut"][0]) for got in ranks)[1:]


def slab_hit_counts(ranks, one, dim):
    """per view: first hits in each rank's slab (from the voxel plane's global linear index)"""
    bounds = sorted((int(g["cut"][0]), int(g["cut"][1])) for g in ranks)
    out = {}
    for k in one:
        if k.endswith("_voxel"):
            v = one[k][one[k] >= 0].astype(np.int64)
            z = v // (int(dim[0]) * int(dim[1]))
            out[k] = [int(((z >= a) & (z < b)).sum()) for a, b in bounds]
    return out


@pytest.mark.parametrize("world,model,u8", [(2, "SH1", False), (3, "LED", True), (4, "SH2", False)])
def test_views_and_report_equal_the_single_rank_context(built, tmp_path, world, model, u8):
    spec = dict(model=model, N=44, F=5, W=96, H=72, u8=u8, phase="render")
    ranks = run(tmp_path, "ranks", world, **spec)
    one = run(tmp_path, "one", 1, cams=json.loads(str(ranks[0]["cams"])), **spec)[0]
    assert_same_state(ranks, one)
    assert all(str(got["cams"]) == str(ranks[0]["cams"]) for got in ranks)
    assert_same_renders(ranks, one)
    F = spec["F"]
    for f in range(F):                     # report row f == the single view of keyframe f, on N ranks as on one
        assert same(ranks[0]["report"][f], ranks[0][f"kf{f}_stats"]), f
    # the scene really exercises the partition: a brick straddles a cut, and some view has no first hit in some rank's slab
    c = cuts(ranks)
    counts = slab_hit_counts(ranks, one, one["dim"])
    print(f"{world} ranks {model} u8={u8}: cuts {c}, first hits per slab {counts}")
    assert any(z % 8 for z in c), c
    assert any(0 in v for v in counts.values())
    assert all(one[f"kf{f}_stats"][1] > 0 for f in range(F))
    for j, name in enumerate(["down", "up", "level", "inside", "narrow"]):
        assert one[f"cam{j}_stats"][1] > 0, name
    # the level camera's row through cy: rays parallel to the slab planes, hits on it
    assert (one["cam2_voxel"][24] >= 0).any()


@pytest.mark.parametrize("world,model,u8", [(2, "SH1", True), (4, "LED", False)])
def test_iterated_state_renders_equal(built, tmp_path, world, model, u8):
    """a few iterations on N ranks; the stitched state loaded into a fresh N-rank and a fresh single-rank context renders equal"""
    spec = dict(model=model, N=40, F=4, W=80, H=64, u8=u8)
    it = run(tmp_path, "iter", world, phase="iterate", iters=2, **spec)
    st = str(tmp_path / "state.npz")
    np.savez(st, **{k: stitch(it, k) for k in ("dist", "grad", "weight", "rgb")}, poses=it[0]["poses"], light=it[0]["light"])
    ranks = run(tmp_path, "ranks", world, phase="render", state=st, **spec)
    one = run(tmp_path, "one", 1, phase="render", state=st, cams=json.loads(str(ranks[0]["cams"])), **spec)[0]
    assert_same_state(ranks, one)
    assert_same_renders(ranks, one)
    assert one["kf0_stats"][1] > 0


def test_empty_volume_gives_misses_on_every_rank(built, tmp_path):
    ranks = run(tmp_path, "empty", 3, model="SH1", N=32, F=3, W=64, H=48, u8=False, phase="render", empty=True)
    for got in ranks:
        for k in render_keys(got):
            if k.endswith("_voxel"):
                assert (got[k] == -1).all(), k
            elif k.endswith("_stats"):
                assert got[k][0] > 0 and not got[k][1:].any(), k
            elif k == "report":
                assert not got[k][:, 1:].any()
            else:
                assert not got[k].any(), k


def test_mismatched_views_are_an_argument_error_on_every_rank(built, tmp_path):
    ranks = run(tmp_path, "mismatch", 2, timeout=90, model="SH1", N=32, F=3, W=64, H=48, u8=False, phase="mismatch")
    for got in ranks:
        assert "rc=-1" in str(got["error"]), str(got["error"])
        assert got["after"][1] > 0
    assert same(ranks[0]["after"], ranks[1]["after"])


def test_voxelps_render_keyframes_on_ranks(built, margins, tmp_path):
    """voxelPS --gpus 2 --render-keyframes: the single-process run's render/ files and report lines (numbers within what the two runs' states
    differ by); every other file byte-identical to a 2-rank run without the flag"""
    from PIL import Image
    from test_voxelps_ranks_gpu import EXE, config
    ranks = 2
    env = {"VOXELPS_SHARE_GPU": "1", "VOXELPS_CU_MASKS": ",".join(f"{r * NCU // ranks}:{(r + 1) * NCU // ranks}" for r in range(ranks))}
    outs = {}
    for name, extra, e in (("one", ["--render-keyframes"], {}), ("ranks", ["--gpus", str(ranks), "--transport", "sockets", "--render-keyframes"], env),
                           ("plain", ["--gpus", str(ranks), "--transport", "sockets"], env)):
        out = str(tmp_path / name) + "/"; os.makedirs(out)
        r = subprocess.run([EXE, "--config_file", config(out, **{"max iter": 6})] + extra, capture_output=True, text=True, timeout=300, env=dict(os.environ, **e))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = out

    def files(d):
        return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)
    skip = ("config.json", "saved_config.json")
    one, rk, plain = files(outs["one"]), files(outs["ranks"]), files(outs["plain"])
    rend = [f for f in rk if f.startswith("render")]
    assert rend == [f for f in one if f.startswith("render")] and "render_report.txt" in rend and len(rend) > 4
    assert [f for f in rk if f not in rend] == plain
    for f in plain:
        if f not in skip:
            assert open(outs["ranks"] + f, "rb").read() == open(outs["plain"] + f, "rb").read(), f
    la = [l.split() for l in open(outs["one"] + "render_report.txt") if not l.startswith("#")]
    lb = [l.split() for l in open(outs["ranks"] + "render_report.txt") if not l.startswith("#")]
    assert len(la) == len(lb) > 0 and [a[0] for a in la] == [b[0] for b in lb]
    im = Image.open(os.path.join(outs["one"], rend[0]))
    npx = im.size[0] * im.size[1]
    dh = max(abs(int(a[1]) - int(b[1])) for a, b in zip(la, lb)) / npx
    drel = max(abs(float(a[k]) - float(b[k])) / max(abs(float(a[k])), 1e-30) for a, b in zip(la, lb) for k in (3, 5))
    dpng = max(float(np.abs(np.asarray(Image.open(outs["one"] + f), np.int16) - np.asarray(Image.open(outs["ranks"] + f), np.int16)).mean()) for f in rend if f.endswith(".png"))
    margins(hits_frac=dh, rel_rmse_robust=drel, png_mean_abs_u8=dpng)
    print(f"voxelPS 2 ranks vs one process: hits differ by {dh:.2e} of the pixels, rmse / robust by {drel:.2e} relative, PNG bytes by {dpng:.3f} on average")
    # the two runs end in states that differ in the last bits of rank-order sums (test_voxelps_ranks_gpu.py): the renders agree to that extent
    assert dh <= 2e-3 and drel <= 1e-2 and dpng <= 0.5
