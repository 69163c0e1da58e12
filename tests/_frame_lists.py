"""Scenes whose per-keyframe observation lists end where the frame-major sweeps and `build_band` partition them (tests/test_frame_lists_cpu.py,
tests/test_frame_lists_gpu.py): `skew` edits a scene's visibility so that named keyframes see a chosen number of band voxels, `CASES` are the scenes
both files run, `frame_counts` reads the lists' lengths back from a band."""
import copy

import numpy as np

from psgradientsdf_amd import capi, synth


def frame_bit(vis, f):
    """bool [nvox]: visibility bit of frame f (bit f & 63 of word f >> 6)"""
    return ((vis[:, f >> 6] >> np.uint64(f & 63)) & np.uint64(1)).astype(bool)


def skew(sc, counts, pick="spread"):
    """A shallow copy of `sc` with only `sc.vis` replaced: frame f of `counts` keeps its bit on counts[f] of its band candidates (voxels with
    |dist| <= sqrt(3) voxel and any bit set that carry bit f) and loses it everywhere else, outside the band too; frames not named keep their bits.
    pick (one name, or {frame: name} with "spread" for the rest): "spread" = indices round(linspace(0, len - 1, n)) of the frame's candidates, so that
    the kept voxels cover the frame's whole view; "first" / "last" = the n lowest / highest linear indices."""
    vis = sc.vis.copy()
    near = (np.abs(sc.dist.reshape(-1)) <= np.sqrt(3) * sc.voxel_size) & (sc.vis != 0).any(axis=1)
    for f, n in counts.items():
        how = pick.get(f, "spread") if isinstance(pick, dict) else pick
        cand = np.nonzero(near & frame_bit(sc.vis, f))[0]
        assert 0 <= n <= len(cand), (f, n, len(cand))
        if how == "spread":
            keep = cand[np.round(np.linspace(0, len(cand) - 1, n)).astype(np.int64)] if n else cand[:0]
        elif how == "first":
            keep = cand[:n]
        elif how == "last":
            keep = cand[len(cand) - n:]
        else:
            raise ValueError(how)
        bit = np.uint64(1) << np.uint64(f & 63)
        vis[:, f >> 6] &= ~bit
        vis[keep, f >> 6] |= bit
        assert int(frame_bit(vis, f).sum()) == n == len(np.unique(keep)), (f, n)
    out = copy.copy(sc)
    out.vis = np.ascontiguousarray(vis)
    return out


def frame_counts(band, vis, F):
    """length of every keyframe's observation list: band rows that carry the frame's bit"""
    return [int(frame_bit(vis[band], f).sum()) for f in range(F)]


LED_KW = dict(reg_weight_n=0.1, reg_weight_l=5.0, damping=3.0)      # config_basket_LED.json, as elsewhere in the suite
MODEL_ID = {"SH1": capi.SH1, "SH2": capi.SH2, "LED": capi.LED}

# name -> (scene arguments, u8, counts, pick, settings).  A: lists that end one short of, on and one past the default chunk of 1024 observations, and an
# empty one; B: wavefront (64) and workgroup (256) boundaries, lists of one and of no observation at the first and near the last blockIdx.y, a list
# from the band's first rows only and one from its last 2048-row block only; B1: one keyframe sees anything at all; C: the boundary between the two
# visibility words; D: lists rebuilt by the 2x refinement.
_B = {0: 1, 1: 63, 2: 64, 3: 65, 4: 255, 5: 256, 6: 257, 7: 0, 8: 300, 9: 300}
_B_PICK = {8: "first", 9: "last"}
_A = {2: 0, 4: 1023, 5: 1024, 6: 1025}
CASES = {
    "A-SH1": (dict(N=32, F=7, W=128, H=96, model="SH1"), False, _A, "spread", {}),
    "A-SH1-u8": (dict(N=32, F=7, W=128, H=96, model="SH1", u8=True), True, _A, "spread", {}),
    "A-SH2": (dict(N=32, F=14, W=128, H=96, model="SH2"), False, _A, "spread", {}),
    "A-LED": (dict(N=32, F=7, W=128, H=96, model="LED"), False, _A, "spread", LED_KW),
    "B-SH1": (dict(N=32, F=11, W=128, H=96, model="SH1"), False, _B, _B_PICK, {}),
    "B-LED": (dict(N=32, F=11, W=128, H=96, model="LED"), False, _B, _B_PICK, LED_KW),
    "B1-SH1": (dict(N=32, F=11, W=128, H=96, model="SH1"), False, {f: 0 for f in range(10)}, "spread", {}),
    "B1-LED": (dict(N=32, F=11, W=128, H=96, model="LED"), False, {f: 0 for f in range(10)}, "spread", LED_KW),
    "C-SH1": (dict(N=32, F=70, W=96, H=72, model="SH1"), False, {63: 0, 64: 1024, 65: 0, 69: 1025}, "spread", {}),
    "D-SH1": (dict(N=24, F=5, W=128, H=96, model="SH1"), False, {1: 0, 3: 512}, "spread", dict(upsample=1, max_it=8, conv_threshold=0.0)),
    # With the default damping the reference's loop leaves through its divergence exit at iteration 5 on this scene, BEFORE the refinement (and so does
    # the unedited scene of tests/test_edge_gpu.py test_laplacian_and_upsample_schedule at iteration 6): damping 10 carries it through the refinement
    # (tests/test_parity_gpu.py test_optimize_matches_oracle), so that one more iteration runs on the rebuilt lists.
    "D-SH1-refined": (dict(N=24, F=5, W=128, H=96, model="SH1"), False, {1: 0, 3: 512}, "spread", dict(upsample=1, max_it=8, conv_threshold=0.0, damping=10.0)),
}
STATE_CASES = ["A-SH1", "A-SH1-u8", "A-SH2", "A-LED", "C-SH1"]      # two iterations compared with the oracle
OPTIMIZE_CASES = ["D-SH1", "D-SH1-refined"]                          # a whole optimisation

# what the GPU file asserts (tests/test_edge_gpu.py compare, tests/test_parity_gpu.py LIGHT_RTOL x 3 as test_iterations); the CPU file holds the oracle's
# own FMA build to a third of each
LIGHT_RTOL = {"SH1": 1e-4, "SH2": 1e-3, "LED": 1e-4}
TOL = {"dist_vs": 1e-4, "pose": 1e-5, "e_total_rel": 2e-4}
TOL_D_E = 2e-3
NE_TOL = 2e-5      # per-frame normal equations (tests/test_parity_gpu.py test_normal_equations), relative to the frame's largest oracle entry


def light_tol(name):
    return 3 * LIGHT_RTOL[name]


_scenes = {}


def scene(case):
    """(skewed scene, u8, requested counts, settings) of a case; the synthesised scene is shared by the cases with the same arguments"""
    args, u8, counts, pick, kw = CASES[case]
    key = tuple(sorted(args.items()))
    if key not in _scenes:
        _scenes[key] = synth.make_scene(**args)
    sc = skew(_scenes[key], counts, pick)
    return sc, u8, counts, capi.default_settings(MODEL_ID[args["model"]], **kw)


def model_of(case):
    return CASES[case][0]["model"]


def expected_counts(sc, counts, band):
    """the lists' lengths in `band` from the edited visibility, after asserting that the named frames have exactly what was asked"""
    got = frame_counts(band, sc.vis, sc.F)
    assert all(got[f] == n for f, n in counts.items()), (counts, got)
    return got


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
