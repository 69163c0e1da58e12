"""One context walked through every path on which it lets go of memory and takes new (a second volume, keyframes of another count and of the
other pixel format, the refined grid, wider visibility words, larger frames) ends on the BITS of a fresh context that only ever saw the final
inputs: nothing of what a context held before may show in what it computes.  No tolerance anywhere: equal as bytes."""
import numpy as np
import pytest

from psgradientsdf_amd import capi, synth

pytestmark = pytest.mark.gpu

_ENERGIES = ("e_after", "e_n", "e_l", "e_total", "e_r", "e_n_in", "e_l_in", "cg_iters")


def snapshot(api, records):
    """everything the comparison looks at, by name, as bytes"""
    s = {f"iter{i}.{k}": np.asarray(r[k], np.float64).tobytes() for i, r in enumerate(records) for k in _ENERGIES}
    v = api.download_volume()
    for k in ("dist", "grad", "weight", "rgb"):
        s["volume." + k] = np.ascontiguousarray(v[k]).tobytes()
    s["poses"] = np.ascontiguousarray(api.download_poses()).tobytes()
    s["light"] = np.ascontiguousarray(api.download_light()).tobytes()
    s["band"] = np.ascontiguousarray(api.download_band()).tobytes()
    return s


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if a[k] != b[k]]


def prepare(api, sc, n_iters, frames=slice(None), normalize=True):
    api.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)
    api.set_keyframes(sc.frame_idx[frames], sc.images[frames], sc.poses[frames])
    api.init(); api.init_albedo()
    if normalize:
        api.normalize_weights()
    return api.iterate(capi.ALL, n_iters)


@pytest.mark.parametrize("model", ["SH1", "LED"])
def test_walked_context_ends_on_the_bits_of_a_fresh_one(built, model):
    sc = synth.make_scene(N=40, F=6, W=160, H=120, model=model)
    st = capi.default_settings(sc.model_id)
    u8 = np.clip(np.rint(sc.images * 255.0), 0, 255).astype(np.uint8)
    A = capi.load_engine(sc, sc.K, st, 0)
    # four keyframes, one iteration: band, lists, accumulators of another size.  Without normalize_weights: it SCALES the regulariser weights the
    # context holds (reg_weight_n *= E / E_n, as the reference does once per run), and no later call puts them back -- a second normalisation on one
    # context starts from the first one's result (measured: reg_weight_n 6879.59 instead of 288.497 on this scene), which is the interface's
    # behaviour and no business of the memory this test is about.
    prepare(A, sc, 1, frames=slice(0, 4), normalize=False)
    A.set_keyframes_u8(sc.frame_idx, u8, 1.0 / 255.0, sc.poses)                  # float -> 8-bit images ...
    A.set_keyframes(sc.frame_idx, sc.images, sc.poses)                           # ... and back
    A.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)   # the volume again, over the one that was optimised
    A.init(); A.init_albedo(); A.normalize_weights()
    ra = A.iterate(capi.ALL, 2)
    B = capi.load_engine(sc, sc.K, st, 0)
    rb = prepare(B, sc, 2)
    assert A.info().n_band == B.info().n_band > 1000
    assert differing(snapshot(A, ra), snapshot(B, rb)) == []
    # the refined grid: the dense planes change hands
    for api in (A, B):
        api.upsample2x()
    ra, rb = A.iterate(capi.ALL, 1), B.iterate(capi.ALL, 1)
    assert A.info().n_band == B.info().n_band > 4000
    assert differing(snapshot(A, ra), snapshot(B, rb)) == []


def test_fusion_regrows_its_buffers(built):
    """the second frame is larger (device and pinned staging and the normals cache are replaced) and its number lies beyond what
    volume_init was told (the visibility words are widened): the same volume as in a context that was told from the start"""
    small = synth.make_scene(N=40, F=6, W=96, H=72, model="SH1")
    large = synth.make_scene(N=40, F=6, W=160, H=120, model="SH1")
    st = capi.default_settings(capi.SH1)
    out = []
    for max_frames in (64, 128):
        api = capi.load_engine(large, large.K, st, 0)
        api.volume_init(max_frames)
        for sc, f, counter in ((small, 0, 0), (large, 1, 70)):      # (normals: the engine's own, through its cache)
            api.integrate_frame(sc.images[f], sc.depth[f], api.estimate_normals(sc.depth[f]), sc.poses_gt[f], counter)
        v = api.download_volume()
        out.append((v, api.download_vis_seq(2)))
    (va, sa), (vb, sb) = out
    assert (va["weight"] > 0).sum() > 1000 and (sa[:, 0] != 0).any() and (sa[:, 1] != 0).any()
    for k in ("dist", "grad", "weight", "rgb"):
        assert va[k].tobytes() == vb[k].tobytes(), k
    assert sa.tobytes() == sb.tobytes()
