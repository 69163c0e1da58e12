"""Relighting on the device (include/psgsdf_relight.h, csrc/relight.hip).  The floor-and-wall volume of test_relight_cpu against
closed form: the device's per-pixel count of occluded rays must equal the analytic one wherever no ray of the pixel is within 1e-3 voxels of its
limit; the analytic plane; the geometry planes and an SH light against psgsdf_render bit for bit; the device against the yardstick
tests/_relight_ref.py started from the device's OWN geometry planes (the interface returns a pixel's count, not its rays' bits: a pixel whose
count differs by d has at least d differing rays, and the sum of those is held under 2e-3 of the rays, the project's cap for this walk);
monotonicity in the reach, reproducibility, errors, ranks and `voxelPS --relight`."""
import json
import os

import numpy as np
import pytest

import _relight_ref as lref
import _render_ref as rref
from _refused_ranks import refused_ranks
from psgradientsdf_amd import capi, synth
from test_mesh_components_gpu import vs_of
from test_occlusion_cpu import VS, corner_volume
from test_relight_cpu import FOCAL, H, INTR, NEAR_SHARE, W, corner_analytic, corner_cases, corner_pose
from test_render_voxelps_gpu import GOLD, _files, _run

pytestmark = pytest.mark.gpu
f32 = np.float32
RAY_SHARE = 2e-3
GEO = ("depth", "normal", "albedo", "voxel")


def volume_engine(v, dim, vs, pose, K, Wk, Hk, truncation=5.0):
    """test_mesh_components_gpu.upload plus two keyframes at `pose` and psgsdf_init: relighting is valid where rendering is"""
    g = capi.GridDesc(); g.dim[:] = [int(x) for x in dim]; g.voxel_size = vs; g.shift[:] = [0.0, 0.0, 0.0]; g.truncation = truncation * vs
    eng = capi.load_engine(g, K, capi.default_settings(capi.SH1), 0)
    n = int(np.prod(dim))
    eng.upload_volume(v["dist"], v["grad"], v["weight"], v["rgb"], np.where(v["weight"] > 0, 1, 0).astype(np.uint64).reshape(n, 1), 1)
    eng.set_keyframes(np.arange(2, dtype=np.int32), np.full((2, Hk, Wk, 3), 0.5, f32), np.stack([np.asarray(pose, f32).reshape(16)] * 2))
    eng.init()
    return eng


def counts_of(vis, K):
    """the occluded rays of every pixel from its visibility (K - c) / K: exact, both are small integers over a power of two"""
    c = K - vis.astype(np.float64) * K
    assert np.array_equal(c, np.round(c))
    return c.astype(np.int64)


def assert_consistent(r, l, geo, K, lit=None):
    """what follows from the planes exactly: misses and unlit pixels hold the defined values, the counts are the planes' sums"""
    hit = geo["voxel"] >= 0
    vis, ren, cn = r["visibility"][l], r["rendered"][l], r["counts"][l]
    assert tuple(cn) == lref.COUNTS
    assert not vis[~hit].any() and not ren[:, ~hit].any()
    assert cn["n_hits"] == int(hit.sum()) and cn["n_rays"] == K * cn["n_lit"] and 0 <= cn["n_buried"] <= cn["n_occluded"]
    if lit is not None:
        assert cn["n_lit"] == int(lit.sum()) and not vis[hit & ~lit].any()
        assert cn["n_occluded"] == int(counts_of(vis, K)[lit].sum())


@pytest.fixture(scope="module")
def corner(built):
    v, dim = corner_volume()
    # the device's volume has its own origin (shift 0: minus half the grid): the scene is placed relative to it
    probe = capi.GridDesc(); probe.dim[:] = list(dim); probe.voxel_size = VS; probe.shift[:] = [0.0, 0.0, 0.0]; probe.truncation = 5 * VS
    e0 = capi.load_engine(probe, np.array([FOCAL, 0, INTR[2], 0, FOCAL, INTR[3], 0, 0, 1], f32), capi.default_settings(capi.SH1), 0)
    origin = tuple(float(x) for x in e0.info().origin)
    e0.close()
    eng = volume_engine(v, dim, VS, corner_pose(origin), np.array([FOCAL, 0, INTR[2], 0, FOCAL, INTR[3], 0, 0, 1], f32), W, H)
    assert tuple(float(x) for x in eng.info().origin) == origin
    return eng, origin


@pytest.mark.parametrize("case", range(9))
def test_corner_equals_the_closed_form(corner, case):
    eng, origin = corner
    vs = vs_of(eng)
    name, light, bias, reach, expected = corner_cases(origin)[case]
    r = eng.relight([light], frame=0, bias=bias * vs, reach=reach * vs, geometry=True)
    geo = {k: r[k] for k in GEO}
    hit = geo["voxel"] >= 0
    assert hit.all()
    # the definition's rays from the device's own planes (the walk of the yardstick is not needed: no volume)
    empty = dict(dist=np.ones(8, f32), grad=np.zeros((3, 8), f32), weight=np.zeros(8, f32), rgb=np.zeros((3, 8), f32))
    y = lref.relight(empty, (2, 2, 2), vs, origin, corner_pose(origin), INTR, geo, [light], bias * vs, reach * vs)[0]
    K, lit = y["K"], y["lit"]
    bits, t, near = corner_analytic(y["o"], y["w"], y["limit"], origin)
    assert_consistent(r, 0, geo, K, lit)
    dev = counts_of(r["visibility"][0], K)
    clear = lit & ~near.any(-1)
    differ = clear & (dev != bits.sum(-1))
    cn = r["counts"][0]
    print(f"{name}: {cn['n_lit']} lit pixels, {cn['n_occluded']} of {cn['n_rays']} rays occluded (closed form {int(bits[lit].sum())}, float64 run on the stored gradients {expected[0]} of {expected[1]}), "
          f"{cn['n_buried']} buried, {int(differ.sum())} pixels differ, {int(near[lit].sum())} rays within 1e-3 vs of the limit")
    assert near[lit].sum() <= NEAR_SHARE * max(cn["n_rays"], 1)
    assert not differ.any()
    if not near[lit].any():
        assert cn["n_occluded"] == int(bits[lit].sum())
    # lit, unshadowed pixels whose normal is the floor's: rho (ambient + colour cosv fall), the cosine and fall-off in closed form at the hit point
    floor = lit & (dev == 0) & (geo["normal"][2] == 1) & (geo["normal"][0] == 0) & (geo["normal"][1] == 0)
    if floor.any():
        q = y["o"] - bias * vs * np.array([0.0, 0.0, 1.0])
        vec = np.asarray(light["vec"], f32).astype(np.float64)
        d = np.broadcast_to(vec, q.shape) if light["kind"] == "directional" else vec - q
        cosv = d[..., 2] / np.linalg.norm(d, axis=-1)
        fall = 1.0 if light["kind"] == "directional" else 1.0 / (d * d).sum(-1)
        exp = geo["albedo"].astype(np.float64) * (cosv * fall)[None]
        err = np.abs(r["rendered"][0][:, floor] / exp[:, floor] - 1).max()
        print(f"{name}: rendered against the closed form on {int(floor.sum())} floor pixels: {err:.2e} relative")
        assert err < 1e-6


def test_analytic_plane(built):
    vs, N, off = 0.01, 48, 0.004
    dim, _, dist, grad, weight, n = rref.plane_volume(N=N, vs=vs, offset=off)
    Wp, Hp, fx = 96, 72, 80.0
    cx, cy = (Wp - 1) / 2.0, (Hp - 1) / 2.0
    pose = rref.look_at(0.62 * n + np.array([0.03, -0.02, 0.0]), np.zeros(3)).astype(f32)
    v = dict(dist=dist, grad=grad, weight=weight, rgb=np.full((3, len(dist)), 0.5, f32))
    eng = volume_engine(v, dim, vs, pose, np.array([fx, 0, cx, 0, fx, cy, 0, 0, 1], f32), Wp, Hp, truncation=3.0)
    colour = [1.0, 0.5, 0.25]
    above = [dict(kind="directional", vec=list(n + [0.1, 0.05, 0.0]), colour=colour), dict(kind="directional", vec=list(n), colour=colour, spread=0.2, samples=64)]
    r = eng.relight(above + [dict(kind="directional", vec=list(-n), colour=colour, samples=8), dict(kind="point", vec=list(-0.3 * n), samples=16, spread=0.01)], frame=0, geometry=True)
    geo = {k: r[k] for k in GEO}
    hit = geo["voxel"] >= 0
    assert hit.mean() > 0.5
    for l, L in enumerate(above):
        assert_consistent(r, l, geo, L.get("samples", 1), hit)
        assert (r["visibility"][l][hit] == 1).all() and r["counts"][l]["n_occluded"] == 0
        wc = np.asarray(L["vec"], f32).astype(np.float64); wc /= np.linalg.norm(wc)
        m = geo["normal"].astype(np.float64); m /= np.where(hit, np.sqrt((m * m).sum(0)), 1.0)
        exp = geo["albedo"].astype(np.float64) * np.asarray(colour)[:, None, None] * (m * wc[:, None, None]).sum(0)[None]
        assert np.abs(r["rendered"][l][:, hit] / exp[:, hit] - 1).max() < 1e-6
    for l, K in ((2, 8), (3, 16)):      # below the plane: every hit is unlit
        assert_consistent(r, l, geo, K, np.zeros_like(hit))
        assert r["counts"][l]["n_rays"] == 0 and r["counts"][l]["n_lit"] == 0 and not r["visibility"][l].any() and not r["rendered"][l].any()


def scene(model, N=32):
    sc = synth.make_scene(N=N, F=6, W=160, H=120, model=model)
    eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    eng.load_scene(sc)
    eng.init_albedo()
    eng.iterate(capi.ALL, 2)
    return eng, sc


@pytest.fixture(scope="module")
def sh1(built):
    return scene("SH1")


def scene_lights(eng, sc):
    """a directional and a point light for the synthetic scene (a bumpy sphere of radius 0.34 N vs seen from 1.5 N vs): both from the side of
    camera 0, so that the terminator crosses the view and the soft lights' discs dip below the horizon of many pixels; 16 rays each"""
    P0 = eng.download_poses()[0].reshape(4, 4).astype(np.float64)
    eye, fwd, right = P0[:3, 3], P0[:3, 2], P0[:3, 0]
    Nvs = int(eng.info().dim[0]) * vs_of(eng)
    side = (right - 0.3 * fwd) / np.linalg.norm(right - 0.3 * fwd)
    return [dict(kind="directional", vec=list(side), colour=[1.0, 0.9, 0.8], ambient=[0.05, 0.05, 0.1], spread=0.2, samples=16),
            dict(kind="point", vec=list(eye + 1.5 * Nvs * fwd + 0.6 * Nvs * side), colour=[0.02, 0.02, 0.02], spread=3 * vs_of(eng), samples=16)]


@pytest.mark.parametrize("model,n_sh", [("SH1", 4), ("SH2", 9)])
def test_geometry_and_sh_light_equal_render(built, sh1, model, n_sh):
    eng, sc = sh1 if model == "SH1" else scene("SH2")
    light = eng.download_light()
    for f in (0, 3):
        ref = eng.render(frame=f)
        r = eng.relight([dict(kind="sh", sh=light[f][:n_sh]), dict(kind="sh", sh=light[f][:n_sh], colour=[0.5, 1.0, 2.0], ambient=[0.25, 0, 0])], frame=f, geometry=True)
        for k in GEO:
            assert r[k].dtype == ref[k].dtype and r[k].tobytes() == ref[k].tobytes(), (model, f, k)
        hit = ref["voxel"] >= 0
        assert hit.sum() > 1000
        assert r["rendered"][0].tobytes() == ref["rendered"].tobytes(), (model, f)      # colour 1, ambient 0: the forward model's own product
        assert np.array_equal(r["visibility"][0], hit.astype(f32))
        assert r["counts"][0] == dict(n_hits=int(hit.sum()), n_lit=int(hit.sum()), n_rays=0, n_occluded=0, n_buried=0)
        exp = (ref["albedo"].astype(np.float64) * (np.array([0.25, 0, 0])[:, None, None] + np.array([0.5, 1.0, 2.0])[:, None, None] * ref["shading"].astype(np.float64)[None])).astype(f32)
        assert np.array_equal(r["rendered"][1][:, hit], exp[:, hit])
    # a caller's camera: the geometry of psgsdf_render for the same camera (light_frame is ignored)
    pose = eng.download_poses()[1]
    ref = eng.render(pose=pose, K=sc.K, size=(150, 97), light_frame=2)
    r = eng.relight([dict(kind="sh", sh=light[2][:n_sh])], pose=pose, K=sc.K, size=(150, 97), geometry=True)
    for k in GEO:
        assert r[k].tobytes() == ref[k].tobytes(), (model, k)
    assert r["rendered"][0].tobytes() == ref["rendered"].tobytes()


def test_device_against_the_yardstick(sh1):
    eng, sc = sh1
    vs = vs_of(eng)
    lights = scene_lights(eng, sc)
    r = eng.relight(lights, frame=0, bias=vs, reach=0.0, geometry=True)
    geo = {k: r[k] for k in GEO}
    v = eng.download_volume()
    dim = [int(x) for x in eng.info().dim]
    k = np.asarray(sc.K, np.float64).reshape(-1)
    y = lref.relight(v, dim, vs, list(eng.info().origin), eng.download_poses()[0], (k[0], k[4], k[2], k[5]), geo, lights, vs, 0.0)
    for l, (L, yl) in enumerate(zip(lights, y)):
        K = L["samples"]
        assert_consistent(r, l, geo, K, yl["lit"])
        dev = counts_of(r["visibility"][l], K)
        d = np.where(yl["lit"], np.abs(dev - yl["count"]), 0)
        share = d.sum() / max(yl["n_rays"], 1)
        cn = r["counts"][l]
        print(f"{L['kind']} K {K}: {cn['n_lit']} lit of {cn['n_hits']} hits, {cn['n_occluded']} of {cn['n_rays']} rays occluded ({cn['n_buried']} buried), yardstick {yl['n_occluded']} ({yl['n_buried']}); "
              f"at least {int(d.sum())} rays differ ({share:.2e}) on {int((d > 0).sum())} pixels")
        assert cn["n_lit"] > 500 and cn["n_occluded"] <= cn["n_rays"]
        assert share <= RAY_SHARE, (L["kind"], share)
        same = (geo["voxel"] >= 0) & (d == 0)
        big = same & (np.abs(yl["rendered"]).max(0) > 0)
        err = np.abs(r["rendered"][l][:, big].astype(np.float64) - yl["rendered"][:, big]).max(0) / np.abs(yl["rendered"][:, big]).max(0)
        print(f"{L['kind']} K {K}: rendered where the counts agree: {err.max():.2e} relative")
        assert err.max() < 1e-6


def test_monotonic_reproducible_and_leaves_the_state_alone(sh1):
    eng, sc = sh1
    vs = vs_of(eng)
    lights = scene_lights(eng, sc) + [dict(kind="sh", sh=[0.6, 0.1, 0.2, -0.5]), dict(kind="directional", vec=[0.3, 0.2, -1.0], samples=64, spread=0.3)]
    xyz, nrm = eng.extract_mesh_indexed()[:2]
    before = (eng.render_report(), eng.extract_mesh_indexed(), eng.occlusion_points(xyz, nrm))
    a = eng.relight(lights, frame=1, reach=8 * vs, geometry=True)
    b = eng.relight(lights, frame=1, reach=8 * vs, geometry=True)
    for k in ("rendered", "visibility") + GEO:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"] == b["counts"]
    short = eng.relight(lights, frame=1, reach=4 * vs)
    for l, L in enumerate(lights):
        assert (short["visibility"][l] >= a["visibility"][l]).all()      # a shorter reach shadows a subset
        assert short["counts"][l]["n_occluded"] <= a["counts"][l]["n_occluded"] and short["counts"][l]["n_lit"] == a["counts"][l]["n_lit"]
    print("occluded rays at reach 4 and 8 voxels:", [(x["n_occluded"], y["n_occluded"]) for x, y in zip(short["counts"], a["counts"])])
    for l, L in enumerate(lights):      # one call with L lights: L calls with one light each
        one = eng.relight([L], frame=1, reach=8 * vs)
        assert one["rendered"][0].tobytes() == a["rendered"][l].tobytes() and one["visibility"][0].tobytes() == a["visibility"][l].tobytes() and one["counts"][0] == a["counts"][l]
    after = (eng.render_report(), eng.extract_mesh_indexed(), eng.occlusion_points(xyz, nrm))
    assert before[0] == after[0]
    for x, y in zip(before[1], after[1]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for k in ("mask", "occlusion", "dirs"):
        assert before[2][k].tobytes() == after[2][k].tobytes()
    assert before[2]["counts"] == after[2]["counts"]


def test_a_call_between_two_iterations_changes_nothing(built):
    ends = []
    for relight in (False, True):
        sc = synth.make_scene(N=32, F=3, W=64, H=48, model="SH1")
        eng = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
        eng.load_scene(sc)
        eng.init_albedo()
        eng.iterate(capi.ALL, 1)
        if relight:
            assert eng.relight(scene_lights(eng, sc), frame=0)["counts"][0]["n_rays"] > 1000
        eng.iterate(capi.ALL, 1)
        v = eng.download_volume()
        ends.append((v["dist"], v["grad"], v["rgb"], eng.download_poses(), eng.download_light()))
    for x, y in zip(*ends):
        assert x.tobytes() == y.tobytes()


def test_errors(sh1):
    eng, sc = sh1
    vs = vs_of(eng)
    good = dict(kind="directional", vec=[0, 0, -1.0], samples=8, spread=0.1)
    nan, inf = float("nan"), float("inf")
    bad_lights = [dict(good, vec=[0, 0, 0]), dict(good, vec=[0, nan, 1]), dict(good, samples=4), dict(good, samples=0), dict(good, samples=128), dict(good, samples=1), dict(good, spread=-0.1),
                  dict(good, spread=inf), dict(good, colour=[1, -1, 1]), dict(good, ambient=[nan, 0, 0]), dict(kind=3, vec=[0, 0, 1]), dict(kind="point", vec=[inf, 0, 0]),
                  dict(kind="sh", sh=[1, 0, 0]), dict(kind="sh", sh=[1, 0, 0, nan]), dict(kind="sh", sh=[1, 0, 0, 0], samples=8)]

    def refused(rc, lights=(good,), **kw):
        """the call returns rc and leaves the outputs untouched"""
        v, Wv, Hv = eng._view("relight", kw.pop("frame", 0), kw.pop("pose", None), kw.pop("K", None), kw.pop("size", None))
        for k, x in kw.pop("view", {}).items():
            setattr(v, k, x)
        arr = (capi.Light * max(len(lights), 1))(*[capi.make_light(d) for d in lights])
        p = capi.RelightParams(kw.get("bias", vs), kw.get("reach", 0.0), kw.get("n_lights", len(lights)), kw.get("reserved", 0))
        out = np.full((max(len(lights), 1), 4, 8, 8), 7.0, f32); geo = np.full((8, 8, 8), 7.0, f32); cnt = (capi.RelightCounts * max(len(lights), 1))()
        for c in cnt:
            c.n_hits = -7
        import ctypes as C
        got = eng._fn("relight")(eng.ctx, C.byref(v), arr, C.byref(p), out.ctypes.data_as(C.c_void_p), geo.ctypes.data_as(C.c_void_p), cnt)
        assert got == rc, (got, rc, lights, kw)
        assert (out == 7).all() and (geo == 7).all() and all(c.n_hits == -7 for c in cnt)

    ARG, UNSUPPORTED, STATE = -1, -3, -4
    for L in bad_lights:
        refused(ARG, [L])
        refused(ARG, [good, L])
    for kw in (dict(bias=0.0), dict(bias=-vs), dict(bias=nan), dict(bias=inf), dict(reach=-vs), dict(reach=nan), dict(reach=inf), dict(n_lights=0), dict(n_lights=65), dict(reserved=1),
               dict(view=dict(frame=6)), dict(view=dict(frame=1000)), dict(frame=None, pose=np.eye(4), K=sc.K, size=(0, 10)), dict(frame=None, pose=np.eye(4), K=[0, 1, 0, 0], size=(8, 8))):
        refused(ARG, **kw)
    refused(UNSUPPORTED, frame=None, pose=np.eye(4), K=sc.K, size=(4097, 4096))      # more than 2^24 pixels
    with pytest.raises(capi.PsgsdfError, match="rc=-1"):
        eng.relight([good] * 65, frame=0)
    assert eng.relight([good] * 64, frame=0)["visibility"].shape == (64, 120, 160)      # ... and 64 lights are served
    fresh = capi.load_engine(sc, sc.K, capi.default_settings(sc.model_id), 0)
    v = capi.View(); v.frame = -1; v.fx = v.fy = 100.0; v.width = v.height = 8
    v.pose[:] = [float(x) for x in np.eye(4).reshape(16)]
    import ctypes as C
    p, L, out = capi.RelightParams(vs, 0.0, 1, 0), capi.make_light(good), np.full((4, 8, 8), 7.0, f32)
    assert fresh._fn("relight")(fresh.ctx, C.byref(v), C.byref(L), C.byref(p), out.ctypes.data_as(C.c_void_p), None, None) == STATE and (out == 7).all()


def test_ranks_are_refused_before_any_exchange(built, tmp_path):
    """on a context attached to a rank: PSGSDF_ERR_UNSUPPORTED at once -- only rank 1 calls, so a collective refusal would hang -- and the
    context goes on working (the collective psgsdf_extract_mesh_indexed afterwards)"""
    res = refused_ranks(tmp_path, "relight")
    assert res[0]["errors"] == [] and len(res[1]["errors"]) == 2
    for e in res[1]["errors"]:
        assert "rc=-3" in e and "rank 1 of 2" in e and "relight" in e, e
    assert res[0]["faces"] + res[1]["faces"] > 1000 and res[0]["first"] == 0 and res[1]["first"] > 0


def test_voxelps_relight_on_sokrates(built, tmp_path):
    from PIL import Image
    a, b = str(tmp_path / "plain") + "/", str(tmp_path / "relight") + "/"
    lights = tmp_path / "lights.json"
    lights.write_text(json.dumps({"bias_voxels": 1, "reach_voxels": 0, "lights": [
        {"kind": "directional", "vec": [0.4, -0.3, -1.0], "colour": [1.0, 0.95, 0.9], "ambient": [0.05, 0.05, 0.08], "spread": 0.05, "samples": 16},
        {"kind": "point", "vec": [0.3, 0.0, 0.0], "colour": [0.6, 0.6, 0.6], "samples": 1}]}))
    _run(a, [])
    _run(b, ["--relight", str(lights)])
    plain, relit = _files(a), _files(b)
    extra = [f for f in relit if f not in plain]
    assert set(plain) <= set(relit)
    for f in plain:
        if f == "config.json" or f == "saved_config.json":
            continue                                                    # (they name the output directory)
        assert open(a + f, "rb").read() == open(b + f, "rb").read(), f
    rows = [l.split() for l in open(b + "relight_report.txt") if not l.startswith("#")]
    Wk, Hk = Image.open(os.path.join(GOLD, "color000001.png")).size
    names = sorted({r[0] for r in rows})
    assert len(names) >= 2 and len(rows) == 2 * len(names) and all(len(r) == 9 for r in rows)
    pngs = [f for f in extra if f.endswith(".png")]
    assert len(pngs) == 2 * len(rows) and "relight_report.txt" in extra and sorted(extra) == sorted(pngs + ["relight_report.txt"])
    for name, l, kind, samples, hits, lit, rays, occluded, buried in rows:
        assert kind == ("directional", "point")[int(l)] and int(samples) == (16, 1)[int(l)]
        assert int(hits) > 1000 and 0 < int(lit) <= int(hits) and int(rays) == int(samples) * int(lit) and 0 <= int(buried) <= int(occluded) <= int(rays)
        for suffix, mode in (("", "RGB"), ("_visibility", "L")):
            im = Image.open(os.path.join(b, "relight", f"{name}_light{int(l):02d}{suffix}.png"))
            assert im.size == (Wk, Hk) and im.mode == mode
            assert np.asarray(im).max() > 0
    print("sokrates relit after the run:", [(r[0], r[1], r[5], r[7]) for r in rows])
