"""Field queries without a GPU (include/psgsdf_query.h, DESIGN.md 22 "Field queries"): the yardstick tests/_query_ref.py against closed-form geometry
-- the analytic plane, on which both models are exact; a sphere of radius 10 voxels, where the cell model is off by at most |e|^2 / (2 rho) and the
trilinear cell by 3/8 / rho; the floor-and-wall volume of test_occlusion_cpu for the rays' t_min / t_max; the welded mesh, whose vertices are zeros of
the trilinear cell -- every status byte in one mixed call; the header as C99, the exported symbols and struct sizes, the calls' returns without a
context, the refusals of `voxelPS --query-ply` and the new kernels' resources.

On the rays' ends: a ray whose analytic parameter is below t_min starts behind the wall, inside the solid: within the observed shell it is buried,
beyond it nothing is observed and it misses.  So "a hit iff the analytic parameter lies in (t_min, t_max]" is asserted of status 0, the hits that are
not buried, and the rays below t_min must be buried or miss."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _mesh_ref as mref
import _occlusion_ref as oref
import _query_ref as qref
from test_mesh_components_cpu import EXE, HIPCC, ROOT, pieces_volume
from test_occlusion_cpu import NEAR, VS, VS32, X0, Z0, corner_samples, corner_volume, plane

f32 = np.float32
R_SPHERE, C_SPHERE = 10.0, np.array([15.3, 16.1, 15.7])      # voxels
BOUND = 0.0625                                              # voxels: both models against the sphere (3/8 / rho and 0.75 / (2 rho) at rho >= 6)
TOL = 1e-3                                                  # voxels: the projection's tolerance
RAY_CASES = [(0.0, 8.0), (0.25, 8.0), (2.0, 6.0), (1.0, 16.0)]      # (t_min, t_max) in voxels, on the corner volume (the sphere rays run without a t_max)


@functools.lru_cache(maxsize=None)
def sphere_volume(N=32):
    """a sphere of radius 10 voxels about (15.3, 16.1, 15.7) voxels, positions X = vs x index: dist = (rho - r) vs, the unit radial gradient, weight 1
    within 3 voxels of the surface, a smooth albedo.  Returns (v, dim)."""
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    x = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) - C_SPHERE
    rho = np.linalg.norm(x, axis=1)
    d = (rho - R_SPHERE) * VS
    grad = (x / rho[:, None]).T.astype(f32)
    rgb = (0.5 + 0.4 * np.sin(0.3 * x + np.array([0.0, 1.0, 2.0]))).T.astype(f32)
    return dict(dist=d.astype(f32), grad=np.ascontiguousarray(grad), weight=(np.abs(rho - R_SPHERE) < 3).astype(f32), rgb=np.ascontiguousarray(rgb)), (N, N, N)


@functools.lru_cache(maxsize=None)
def sphere_points(n=4000):
    """points on random radials, offset uniformly in +-2 voxels from the sphere: q [n, 3] float32 (mesh units), the offsets [n] in voxels"""
    rng = np.random.default_rng(3)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    off = rng.uniform(-2.0, 2.0, size=n)
    return ((C_SPHERE + (R_SPHERE + off)[:, None] * u) * VS).astype(f32), off


def sphere_offset(xyz):
    """|x - c| - r of float32 positions as the engine reads them, in voxels"""
    return np.linalg.norm(np.asarray(xyz, f32).astype(np.float64) / VS32 - C_SPHERE, axis=1) - R_SPHERE


@functools.lru_cache(maxsize=None)
def sphere_rays(n=3000):
    """rays from 14 to 15 voxels off the centre, aimed at c + 0.35 r x normal deviates: origins, directions [n, 3] float32"""
    rng = np.random.default_rng(7)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    o = C_SPHERE + rng.uniform(14.0, 15.0, size=n)[:, None] * u
    target = C_SPHERE + 0.35 * R_SPHERE * rng.normal(size=(n, 3))
    return (o * VS).astype(f32), ((target - o) * VS).astype(f32)


def sphere_ray_analytic(o32, w32):
    """of float32 rays: hit [n], the parameter t [n] in mesh units (inf: a miss), the incidence cosine [n]"""
    o = o32.astype(np.float64) / VS32 - C_SPHERE; w = w32.astype(np.float64); w /= np.linalg.norm(w, axis=1)[:, None]      # in voxels, as the engine places them
    r = R_SPHERE
    b = (o * w).sum(1); disc = b * b - ((o * o).sum(1) - r * r)
    hit = (disc > 0) & (b < 0)
    t = np.where(hit, -b - np.sqrt(np.where(hit, disc, 0.0)), np.inf)
    x = o + np.where(hit, t, 0.0)[:, None] * w
    cos = np.where(hit, -(x * w).sum(1) / r, 0.0)
    return hit, t * VS32, cos


def check_sphere_points(got, model, tag):
    q, off = sphere_points()
    ok = got["status"] == qref.OK
    err = np.abs(got["dist"].astype(np.float64) / VS32 - sphere_offset(q))[ok]
    radial = q.astype(np.float64) / VS32 - C_SPHERE; radial /= np.linalg.norm(radial, axis=1)[:, None]
    cosn = (got["normal"].astype(np.float64) * radial).sum(1)[ok]
    print(f"{tag} sphere points, model {model}: {int(ok.sum())} of {len(q)} valid (prototype: 4000 cell, 3932 trilinear), max |phi - exact| {err.max():.4f} voxel (bound {BOUND}; "
          f"prototype 0.035 cell, 0.031 trilinear), min normal . radial {cosn.min():.4f}")
    assert set(np.unique(got["status"]).tolist()) <= {qref.OK, qref.UNOBSERVED}
    if qref.MODELS[model] == qref.CELL:
        assert ok.all()                                     # |offset| <= 2 and half a cell diagonal: always inside the observed shell of 3 voxels
    else:
        assert ok[np.abs(off) < 3 - np.sqrt(3)].all() and ok.sum() >= 0.6 * len(q)      # every corner is within sqrt(3) voxels of the point
    assert err.max() <= BOUND
    assert cosn.min() > 0.99                                # the normal: radial to within a cell's turn of it (0.87 / 6 rad at the worst)
    assert (got["voxel"][ok] >= 0).all() and got["counts"]["n_ok"] == int(ok.sum()) and got["counts"]["n"] == len(q)


def check_sphere_projection(got, model, tag):
    q, off = sphere_points()
    st = got["status"]
    conv = st == qref.OK
    end = np.abs(sphere_offset(got["xyz"]))
    print(f"{tag} sphere projection, model {model}: {int(conv.sum())} converged, {int((st == qref.NOT_CONVERGED).sum())} not, "
          f"{int(((st == 1) | (st == 2)).sum())} left; iterations up to {int(got['iterations'][conv].max())}; converged points within {end[conv].max():.4f} voxel of the sphere")
    assert end[conv].max() <= BOUND + TOL
    assert (np.abs(got["residual"][conv]) <= f32(TOL * VS32)).all()      # (rounding to float32 is monotonic)
    if qref.MODELS[model] == qref.TRILINEAR:
        return conv
    assert (st == qref.NOT_CONVERGED).sum() <= 0.01 * len(q)
    return conv


def check_sphere_rays(got, tag):
    o, w = sphere_rays()
    hit, t, cos = sphere_ray_analytic(o, w)
    found = got["status"] != qref.MISS
    steep = hit & found & (cos >= 0.5)
    err = np.abs(got["t"].astype(np.float64) - t)[steep] / VS32
    print(f"{tag} sphere rays: {int(hit.sum())} analytic hits, {int((~hit).sum())} misses (prototype 2967 / 33), {int((hit != found).sum())} wrong; {int(steep.sum())} with cosine >= 0.5 "
          f"(prototype 2901), max |t - analytic| {err.max():.4f} voxel (bound 0.125, prototype 0.053)")
    assert (got["status"] <= qref.MISS).all() and got["counts"]["n_valid"] == len(o) and got["counts"]["n_buried"] == 0
    assert not (hit != found).any()
    assert err.max() <= 0.125
    assert got["counts"]["n_hits"] == int(hit.sum())
    return float(err.max())


def corner_rays(bias=1.0, K=16):
    """the rays of test_occlusion_cpu's samples (K directions each, about the floor's normal): origins, directions [141 K, 3] float32 and each ray's
    analytic parameter to the wall's plane in mesh units (inf: it runs away from the wall)"""
    q, _ = corner_samples()
    D = oref.dirs(K)
    o = np.repeat(q.astype(np.float64) + np.array([0, 0, bias * VS32]), K, 0).astype(f32)
    w = np.tile(D, (len(q), 1)).astype(f32)
    wn = w.astype(np.float64); wn /= np.sqrt((wn[:, 0] * wn[:, 0] + wn[:, 1] * wn[:, 1]) + wn[:, 2] * wn[:, 2])[:, None]
    ox = o[:, 0].astype(np.float64) - X0 * VS32
    with np.errstate(divide="ignore"):
        t = np.where(wn[:, 0] < 0, ox / -wn[:, 0], np.inf)
    return o, w, t


def check_corner_rays(cast, tag):
    """cast(origins, directions, t_min, t_max) -> the call's dict"""
    o, w, t = corner_rays()
    for t_min, t_max in RAY_CASES:
        got = cast(o, w, t_min * VS32, t_max * VS32)
        tf = np.where(np.isfinite(t), t, 1e9)
        near = (np.abs(tf - t_min * VS32) <= NEAR * VS32) | (np.abs(tf - t_max * VS32) <= NEAR * VS32)
        clean = (t > t_min * VS32) & (t <= t_max * VS32)
        st = got["status"]
        err = np.abs(got["t"].astype(np.float64) - t)[clean & (st == qref.HIT)] / VS32
        print(f"{tag} corner rays t in ({t_min}, {t_max}] voxels: {int(clean.sum())} of {len(t)} analytic hits, {int((st == qref.HIT).sum())} found, {int((st == qref.BURIED).sum())} buried, "
              f"{int(near.sum())} within {NEAR} voxel of an end, hit parameter within {err.max():.2e} voxel")
        assert not near.any()
        assert np.array_equal(st == qref.HIT, clean)
        assert np.isin(st[t <= t_min * VS32], (qref.MISS, qref.BURIED)).all() and (st[t > t_max * VS32] == qref.MISS).all()
        assert err.max() < 1e-4                             # the model is exact on both planes (test_occlusion_cpu)
        assert (got["voxel"][st == qref.MISS] == -1).all() and not got["t"][st == qref.MISS].any()
    # started inside the floor: buried at t_min
    q, _ = corner_samples()
    o = (q.astype(np.float64) - np.array([0, 0, 1.0 * VS32])).astype(f32); w = np.tile(f32([0, 0, 2]), (len(q), 1))
    for t_min in (0.0, 0.3 * VS32):
        got = cast(o, w, t_min, np.inf)
        assert (got["status"] == qref.BURIED).all() and (got["t"] == f32(t_min)).all() and got["counts"]["n_buried"] == got["counts"]["n_hits"] == len(q)


def mixed_points():
    """every status on the corner volume (48^3): [n, 3] float32 and the status each must get under (cell, trilinear)"""
    s = VS32
    pts = [([25.0, 20.0, Z0 + 0.2], 0, 0),                  # on the floor
           ([np.nan, 20.0, 18.0], 3, 3), ([25.0, np.inf, 18.0], 3, 3), ([25.0, 20.0, -np.inf], 3, 3),
           ([-0.6, 20.0, 18.0], 1, 1), ([47.6, 20.0, 18.0], 1, 1), ([25.0, -0.6, 18.0], 1, 1), ([25.0, 47.6, 18.0], 1, 1), ([25.0, 20.0, -0.6], 1, 1), ([25.0, 20.0, 47.6], 1, 1),
           ([47.2, 20.0, Z0 + 0.2], 0, 1),                  # on the last plane: a cell of the cell model, no trilinear cell
           ([-0.3, 20.0, Z0 + 0.2], 2, 1),                  # (behind the wall, unobserved) the first cell's lower half
           ([30.0, 20.0, 30.0], 2, 2)]                      # free space, unobserved
    return (np.array([p for p, _, _ in pts]) * s).astype(f32), np.array([[a, b] for _, a, b in pts], np.uint8)


def check_mixed(got, model):
    pts, want = mixed_points()
    k = qref.MODELS[model]
    st = got["status"]
    assert np.array_equal(st, want[:, k]), (model, st, want[:, k])
    assert set(st.tolist()) == ({0, 1, 2, 3})
    bad = st != 0
    for key in ("dist", "normal", "rgb", "weight"):
        if key in got:
            assert not got[key][bad].any(), key
    keeps = (st == 0) | ((st == 2) & (k == qref.CELL))
    assert (got["voxel"][keeps] >= 0).all() and (got["voxel"][~keeps] == -1).all()


# ---- the yardstick against closed form
def plane_points(n_pts=300):
    """random points within 2 voxels of the plane n.x = offset, in the mesh's units (mesh = world - origin: test_occlusion_cpu.plane_samples): q
    [n, 3] float32 and their heights over the plane [n] in voxels"""
    _, dim, n = plane()
    rng = np.random.default_rng(5)
    e1 = np.cross(n, [0, 0, 1.0]); e1 /= np.linalg.norm(e1); e2 = np.cross(n, e1)
    ab = rng.uniform(-8 * VS, 8 * VS, size=(n_pts, 2)); h = rng.uniform(-2.0, 2.0, size=n_pts)
    world = (0.004 + h * VS)[:, None] * n + ab[:, :1] * e1 + ab[:, 1:] * e2
    return (world + 0.5 * VS * np.asarray(dim)).astype(f32), h


def check_plane(got, model, tag):
    """both models are exact on the plane: what is left is the float32 rounding of dist and grad at up to 3.9 voxels, 2^-24 x 3.9 = 2.3e-7 voxel"""
    _, dim, n = plane()
    q, h = plane_points()
    ok = got["status"] == qref.OK
    # the field the volume holds, at the voxel coordinates the engine gives the point (q / vs with its float32 vs)
    exact = ((q.astype(np.float64) / VS32 - 0.5 * np.asarray(dim)) * VS) @ n - 0.004
    err = np.abs(got["dist"].astype(np.float64) - exact)[ok] / VS
    nerr = np.abs(got["normal"].astype(np.float64) - n)[ok].max()
    print(f"{tag} plane, model {model}: {int(ok.sum())} of {len(q)} valid, max |phi - (n.x - offset)| {err.max():.2e} voxel, normal within {nerr:.2e}")
    if qref.MODELS[model] == qref.CELL:
        assert ok.all()                                     # the cell's centre is within 2 + sqrt(3) / 2 < 3 voxels of the plane
    else:
        assert ok[np.abs(h) < 3 - np.sqrt(3)].all() and set(got["status"][~ok].tolist()) <= {qref.UNOBSERVED}
    assert err.max() <= 1e-6 and nerr <= 1e-6


@pytest.mark.parametrize("model", ["cell", "trilinear"])
def test_plane_both_models_are_exact(model):
    v, dim, _ = plane()
    check_plane(qref.query_points(v, dim, VS, plane_points()[0], model), model, "yardstick")


@pytest.mark.parametrize("model", ["cell", "trilinear"])
def test_sphere_points_and_projection(model):
    v, dim = sphere_volume()
    q, off = sphere_points()
    got = qref.query_points(v, dim, VS, q, model)
    check_sphere_points(got, model, "yardstick")
    pr = qref.project_points(v, dim, VS, q, model, TOL * VS32, 16)
    conv = check_sphere_projection(pr, model, "yardstick")
    started = got["status"] == qref.OK
    if model == "trilinear":
        assert np.array_equal(conv, started)                # every point that starts valid converges
        assert pr["iterations"][conv].max() <= 4
        far = conv & (np.abs(off) > BOUND)
        assert np.array_equal(np.sign(pr["distance"][far]), np.sign(off[far]))
    assert not pr["distance"][~started].any() and not pr["iterations"][~started].any()
    assert np.array_equal(pr["xyz"][~started], q[~started])


def test_sphere_and_corner_rays():
    v, dim = sphere_volume()
    o, w = sphere_rays()
    got = qref.cast_rays(v, dim, VS, o, w)
    dev = check_sphere_rays(got, "yardstick")
    print(f"yardstick's own maximum deviation from closed form on the steep sphere rays: {dev:.6f} voxel")
    cv, cdim = corner_volume()
    check_corner_rays(lambda o, w, a, b: qref.cast_rays(cv, cdim, VS, o, w, a, b), "yardstick")


def test_mesh_vertices_are_zeros_of_the_trilinear_cell():
    v, dim, vs = pieces_volume(torus=True)
    xyz = mref.mesh(v, dim, vs)[0]
    assert len(xyz) == 4280
    for model in ("cell", "trilinear"):
        got = qref.query_points(v, dim, vs, xyz, model)
        worst = np.abs(got["dist"]).max() / vs
        print(f"welded mesh, model {model}: {got['counts']['n_ok']} of {len(xyz)} vertices valid, max |phi| {worst:.2e} voxel (prototype, trilinear: 3.2e-6)")
        assert (got["status"] == qref.OK).all()
        if model == "trilinear":
            assert worst <= 1e-5


@pytest.mark.parametrize("model", ["cell", "trilinear"])
def test_every_status_in_one_call(model):
    v, dim = corner_volume()
    pts, _ = mixed_points()
    got = qref.query_points(v, dim, VS, pts, model)
    check_mixed(got, model)
    assert got["counts"] == dict(n=len(pts), n_ok=int((got["status"] == 0).sum()), n_outside=int((got["status"] == 1).sum()), n_unobserved=int((got["status"] == 2).sum()), n_invalid=3)
    pr = qref.project_points(v, dim, VS, pts, model, TOL * VS32, 16)
    assert np.array_equal(pr["status"] != 0, got["status"] != 0) and (pr["status"][got["status"] != 0] == got["status"][got["status"] != 0]).all()
    moved = pr["iterations"] > 0
    assert np.array_equal(pr["xyz"][~moved].view(np.uint32), pts[~moved].view(np.uint32))      # a point that never moved keeps its bits, NaN included
    for bad in (("cell", -1.0, 16), ("cell", np.nan, 16), ("cell", 0.0, 0), ("cell", 0.0, 65), ("linear", 0.0, 16)):
        with pytest.raises(ValueError):
            qref.check_project_params(*bad)
    for bad in ((-1.0, 1.0), (np.nan, 1.0), (np.inf, np.inf), (1.0, 1.0), (2.0, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            qref.check_ray_params(*bad)


# ---- the interface
def test_library_exports_the_calls(built):
    import __graft_entry__ as g
    from psgradientsdf_amd import capi
    names = ["psgsdf_cast_rays", "psgsdf_project_points", "psgsdf_query_points"]
    assert g._declared_symbols("psgsdf_query.h") == names
    for path in (capi.ENGINE_LIB, capi.ENGINE_LIB_DEV):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, s) for s in names), path
    assert all(hasattr(capi.Api, s) for s in ("query_points", "project_points", "cast_rays"))
    assert tuple(ctypes.sizeof(s) for s in (capi.QueryCounts, capi.ProjectParams, capi.ProjectCounts, capi.RayParams, capi.RayCounts)) == (40, 24, 40, 16, 32)
    lib = ctypes.CDLL(capi.ENGINE_LIB)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    pts = lib.psgsdf_query_points; pts.argtypes = [P, P, I64, ctypes.c_int32] + [P] * 7
    prj = lib.psgsdf_project_points; prj.argtypes = [P, P, I64, P] + [P] * 8
    ray = lib.psgsdf_cast_rays; ray.argtypes = [P, P, P, I64, P] + [P] * 7
    x = (ctypes.c_float * 3)(0, 0, 1)
    ARG, STATE = -1, -4
    o6 = [ctypes.byref(P()) for _ in range(6)]; o7 = [ctypes.byref(P()) for _ in range(7)]
    qc, pc, rc = capi.QueryCounts(), capi.ProjectCounts(), capi.RayCounts()
    pp, rp = capi.ProjectParams(1, 16, 1e-5, 0.0), capi.RayParams(0.0, float("inf"))
    for k in range(7):                                   # a NULL output pointer, the counts among them
        outs = [None if i == k else r for i, r in enumerate(o6 + [ctypes.byref(qc)])]
        assert pts(None, x, 1, 0, *outs) == ARG
        outs = [None if i == k else r for i, r in enumerate(o6 + [ctypes.byref(rc)])]
        assert ray(None, x, x, 1, ctypes.byref(rp), *outs) == ARG
    for k in range(8):
        outs = [None if i == k else r for i, r in enumerate(o7 + [ctypes.byref(pc)])]
        assert prj(None, x, 1, ctypes.byref(pp), *outs) == ARG
    q_out, p_out, r_out = o6 + [ctypes.byref(qc)], o7 + [ctypes.byref(pc)], o6 + [ctypes.byref(rc)]
    assert pts(None, None, 1, 0, *q_out) == ARG and pts(None, x, -1, 0, *q_out) == ARG and pts(None, x, 1, 2, *q_out) == ARG and pts(None, x, 1, -1, *q_out) == ARG
    assert prj(None, None, 1, ctypes.byref(pp), *p_out) == ARG and prj(None, x, -1, ctypes.byref(pp), *p_out) == ARG and prj(None, x, 1, None, *p_out) == ARG
    for bad in (capi.ProjectParams(2, 16, 1e-5, 0.0), capi.ProjectParams(-1, 16, 1e-5, 0.0), capi.ProjectParams(1, 0, 1e-5, 0.0), capi.ProjectParams(1, 65, 1e-5, 0.0),
                capi.ProjectParams(1, 16, -1e-5, 0.0), capi.ProjectParams(1, 16, float("nan"), 0.0), capi.ProjectParams(1, 16, float("inf"), 0.0), capi.ProjectParams(1, 16, 1e-5, 1.0),
                capi.ProjectParams(1, 16, 1e-5, float("nan"))):
        assert prj(None, x, 1, ctypes.byref(bad), *p_out) == ARG, (bad.model, bad.max_iters, bad.tol, bad.reserved)
    assert ray(None, None, x, 1, ctypes.byref(rp), *r_out) == ARG and ray(None, x, None, 1, ctypes.byref(rp), *r_out) == ARG
    assert ray(None, x, x, -1, ctypes.byref(rp), *r_out) == ARG and ray(None, x, x, 1, None, *r_out) == ARG
    for bad in (capi.RayParams(-1.0, 1.0), capi.RayParams(float("nan"), 1.0), capi.RayParams(float("inf"), float("inf")), capi.RayParams(1.0, 1.0), capi.RayParams(2.0, 1.0),
                capi.RayParams(0.0, float("nan"))):
        assert ray(None, x, x, 1, ctypes.byref(bad), *r_out) == ARG, (bad.t_min, bad.t_max)
    # everything in order but the context: PSGSDF_ERR_STATE, nothing touched
    for model in (0, 1):
        assert pts(None, x, 1, model, *q_out) == STATE and pts(None, None, 0, model, *q_out) == STATE
        assert prj(None, x, 1, ctypes.byref(capi.ProjectParams(model, 64, 0.0, 0.0)), *p_out) == STATE and prj(None, None, 0, ctypes.byref(pp), *p_out) == STATE
    assert ray(None, x, x, 1, ctypes.byref(rp), *r_out) == STATE and ray(None, None, None, 0, ctypes.byref(capi.RayParams(1.0, 2.0)), *r_out) == STATE
    assert (qc.n, pc.n, rc.n) == (0, 0, 0)


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "use_query.c"
    src.write_text('#include "psgsdf_query.h"\n'
                   'typedef char a_size[sizeof(psgsdf_query_counts) == 40 ? 1 : -1];\ntypedef char b_size[sizeof(psgsdf_project_params) == 24 ? 1 : -1];\n'
                   'typedef char c_size[sizeof(psgsdf_project_counts) == 40 ? 1 : -1];\ntypedef char d_size[sizeof(psgsdf_ray_params) == 16 ? 1 : -1];\n'
                   'typedef char e_size[sizeof(psgsdf_ray_counts) == 32 ? 1 : -1];\n'
                   'int use(psgsdf_ctx* c, const float* x, const float* w) {\n    psgsdf_query_counts qc; psgsdf_project_params pp; psgsdf_project_counts pc; psgsdf_ray_params rp; psgsdf_ray_counts rc;\n'
                   '    const uint8_t *st, *it; const float *d, *n, *col, *wt, *t, *y; const int64_t* v; int rc_;\n'
                   '    pp.model = PSGSDF_Q_TRILINEAR; pp.max_iters = 16; pp.tol = 1e-5; pp.reserved = 0; rp.t_min = 0; rp.t_max = 1;\n'
                   '    rc_ = psgsdf_query_points(c, x, 1, PSGSDF_Q_CELL, &st, &d, &n, &col, &wt, &v, &qc);\n'
                   '    if (!rc_) rc_ = psgsdf_project_points(c, x, 1, &pp, &st, &y, &d, &n, &v, &it, &t, &pc);\n'
                   '    if (!rc_) rc_ = psgsdf_cast_rays(c, x, w, 1, &rp, &st, &t, &y, &n, &col, &v, &rc);\n'
                   '    return rc_ ? rc_ : (int)(qc.n_ok + pc.n_converged + rc.n_hits + (st[0] == PSGSDF_RAY_BURIED) + (it[0] == PSGSDF_Q_NOT_CONVERGED));\n}\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_query.o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(not os.path.exists(EXE), reason="voxelPS not built")
def test_voxelps_refuses_query_flags_without_a_file_on_several_gpus_and_a_bad_model(tmp_path):
    cfg = ["--config_file", str(tmp_path / "none.json")]
    for extra, words in ((["--query-model", "cell"], ("--query-model", "--query-ply")), (["--query-project"], ("--query-project", "--query-ply")),
                         (["--query-ply", "x.ply", "--query-model", "cubic"], ("--query-model", "cell", "trilinear")),
                         (["--query-ply", "x.ply", "--gpus", "2"], ("--query-ply", "--gpus"))):
        r = subprocess.run([EXE] + cfg + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (extra, r.stdout + r.stderr)
        assert "load the config file" not in r.stdout      # refused while parsing: no rank was started, no configuration read


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_query_kernels_use_no_scratch_and_the_other_walkers_keep_their_registers(tmp_path):
    from test_occlusion_cpu import test_occlusion_kernels_use_no_scratch_and_the_other_walkers_keep_their_registers as pins
    from test_kernel_resources import resources
    ks = {k: v for k, v in resources("query.hip", tmp_path).items() if "k_query_" in k}
    print(ks)
    assert len(ks) == 5 and all(v["scratch"] == 0 and v["vgpr"] <= 128 for v in ks.values()), ks      # two models x points and projection, and the rays: 4 waves per SIMD
    src = open(os.path.join(ROOT, "psgradientsdf_amd", "csrc", "query.hip")).read()
    assert src.count("__shared__") == 0 and src.count("__syncthreads") == 0
    pins(tmp_path)      # render_trace.h is untouched: k_occlusion, k_render, k_render_report and k_bake are the kernels they were
