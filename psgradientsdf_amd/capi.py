"""ctypes binding of the C ABI declared in include/psgsdf.h.

This is host-side plumbing for tests and bench.py (the reference is C++; the C++ mirror of its
PsOptimizer/LedOptimizer interface lives in psgradientsdf_amd/host/).  `Api` is generic over
(shared library, symbol prefix) so that a test harness can bind another implementation of the
same C ABI; the product only ever instantiates it through `load_engine()`, which binds
`libpsgsdf.so` and raises if the HIP library is missing — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ALBEDO, LIGHT, DIST, POSE, ALL = 1, 2, 4, 8, 15
SH1, SH2, LED = 0, 1, 2
L2, CAUCHY, HUBER, TUKEY, TRUNC_L2 = 0, 1, 2, 3, 4
# output planes of Api.render (include/psgsdf_render.h), in bit order, with their channel counts
R_DEPTH, R_NORMAL, R_ALBEDO, R_SHADING, R_RENDERED, R_RESIDUAL, R_VOXEL = 1, 2, 4, 8, 16, 32, 64
R_ALL = 127
_R_PLANES = [("depth", R_DEPTH, 1), ("normal", R_NORMAL, 3), ("albedo", R_ALBEDO, 3), ("shading", R_SHADING, 1),
             ("rendered", R_RENDERED, 3), ("residual", R_RESIDUAL, 3), ("voxel", R_VOXEL, 1)]

_HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_LIB = os.environ.get("PSGSDF_ENGINE_LIB") or os.path.join(_HERE, "csrc", "libpsgsdf.so")      # (the override is for A/B runs of two BUILDS on one box: tools/)
# the development build (-DPSGSDF_DEV): the same engine plus the fault-injection / ablation knobs the product library does not contain; tests and tools only
ENGINE_LIB_DEV = os.path.join(_HERE, "csrc", "libpsgsdf_dev.so")


class GridDesc(C.Structure):
    _fields_ = [("dim", C.c_int32 * 3), ("voxel_size", C.c_float), ("shift", C.c_float * 3), ("truncation", C.c_float)]


class Settings(C.Structure):
    _fields_ = [("model", C.c_int32), ("loss", C.c_int32), ("lambda_", C.c_float), ("damping", C.c_float),
                ("reg_weight_rho", C.c_float), ("reg_weight_n", C.c_float), ("reg_weight_l", C.c_float),
                ("max_it", C.c_int32), ("conv_threshold", C.c_float), ("upsample", C.c_int32),
                ("ref_quirks", C.c_int32), ("cg_max_it", C.c_int32)]


class StepStats(C.Structure):
    _fields_ = [("block", C.c_int32), ("cg_iters", C.c_int32), ("cg_converged", C.c_int32), ("applied", C.c_int32),
                ("e_in", C.c_double), ("cg_error", C.c_double), ("n_accepted", C.c_int64), ("n_obs", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IterStats(C.Structure):
    _fields_ = [("e_after", C.c_double * 4), ("e_n", C.c_double), ("e_l", C.c_double), ("e_total", C.c_double),
                ("rel_diff", C.c_double), ("reg_weight_n", C.c_float), ("reg_weight_l", C.c_float),
                ("cg_iters", C.c_int32), ("converged", C.c_int32), ("diverged", C.c_int32), ("upsampled", C.c_int32),
                ("e_r", C.c_double), ("e_n_in", C.c_double), ("e_l_in", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["e_after"] = list(self.e_after)
        return d

    def __getitem__(self, k):      # (a record reads like its dict: the passive observer hands out struct copies, not dicts -- it runs between two launches)
        v = getattr(self, k)
        return list(v) if k == "e_after" else v


class Info(C.Structure):
    _fields_ = [("dim", C.c_int32 * 3), ("voxel_size", C.c_float), ("origin", C.c_float * 3), ("n_frames", C.c_int32),
                ("n_band", C.c_int32), ("light_stride", C.c_int32), ("vis_words", C.c_int32),
                ("reg_weight_n", C.c_float), ("reg_weight_l", C.c_float)]


class View(C.Structure):
    _fields_ = [("frame", C.c_int32), ("pose", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("light_frame", C.c_int32)]


class MeshFilter(C.Structure):      # psgsdf_mesh_filter (include/psgsdf_mesh.h)
    _fields_ = [("min_faces", C.c_int64), ("min_area", C.c_double), ("keep_largest", C.c_int32)]


class Bake(C.Structure):      # psgsdf_bake (include/psgsdf_bake.h)
    _fields_ = [("xyz", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("rgb", C.POINTER(C.c_uint8)), ("faces", C.POINTER(C.c_int32)), ("vertex_map", C.POINTER(C.c_int32)),
                ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("n_vertices_in", C.c_int64), ("n_faces_in", C.c_int64),
                ("uv", C.POINTER(C.c_float)), ("width", C.c_int32), ("height", C.c_int32),
                ("albedo", C.POINTER(C.c_uint8)), ("normal", C.POINTER(C.c_float)), ("displacement", C.POINTER(C.c_float)), ("voxel", C.POINTER(C.c_int32)), ("face", C.POINTER(C.c_int32)),
                ("n_texels", C.c_int64), ("n_hits", C.c_int64), ("n_hits_off_band", C.c_int64), ("n_buried", C.c_int64), ("n_misses", C.c_int64)]


class AoParams(C.Structure):      # psgsdf_ao_params (include/psgsdf_occlusion.h)
    _fields_ = [("n_dirs", C.c_int32), ("reserved", C.c_int32), ("radius", C.c_double), ("bias", C.c_double)]


class AoCounts(C.Structure):      # psgsdf_ao_counts
    _fields_ = [("n_samples", C.c_int64), ("n_valid", C.c_int64), ("n_rays", C.c_int64), ("n_occluded", C.c_int64), ("n_buried", C.c_int64)]


class BakeAo(C.Structure):      # psgsdf_bake_ao
    _fields_ = [("bake", Bake), ("occlusion", C.POINTER(C.c_uint8)), ("mask", C.POINTER(C.c_uint64)), ("dirs", C.POINTER(C.c_double)),
                ("n_dirs", C.c_int32), ("reserved", C.c_int32), ("counts", AoCounts)]


class QueryCounts(C.Structure):      # psgsdf_query_counts (include/psgsdf_query.h)
    _fields_ = [(k, C.c_int64) for k in ("n", "n_ok", "n_outside", "n_unobserved", "n_invalid")]


class ProjectParams(C.Structure):      # psgsdf_project_params
    _fields_ = [("model", C.c_int32), ("max_iters", C.c_int32), ("tol", C.c_double), ("reserved", C.c_double)]


class ProjectCounts(C.Structure):      # psgsdf_project_counts
    _fields_ = [(k, C.c_int64) for k in ("n", "n_converged", "n_left", "n_not_converged", "n_invalid")]


class RayParams(C.Structure):      # psgsdf_ray_params
    _fields_ = [("t_min", C.c_double), ("t_max", C.c_double)]


class RayCounts(C.Structure):      # psgsdf_ray_counts
    _fields_ = [(k, C.c_int64) for k in ("n", "n_valid", "n_hits", "n_buried")]


QUERY_MODELS = {"cell": 0, "trilinear": 1}
Q_OK, Q_OUTSIDE, Q_UNOBSERVED, Q_INVALID, Q_NOT_CONVERGED = 0, 1, 2, 3, 4
RAY_HIT, RAY_MISS, RAY_BURIED, RAY_INVALID = 0, 1, 2, 3


class BakeCurvature(C.Structure):      # psgsdf_bake_curvature (include/psgsdf_curvature.h)
    _fields_ = [("bake", Bake), ("mean", C.POINTER(C.c_float)), ("valid", C.POINTER(C.c_uint8)), ("n_valid", C.c_int64)]


class PhotoParams(C.Structure):      # psgsdf_photo_params (include/psgsdf_photo.h)
    _fields_ = [("bias", C.c_double), ("cos_min", C.c_double), ("shade_min", C.c_double), ("want_status", C.c_int32), ("reserved", C.c_int32)]


class PhotoCounts(C.Structure):      # psgsdf_photo_counts
    _fields_ = [(k, C.c_int64) for k in ("n_samples", "n_pairs", "n_used", "n_outside", "n_grazing", "n_occluded", "n_buried", "n_dark", "n_texels_solved")]


class BakePhoto(C.Structure):      # psgsdf_bake_photo
    _fields_ = [("bake", Bake), ("photo", C.POINTER(C.c_float)), ("photo_rgb", C.POINTER(C.c_uint8)), ("n_obs", C.POINTER(C.c_int32)), ("status", C.POINTER(C.c_uint8)),
                ("n_frames", C.c_int32), ("reserved", C.c_int32), ("counts", PhotoCounts)]


PHOTO_USED, PHOTO_OUTSIDE, PHOTO_GRAZING, PHOTO_OCCLUDED, PHOTO_DARK, PHOTO_NO_SAMPLE = 0, 1, 2, 3, 4, 255


class Light(C.Structure):      # psgsdf_light (include/psgsdf_relight.h)
    _fields_ = [("kind", C.c_int32), ("n_sh", C.c_int32), ("sh", C.c_float * 9), ("vec", C.c_float * 3), ("colour", C.c_float * 3), ("ambient", C.c_float * 3),
                ("spread", C.c_float), ("n_shadow", C.c_int32)]


class RelightParams(C.Structure):      # psgsdf_relight_params
    _fields_ = [("bias", C.c_double), ("reach", C.c_double), ("n_lights", C.c_int32), ("reserved", C.c_int32)]


class RelightCounts(C.Structure):      # psgsdf_relight_counts
    _fields_ = [("n_hits", C.c_int64), ("n_lit", C.c_int64), ("n_rays", C.c_int64), ("n_occluded", C.c_int64), ("n_buried", C.c_int64)]


LIGHT_KINDS = {"sh": 0, "directional": 1, "point": 2}


def make_light(d):
    """a psgsdf_light of a dict: kind ("sh", "directional", "point"), sh (4 or 9 coefficients), vec, colour (default 1, 1, 1), ambient (default 0),
    spread (default 0), samples (the shadow rays K; default 1, an SH light has none)"""
    L = Light()
    kind = d["kind"]
    L.kind = LIGHT_KINDS[kind] if isinstance(kind, str) else int(kind)
    if L.kind == 0:
        sh = [float(x) for x in np.asarray(d["sh"], np.float32).reshape(-1)]
        if len(sh) > 9:
            raise ValueError("relight: an SH light has 4 or 9 coefficients")
        L.n_sh = len(sh)
        L.sh[:len(sh)] = sh
    else:
        L.vec[:] = [float(x) for x in np.asarray(d["vec"], np.float32).reshape(3)]
    L.colour[:] = [float(x) for x in np.broadcast_to(np.asarray(d.get("colour", 1.0), np.float32), (3,))]
    L.ambient[:] = [float(x) for x in np.broadcast_to(np.asarray(d.get("ambient", 0.0), np.float32), (3,))]
    L.spread = float(d.get("spread", 0.0))
    L.n_shadow = int(d.get("samples", 0 if L.kind == 0 else 1))
    return L


class CompareParams(C.Structure):      # psgsdf_compare_params (include/psgsdf_compare.h)
    _fields_ = [("max_dist", C.c_double), ("tau", C.c_double), ("grid_cell", C.c_double), ("reserved", C.c_int32 * 2)]


class CompareSide(C.Structure):      # psgsdf_compare_side
    _fields_ = [("n", C.c_int64), ("n_valid", C.c_int64), ("n_matched", C.c_int64), ("n_within_tau", C.c_int64),
                ("sum_d", C.c_int64), ("sum_d2", C.c_int64), ("sum_signed", C.c_int64), ("hist", C.c_int64 * 16),
                ("max", C.c_double), ("mean", C.c_double), ("rms", C.c_double), ("mean_signed", C.c_double)]


class Compare(C.Structure):      # psgsdf_compare
    _fields_ = [("xyz", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("rgb", C.POINTER(C.c_uint8)), ("faces", C.POINTER(C.c_int32)),
                ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
                ("vertex_dist", C.POINTER(C.c_float)), ("vertex_nearest", C.POINTER(C.c_int32)), ("vertex_side", C.POINTER(C.c_int8)),
                ("ref_dist", C.POINTER(C.c_float)), ("ref_nearest", C.POINTER(C.c_int32)), ("ref_side", C.POINTER(C.c_int8)),
                ("to_reference", CompareSide), ("to_reconstruction", CompareSide),
                ("precision", C.c_double), ("recall", C.c_double), ("fscore", C.c_double)]


class AlignParams(C.Structure):      # psgsdf_align_params (include/psgsdf_align.h)
    _fields_ = [("init", C.c_double * 16), ("max_dist", C.c_double), ("min_dist", C.c_double), ("shrink", C.c_double), ("eps_rot", C.c_double), ("eps_trans", C.c_double),
                ("grid_cell", C.c_double), ("directions", C.c_int32), ("max_iters", C.c_int32), ("reserved", C.c_int32 * 2)]


class AlignIter(C.Structure):      # psgsdf_align_iter
    _fields_ = [("radius", C.c_double), ("rms", C.c_double), ("n_pairs", C.c_int64 * 2), ("min_pivot", C.c_double), ("step", C.c_double * 6)]

    def as_dict(self):
        return dict(radius=self.radius, rms=self.rms, n_pairs=[int(self.n_pairs[0]), int(self.n_pairs[1])], min_pivot=self.min_pivot, step=np.array(self.step, np.float64))


ALIGN_CONVERGED, ALIGN_MAX_ITERS, ALIGN_DEGENERATE, ALIGN_TOO_FEW = 0, 1, 2, 3


class Align(C.Structure):      # psgsdf_align
    _fields_ = [("transform", C.c_double * 16), ("centre", C.c_double * 3), ("status", C.c_int32), ("n_iters", C.c_int32), ("iters", AlignIter * 64), ("system0", C.c_double * 28),
                ("final", AlignIter), ("aligned_xyz", C.POINTER(C.c_float)), ("n_ref", C.c_int64),
                ("xyz", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("rgb", C.POINTER(C.c_uint8)), ("faces", C.POINTER(C.c_int32)), ("n_vertices", C.c_int64), ("n_faces", C.c_int64)]


# psgsdf_mesh_component (include/psgsdf_mesh.h), 88 bytes
MESH_COMPONENT_DTYPE = np.dtype([("first_vertex", "<i8"), ("n_vertices", "<i8"), ("n_faces", "<i8"), ("n_edges", "<i8"), ("n_boundary_edges", "<i8"),
                                 ("n_nonmanifold_edges", "<i8"), ("area", "<f8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("kept", "<i4"), ("reserved", "<i4")])


class RenderStats(C.Structure):
    _fields_ = [("n_pixels", C.c_int64), ("n_hits", C.c_int64), ("n_hits_off_band", C.c_int64),
                ("sum_r2", C.c_double * 3), ("sum_abs_r", C.c_double * 3), ("robust", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["sum_r2"], d["sum_abs_r"] = list(self.sum_r2), list(self.sum_abs_r)
        return d


def default_settings(model=SH1, **kw):
    """config_skorates.json values (cauchy, lambda 0.2, damping 1, reg_n 10, reg_l 0, conv 5e-3)."""
    s = Settings(model=model, loss=CAUCHY, lambda_=0.2, damping=1.0, reg_weight_rho=0.0, reg_weight_n=10.0,
                 reg_weight_l=0.0, max_it=100, conv_threshold=5e-3, upsample=0, ref_quirks=1, cg_max_it=0)
    for k, v in kw.items():
        if k == "lambda":
            k = "lambda_"
        setattr(s, k, v)
    return s


def _fp(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


_F32P, _U8P, _I32P = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
_ITER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(IterStats))      # psgsdf_iter_cb


def _ref(s):
    return None if s is None else C.byref(s)


def _owned(ptr, shape, dtype):
    """The engine's result behind `ptr` as an array the caller owns: the engine's results are valid until the next extraction call, so every one of
    them is copied here.  A shape without elements gives zeros(shape, dtype) and the pointer (NULL, then) is never touched."""
    shape = tuple(int(n) for n in shape)
    if 0 in shape:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ptr, shape=shape).copy()


def _mesh_filter(min_faces, min_area, keep_largest, always=False):
    """the psgsdf_mesh_filter of the three keyword arguments, or None (the engine's NULL: the whole mesh) when all three are zero"""
    if not (always or min_faces or min_area or keep_largest):
        return None
    return MeshFilter(int(min_faces), float(min_area), int(keep_largest))


def _counts(c):
    """a counts struct (AoCounts, PhotoCounts, RelightCounts) as a dict of ints"""
    return {k: int(getattr(c, k)) for k, _ in c._fields_}


def _mesh_arrays(r):
    """xyz, normals, rgb, faces of a result that holds the welded mesh (Bake, Compare, Align, _MeshHead)"""
    V, F = r.n_vertices, r.n_faces
    return dict(xyz=_owned(r.xyz, (V, 3), np.float32), normals=_owned(r.normals, (V, 3), np.float32), rgb=_owned(r.rgb, (V, 3), np.uint8), faces=_owned(r.faces, (F, 3), np.int32))


class _MeshHead:
    """the six out-parameters every welded-mesh call begins with"""

    def __init__(self):
        self.xyz, self.normals, self.rgb, self.faces, self._nv, self._nf = _F32P(), _F32P(), _U8P(), _I32P(), C.c_int64(), C.c_int64()

    n_vertices = property(lambda self: self._nv.value)
    n_faces = property(lambda self: self._nf.value)

    def refs(self):
        """in the ABI's order"""
        return [C.byref(x) for x in (self.xyz, self.normals, self.rgb, self._nv, self.faces, self._nf)]

    def arrays(self):
        return _mesh_arrays(self)


def _reference(ref_xyz, ref_faces):
    """(points [n, 3] float32, faces [f, 3] int32 or None, the four arguments points, n, faces, f of a psgsdf_*_reference call)"""
    xyz = np.ascontiguousarray(ref_xyz, np.float32).reshape(-1, 3)
    faces = None if ref_faces is None else np.ascontiguousarray(ref_faces, np.int32).reshape(-1, 3)
    nf = 0 if faces is None else len(faces)
    return xyz, faces, (xyz.ctypes.data_as(_F32P), C.c_int64(len(xyz)), faces.ctypes.data_as(_I32P) if nf else None, C.c_int64(nf))


class PsgsdfError(RuntimeError):
    pass


class Api:
    """One context behind the C ABI of include/psgsdf.h.  (The binding is generic over (library, symbol prefix): the test oracle exports the same
    entry points under another prefix and subclasses this in oracle/oracle.py; the product only instantiates it through load_engine.)"""

    def __init__(self, lib: C.CDLL, prefix: str, grid: GridDesc, K, settings: Settings, device: int = 0):
        self._lib, self._p = lib, prefix
        self.ctx = C.c_void_p()
        Karr, Kp = _fp(K)
        self._grid, self._settings = grid, settings
        self._check(self._fn("create")(C.byref(grid), Kp, C.byref(settings), C.c_int(device), C.byref(self.ctx)), "create")

    # -- plumbing
    def _fn(self, name):
        f = getattr(self._lib, self._p + name)
        f.restype = C.c_int
        return f

    def _check(self, rc, what):
        if rc != 0:
            msg = ""
            try:
                g = getattr(self._lib, self._p + "last_error")
                g.restype = C.c_char_p
                msg = (g(self.ctx) or b"").decode()
            except Exception:
                pass
            raise PsgsdfError(f"{self._p}{what} failed rc={rc} {msg}")

    def close(self):
        if self.ctx:
            d = getattr(self._lib, self._p + "destroy")
            d.restype = None
            d(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs
    def upload_volume(self, dist, grad, weight, rgb, vis, words):
        a = [_fp(dist), _fp(grad), _fp(weight), _fp(rgb), _fp(vis, np.uint64)]
        self._check(self._fn("upload_volume")(self.ctx, a[0][1], a[1][1], a[2][1], a[3][1], a[4][1], C.c_int(words)), "upload_volume")

    # -- slab-local upload (multi-rank): no rank touches the whole volume
    def slab_plane_count(self, dist_plane, vis_plane, words):
        a = [_fp(dist_plane), _fp(vis_plane, np.uint64)]; out = C.c_double()
        self._check(self._fn("slab_plane_count")(self.ctx, a[0][1], a[1][1], C.c_int(words), C.byref(out)), "slab_plane_count")
        return out.value

    def plan_slab(self, plane_counts):
        a = _fp(plane_counts, np.float64); z0, z1 = C.c_int(), C.c_int()
        self._check(self._fn("plan_slab")(self.ctx, a[1], C.byref(z0), C.byref(z1)), "plan_slab")
        return z0.value, z1.value

    def rebalance_slabs(self):
        """re-cut a slab-parallel fused volume into slabs of equal band-candidate count and move the planes (collective)"""
        self._check(self._fn("rebalance_slabs")(self.ctx), "rebalance_slabs")

    def upload_volume_slab(self, z0, z1, dist, grad, weight, rgb, vis, words):
        a = [_fp(dist), _fp(grad), _fp(weight), _fp(rgb), _fp(vis, np.uint64)]
        self._check(self._fn("upload_volume_slab")(self.ctx, C.c_int(z0), C.c_int(z1), a[0][1], a[1][1], a[2][1], a[3][1], a[4][1], C.c_int(words)), "upload_volume_slab")

    def load_scene_slab(self, sc, rank, n_ranks, planes=None, u8=None):
        """load_scene for a rank of a multi-rank run that only ever looks at ITS planes of the scene: `planes(zlo, zhi)` returns the dict of
        per-voxel arrays (dist, grad, weight, rgb, vis) of the z-planes [zlo, zhi) -- default: slices of the whole-volume arrays of `sc`
        (a scene generator or a file reader produces just those planes).  `sc` supplies the grid, the keyframes and the poses.
        The cut negotiation: rank r counts the band candidates of the r-th of n equal blocks of planes (any split is allowed)."""
        nx, ny, nz = (int(x) for x in sc.dim); plane = nx * ny
        if planes is None:
            def planes(zlo, zhi):
                sl = slice(zlo * plane, zhi * plane)
                return dict(dist=sc.dist[sl], grad=sc.grad[:, sl], weight=sc.weight[sl], rgb=sc.rgb[:, sl], vis=sc.vis[sl])
        cnt = np.zeros(nz)
        a, b = rank * nz // n_ranks, (rank + 1) * nz // n_ranks
        if b > a:
            p = planes(a, b)
            for k in range(a, b):
                sl = slice((k - a) * plane, (k - a + 1) * plane)
                cnt[k] = self.slab_plane_count(p["dist"][sl], p["vis"][sl], sc.vis_words)
        z0, z1 = self.plan_slab(cnt)
        zlo, zhi = max(0, z0 - 1), min(nz, z1 + 1)
        p = planes(zlo, zhi)
        self.upload_volume_slab(z0, z1, p["dist"], p["grad"], p["weight"], p["rgb"], p["vis"], sc.vis_words)
        self._scene_keyframes(sc, u8)
        self.init()
        return z0, z1

    def _scene_keyframes(self, sc, u8, require=False):
        """a scene's keyframes, as 8-bit RGB if u8 (None: whenever the scene has them); require: asking for 8-bit images the scene has not is a ValueError"""
        has_u8 = getattr(sc, "images_u8", None) is not None
        if u8 is None:
            u8 = has_u8
        if u8:
            if require and not has_u8:
                raise ValueError("scene has no 8-bit images")
            self.set_keyframes_u8(sc.frame_idx, sc.images_u8, sc.image_scale, sc.poses)
        else:
            self.set_keyframes(sc.frame_idx, sc.images, sc.poses)

    def set_keyframes(self, frame_idx, images, poses):
        F, H, W, _ = images.shape
        a = [_fp(frame_idx, np.int32), _fp(images), _fp(poses)]
        self._check(self._fn("set_keyframes")(self.ctx, C.c_int(F), a[0][1], a[1][1], C.c_int(W), C.c_int(H), a[2][1]), "set_keyframes")

    def set_keyframes_frames(self, frame_idx, image_list, poses):
        """one array [H][W][3] per keyframe (psgsdf_set_keyframes_frames: the host keeps one allocation per image)"""
        imgs = [np.ascontiguousarray(im, np.float32) for im in image_list]
        H, W, _ = imgs[0].shape
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        a = [_fp(frame_idx, np.int32), _fp(poses)]
        self._check(self._fn("set_keyframes_frames")(self.ctx, C.c_int(len(imgs)), a[0][1], ptrs, C.c_int(W), C.c_int(H), a[1][1]), "set_keyframes_frames")

    def set_keyframes_u8(self, frame_idx, images_u8, scale, poses):
        """8-bit RGB keyframes [F][H][W][3] + the loader's conversion factor (colour = byte * scale)"""
        F, H, W = images_u8.shape[:3]
        img = np.ascontiguousarray(images_u8, dtype=np.uint8)
        a = [_fp(frame_idx, np.int32), _fp(poses)]
        self._check(self._fn("set_keyframes_u8")(self.ctx, C.c_int(F), a[0][1], img.ctypes.data_as(C.c_void_p), C.c_float(scale),
                                                    C.c_int(W), C.c_int(H), a[1][1]), "set_keyframes_u8")

    def load_scene(self, sc, u8=None):
        """u8: hand the keyframes over as 8-bit RGB when the scene has them (default: whenever it has)"""
        self.upload_volume(sc.dist, sc.grad, sc.weight, sc.rgb, sc.vis, sc.vis_words)
        self._scene_keyframes(sc, u8, require=True)
        self.init()

    def init(self):
        self._check(self._fn("init")(self.ctx), "init")

    # -- state producer (VolumetricGradSdf::init / update)
    def volume_init(self, max_frames):
        self._check(self._fn("volume_init")(self.ctx, C.c_int(max_frames)), "volume_init")

    def integrate_frame(self, rgb, depth, normals, pose, counter, z_min=0.05, z_max=10.0):
        H, W = depth.shape
        a = [_fp(rgb), _fp(depth), _fp(normals), _fp(pose)]
        self._check(self._fn("integrate_frame")(self.ctx, a[0][1], a[1][1], a[2][1], C.c_int(W), C.c_int(H), a[3][1], C.c_int(counter),
                                                 C.c_float(z_min), C.c_float(z_max)), "integrate_frame")

    def estimate_normals(self, depth):
        H, W = depth.shape
        a = _fp(depth)
        out = np.empty((3, H, W), np.float32)
        self._check(self._fn("estimate_normals")(self.ctx, a[1], C.c_int(W), C.c_int(H), out.ctypes.data_as(C.c_void_p)), "estimate_normals")
        return out

    def track(self, depth, pose, z_min=0.05, z_max=10.0, num_iterations=50, conv_threshold=1e-3, damping=1.0):
        H, W = depth.shape
        a = _fp(depth)
        P = np.ascontiguousarray(pose, np.float32).reshape(16).copy()
        it = C.c_int(); conv = C.c_int()
        self._check(self._fn("track")(self.ctx, a[1], C.c_int(W), C.c_int(H), P.ctypes.data_as(C.c_void_p), C.c_float(z_min), C.c_float(z_max),
                                      C.c_int(num_iterations), C.c_float(conv_threshold), C.c_float(damping), C.byref(it), C.byref(conv)), "track")
        return P.reshape(4, 4), it.value, bool(conv.value)

    def download_vis_seq(self, words):
        i = self.info()
        n = int(i.dim[0]) * int(i.dim[1]) * int(i.dim[2])
        out = np.zeros((n, words), np.uint64)      # (a slab fills the planes it owns)
        f = self._fn("download_vis_seq")
        rc = f(self.ctx, out.ctypes.data_as(C.c_void_p))
        if rc < 0:
            self._check(rc, "download_vis_seq")
        return out

    # -- hot path
    def init_albedo(self):
        self._check(self._fn("init_albedo")(self.ctx), "init_albedo")

    def energy(self):
        out = (C.c_double * 4)()
        self._check(self._fn("energy")(self.ctx, out), "energy")
        return list(out)

    def normalize_weights(self):
        e = C.c_double()
        self._check(self._fn("normalize_weights")(self.ctx, C.byref(e)), "normalize_weights")
        return e.value

    def step(self, block):
        st = StepStats()
        self._check(self._fn("step")(self.ctx, C.c_int(block), C.byref(st)), "step")
        return st.as_dict()

    def iterate(self, flags, n):
        arr = (IterStats * n)()
        self._check(self._fn("iterate")(self.ctx, C.c_int(flags), C.c_int(n), arr), "iterate")
        return [a.as_dict() for a in arr]

    def optimize(self, flags, cap=256, on_iter=None):
        """on_iter(iterations_done, record_dict) -> truthy aborts the loop (psgsdf_iter_cb: the host's hook for the reference's periodic dumps)"""
        arr = (IterStats * cap)()
        n, res = C.c_int(), C.c_int()
        cb = None
        if on_iter is not None:
            cb = _ITER_CB(lambda user, done, rec: 1 if on_iter(done, rec.contents.as_dict()) else 0)
        self._check(self._fn("optimize")(self.ctx, C.c_int(flags), arr, C.c_int(cap), C.byref(n), C.byref(res), cb, None), "optimize")
        return [arr[i].as_dict() for i in range(min(n.value, cap))], bool(res.value)

    def set_on_iter_period(self, period):
        self._check(self._fn("set_on_iter_period")(self.ctx, C.c_int(period)), "set_on_iter_period")

    def set_record_observer(self, fn):
        """fn(iterations_done, record) -> truthy ends the loop (record: an IterStats copy, rec["e_total"] / rec.as_dict()); passive (psgsdf_set_record_observer): must not call into the engine"""
        if fn is None:
            self._observer = None
            self._check(self._fn("set_record_observer")(self.ctx, None, None), "set_record_observer")
            return
        self._observer = _ITER_CB(lambda user, done, rec: 1 if fn(done, IterStats.from_buffer_copy(rec.contents)) else 0)      # (a 120-byte copy, fields read on demand: the callback sits on the loop's critical path)
        self._check(self._fn("set_record_observer")(self.ctx, self._observer, None), "set_record_observer")

    def upsample2x(self):
        self._check(self._fn("upsample2x")(self.ctx), "upsample2x")

    # -- outputs
    def info(self):
        i = Info()
        self._check(self._fn("get_info")(self.ctx, C.byref(i)), "get_info")
        return i

    def _vs(self):
        """the voxel size as the engine rounds it: the unit of the extraction calls' default radii and biases"""
        return float(np.float32(self.info().voxel_size))

    def download_volume(self, want_vis=False):
        i = self.info()
        n = int(i.dim[0]) * int(i.dim[1]) * int(i.dim[2])
        dist = np.full(n, np.nan, np.float32); grad = np.full((3, n), np.nan, np.float32)      # (a slab fills its own planes only)
        weight = np.full(n, np.nan, np.float32); rgb = np.full((3, n), np.nan, np.float32)
        vis = np.empty((n, i.vis_words), np.uint64) if want_vis else None
        self._check(self._fn("download_volume")(self.ctx, dist.ctypes.data_as(C.c_void_p), grad.ctypes.data_as(C.c_void_p),
                                                 weight.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p),
                                                 vis.ctypes.data_as(C.c_void_p) if want_vis else None), "download_volume")
        return dict(dist=dist, grad=grad, weight=weight, rgb=rgb, vis=vis)

    # -- view rendering (include/psgsdf_render.h)
    def _view(self, what, frame, pose, K, size, light_frame=0):
        """(psgsdf_view, W, H) of a keyframe, or of a caller's camera (pose, K, size)"""
        v = View()
        if frame is not None:
            v.frame = int(frame)
            w_, h_ = C.c_int32(), C.c_int32()
            self._check(self._fn("render_size")(self.ctx, C.byref(v), C.byref(w_), C.byref(h_)), "render_size")
            return v, w_.value, h_.value
        if pose is None or K is None or size is None:
            raise ValueError(f"{what}: a keyframe or (pose, K, size)")
        v.frame = -1
        v.pose[:] = [float(x) for x in np.asarray(pose, np.float32).reshape(16)]
        k = np.asarray(K, np.float64).reshape(-1)
        v.fx, v.fy, v.cx, v.cy = (k[0], k[4], k[2], k[5]) if k.size == 9 else tuple(k[:4])
        v.width, v.height = int(size[0]), int(size[1])
        v.light_frame = int(light_frame)
        return v, v.width, v.height

    def render(self, frame=None, pose=None, K=None, size=None, channels=None, light_frame=0):
        """frame: a keyframe view; otherwise a caller's camera: pose (4x4 or 16 camera->world), K (3x3 or [fx, fy, cx, cy]), size (W, H),
        shaded with the light of keyframe light_frame.  channels: R_* bits (default: every plane the view has).  Returns {plane name: array [ch, H, W] (voxel: int32 [H, W], depth / shading: [H, W])}
        plus "stats" (RenderStats.as_dict).  On a context attached to a rank: a collective call (every rank the same view), every rank gets the whole view."""
        v, W, H = self._view("render", frame, pose, K, size, light_frame)
        if channels is None:
            channels = R_ALL if frame is not None else (R_ALL & ~R_RESIDUAL)
        nch = sum(n for _, bit, n in _R_PLANES if channels & bit)
        out = np.zeros((max(nch, 1), H, W), np.float32)
        st = RenderStats()
        self._check(self._fn("render")(self.ctx, C.byref(v), C.c_uint32(channels), out.ctypes.data_as(C.c_void_p) if nch else None, C.byref(st)), "render")
        res, q = {}, 0
        for name, bit, n in _R_PLANES:
            if channels & bit:
                a = out[q:q + n]
                res[name] = a.view(np.int32)[0].copy() if name == "voxel" else (a[0].copy() if n == 1 else a.copy())
                q += n
        res["stats"] = st.as_dict()
        return res

    # -- relighting (include/psgsdf_relight.h)
    def relight(self, lights, frame=None, pose=None, K=None, size=None, bias=None, reach=None, geometry=False):
        """One view (a keyframe, or a caller's camera: pose, K, size as for render) under up to 64 lights of the caller's, with the shadows the
        reconstruction casts on itself (psgsdf_relight).  lights: a list of dicts (make_light: kind "sh" / "directional" / "point", sh, vec, colour,
        ambient, spread, samples).  bias: the shadow rays' lift off the surface (None: 1 voxel); reach: how far a ray occludes (None or 0: no limit).
        dict of rendered [L, 3, H, W], visibility [L, H, W], counts (per light: n_hits, n_lit, n_rays, n_occluded, n_buried) and, with geometry,
        depth, normal, albedo and voxel as render returns them.  Single contexts only."""
        v, W, H = self._view("relight", frame, pose, K, size)
        arr = (Light * max(len(lights), 1))(*[make_light(d) for d in lights])
        vs = self._vs()
        p = RelightParams(float(vs if bias is None else bias), float(0.0 if reach is None else reach), len(lights), 0)
        out = np.zeros((max(len(lights), 1), 4, H, W), np.float32)
        geo = np.zeros((8, H, W), np.float32) if geometry else None
        cnt = (RelightCounts * max(len(lights), 1))()
        self._check(self._fn("relight")(self.ctx, C.byref(v), arr, C.byref(p), out.ctypes.data_as(C.c_void_p), geo.ctypes.data_as(C.c_void_p) if geometry else None, cnt), "relight")
        res = dict(rendered=out[:, :3].copy(), visibility=out[:, 3].copy(), counts=[_counts(cnt[l]) for l in range(len(lights))])
        if geometry:
            res.update(depth=geo[0].copy(), normal=geo[1:4].copy(), albedo=geo[4:7].copy(), voxel=geo[7].view(np.int32).copy())
        return res

    def render_report(self):
        """per keyframe: RenderStats.as_dict of the re-rendering of that keyframe (one batched pass; collective on a context attached to a rank)"""
        F = self.info().n_frames
        arr = (RenderStats * F)()
        self._check(self._fn("render_report")(self.ctx, arr), "render_report")
        return [arr[f].as_dict() for f in range(F)]

    # -- the writers' geometry, extracted on the device (valid until the next extraction: copied here)
    def extract_mesh(self):
        """(xyz [n_vertices, 3] float32 grid-local, rgb [n_vertices, 3] uint8): three consecutive vertices are one face (psgsdf_extract_mesh)"""
        xyz, rgb, n = _F32P(), _U8P(), C.c_int64()
        self._check(self._fn("extract_mesh")(self.ctx, C.byref(xyz), C.byref(rgb), C.byref(n)), "extract_mesh")
        return _owned(xyz, (n.value, 3), np.float32), _owned(rgb, (n.value, 3), np.uint8)

    def extract_mesh_indexed(self):
        """(xyz [V, 3] float32 grid-local, normals [V, 3] float32, rgb [V, 3] uint8, faces [F, 3] int32, first_vertex): the welded mesh of
        include/psgsdf_mesh.h.  On a context attached to a rank: a collective call returning this rank's share; face indices are global and
        first_vertex is the global number of the share's vertex 0."""
        m, first = _MeshHead(), C.c_int64()
        self._check(self._fn("extract_mesh_indexed")(self.ctx, *m.refs(), C.byref(first)), "extract_mesh_indexed")
        return (*m.arrays().values(), first.value)

    def extract_mesh_components(self, min_faces=0, min_area=0.0, keep_largest=0):
        """The welded mesh without the components the filter drops, and the table of ALL its components (include/psgsdf_mesh.h
        psgsdf_extract_mesh_components): dict of xyz [V, 3] float32, normals [V, 3] float32, rgb [V, 3] uint8, faces [F, 3] int32 (renumbered),
        vertex_component [V] int32 (index into components), components (structured array, MESH_COMPONENT_DTYPE).  A component passes if
        n_faces >= min_faces and area >= min_area; keep_largest > 0 keeps only that many of them, those with the most faces.  Single contexts only."""
        return self._mesh_components("extract_mesh_components", [C.byref(_mesh_filter(min_faces, min_area, keep_largest, always=True))])

    def _mesh_components(self, name, args, more=()):
        """a call that returns the welded mesh, its vertices' components and the component table after its own `args`, and `more` after those"""
        m, vc, comps, nc = _MeshHead(), _I32P(), C.c_void_p(), C.c_int64()
        self._check(self._fn(name)(self.ctx, *args, *m.refs(), C.byref(vc), C.byref(comps), C.byref(nc), *more), name)
        K = nc.value
        table = np.frombuffer(C.string_at(comps, K * MESH_COMPONENT_DTYPE.itemsize), MESH_COMPONENT_DTYPE).copy() if K else np.zeros(0, MESH_COMPONENT_DTYPE)
        return dict(m.arrays(), vertex_component=_owned(vc, (m.n_vertices,), np.int32), components=table)

    def extract_mesh_lod(self, cell, min_faces=0, min_area=0.0, keep_largest=0):
        """A coarser mesh by vertex clustering (include/psgsdf_mesh.h psgsdf_extract_mesh_lod): the vertices of the welded mesh -- of the mesh
        extract_mesh_components(min_faces, min_area, keep_largest) returns, if one of the three is non-zero -- that fall into the same cube of
        edge `cell` (the mesh's units) become one vertex.  dict of xyz [V, 3] float32, normals [V, 3] float32, rgb [V, 3] uint8, faces [F, 3] int32,
        vertex_map [n_vertices_in] int32 (the output vertex of every input vertex, or -1), n_vertices_in, n_faces_in.  Single contexts only."""
        m, vm, nvi, nfi = _MeshHead(), _I32P(), C.c_int64(), C.c_int64()
        self._check(self._fn("extract_mesh_lod")(self.ctx, _ref(_mesh_filter(min_faces, min_area, keep_largest)), C.c_double(float(cell)), *m.refs(),
                                                 C.byref(vm), C.byref(nvi), C.byref(nfi)), "extract_mesh_lod")
        return dict(m.arrays(), vertex_map=_owned(vm, (nvi.value,), np.int32), n_vertices_in=nvi.value, n_faces_in=nfi.value)

    def bake_lod(self, cell, res, reach=None, min_faces=0, min_area=0.0, keep_largest=0):
        """Albedo, normal and displacement maps baked onto the level-of-detail mesh (include/psgsdf_bake.h psgsdf_bake_lod): extract_mesh_lod's dict for
        the same cell and filter, plus uv [F, 3, 2] float32 (v pointing down), width, height, the atlas planes albedo [H, W, 3] uint8, normal [H, W, 3]
        float32, displacement [H, W] float32, voxel [H, W] int32 (-1: no hit), face [H, W] int32 (-1: padding) and the counts n_texels, n_hits,
        n_hits_off_band, n_buried, n_misses.  res: texels along a triangle's edge; reach: how far outside the coarse triangle a texel's ray starts, in
        the mesh's units (None: cell).  Single contexts only."""
        return self._bake("bake_lod", (min_faces, min_area, keep_largest), cell, res, reach, None, Bake())

    def _bake(self, name, flt, cell, res, reach, params, result):
        """one of the psgsdf_bake_lod* calls: the arguments they share (flt: min_faces, min_area, keep_largest), the call's own params struct (or None:
        it has none) and its result struct, a Bake or a struct that begins with one; _bake_dict of that bake, to which the caller adds its own planes"""
        own = () if params is None else (C.byref(params),)
        self._check(self._fn(name)(self.ctx, _ref(_mesh_filter(*flt)), C.c_double(float(cell)), C.c_int32(int(res)), C.c_double(float(cell if reach is None else reach)),
                                   *own, C.byref(result)), name)
        return self._bake_dict(result if isinstance(result, Bake) else result.bake)

    @staticmethod
    def _bake_dict(b):
        Vi, W, H = b.n_vertices_in, b.width, b.height
        out = dict(_mesh_arrays(b), vertex_map=_owned(b.vertex_map, (Vi,), np.int32), n_vertices_in=Vi, n_faces_in=b.n_faces_in,
                   uv=_owned(b.uv, (b.n_faces if W else 0, 3, 2), np.float32), width=W, height=H, albedo=_owned(b.albedo, (H, W, 3), np.uint8),
                   normal=_owned(b.normal, (H, W, 3), np.float32), displacement=_owned(b.displacement, (H, W), np.float32), voxel=_owned(b.voxel, (H, W), np.int32),
                   face=_owned(b.face, (H, W), np.int32))
        for k in ("n_texels", "n_hits", "n_hits_off_band", "n_buried", "n_misses"):
            out[k] = int(getattr(b, k))
        return out

    # -- ambient occlusion (include/psgsdf_occlusion.h)
    def _ao_params(self, n_dirs, radius, bias):
        vs = self._vs()
        return AoParams(int(n_dirs), 0, float(8 * vs if radius is None else radius), float(vs if bias is None else bias))

    def occlusion_points(self, xyz, normals, n_dirs=16, radius=None, bias=None):
        """Ambient occlusion of the reconstructed surface at the caller's points xyz [n, 3] and normals [n, 3] (float32, the mesh's units;
        psgsdf_occlusion_points): n_dirs (8, 16, 32 or 64) cosine-weighted rays per point, each occluded if it meets the surface within `radius`
        (None: 8 voxels) of its origin, which is lifted off the point by `bias` (None: 1 voxel) along the normal.  dict of occlusion [n] uint8
        (255: open), mask [n] uint64 (bit i: ray i is occluded), dirs [n_dirs, 3] float64 and counts, a dict of n_samples, n_valid, n_rays, n_occluded,
        n_buried (the last two count rays).  Single contexts only."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(xyz) != len(normals):
            raise ValueError("occlusion_points: xyz and normals differ in length")
        n, p = len(xyz), self._ao_params(n_dirs, radius, bias)
        mask = C.POINTER(C.c_uint64)(); occ = _U8P(); dirs = C.POINTER(C.c_double)(); cnt = AoCounts()
        self._check(self._fn("occlusion_points")(self.ctx, xyz.ctypes.data_as(_F32P), normals.ctypes.data_as(_F32P), C.c_int64(n), C.byref(p),
                                                 C.byref(mask), C.byref(occ), C.byref(dirs), C.byref(cnt)), "occlusion_points")
        return dict(occlusion=_owned(occ, (n,), np.uint8), mask=_owned(mask, (n,), np.uint64), dirs=_owned(dirs, (p.n_dirs, 3), np.float64), counts=_counts(cnt))

    def bake_lod_ao(self, cell, res, reach=None, n_dirs=16, radius=None, bias=None, min_faces=0, min_area=0.0, keep_largest=0):
        """bake_lod's dict for the same arguments (bit for bit) plus the ambient-occlusion map of the atlas (psgsdf_bake_lod_ao): occlusion [H, W]
        uint8 (255: open; padding 0), mask [H, W] uint64, dirs [n_dirs, 3] float64 and counts, a dict of n_samples (the owned texels), n_valid,
        n_rays, n_occluded, n_buried (rays; the bake's own n_buried, texels, stays where it is).  n_dirs, radius, bias: as for occlusion_points.  Single contexts only."""
        b = BakeAo()
        out = self._bake("bake_lod_ao", (min_faces, min_area, keep_largest), cell, res, reach, self._ao_params(n_dirs, radius, bias), b)
        H, W = out["height"], out["width"]
        out.update(occlusion=_owned(b.occlusion, (H, W), np.uint8), mask=_owned(b.mask, (H, W), np.uint64), dirs=_owned(b.dirs, (b.n_dirs, 3), np.float64), counts=_counts(b.counts))
        return out

    # -- the field at the caller's points and along the caller's rays (include/psgsdf_query.h)
    @staticmethod
    def _query_model(model):
        return QUERY_MODELS[model] if isinstance(model, str) else int(model)

    def query_points(self, xyz, model="trilinear"):
        """The field at the caller's points xyz [n, 3] (float32, the mesh's units; psgsdf_query_points) under `model`: "cell", the renderer's
        first-order model of the point's cell, or "trilinear", the cell the mesher cuts (or the header's 0 / 1).  dict of status [n] uint8 (0 ok,
        1 outside the grid, 2 unobserved, 3 not finite), dist [n], normal [n, 3], rgb [n, 3], weight [n] float32 (zeros unless the status is 0),
        voxel [n] int64 (-1: none) and counts, a dict of n, n_ok, n_outside, n_unobserved, n_invalid.  Single contexts only."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        st = _U8P(); dist, nrm, rgb, wgt = _F32P(), _F32P(), _F32P(), _F32P(); vox = C.POINTER(C.c_int64)(); cnt = QueryCounts()
        self._check(self._fn("query_points")(self.ctx, xyz.ctypes.data_as(_F32P) if n else None, C.c_int64(n), C.c_int32(self._query_model(model)), C.byref(st), C.byref(dist),
                                             C.byref(nrm), C.byref(rgb), C.byref(wgt), C.byref(vox), C.byref(cnt)), "query_points")
        return dict(status=_owned(st, (n,), np.uint8), dist=_owned(dist, (n,), np.float32), normal=_owned(nrm, (n, 3), np.float32), rgb=_owned(rgb, (n, 3), np.float32),
                    weight=_owned(wgt, (n,), np.float32), voxel=_owned(vox, (n,), np.int64), counts=_counts(cnt))

    def project_points(self, xyz, model="trilinear", tol=None, max_iters=16, reserved=0.0):
        """The caller's points moved onto the model's zero set by steps of phi along the model's normal (psgsdf_project_points) until |phi| <= tol
        (None: 1e-3 voxel), the point leaves the observed grid, or max_iters (1 .. 64) moves are made.  dict of status [n] uint8 (as query_points;
        4: not converged), xyz [n, 3] float32 the point at the stop, residual [n] float32 the model there, normal [n, 3] float32, voxel [n] int64,
        iterations [n] uint8 the moves made, distance [n] float32 the length moved, negative for a point that started inside, and counts, a dict
        of n, n_converged, n_left, n_not_converged, n_invalid.  Single contexts only."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        p = ProjectParams(self._query_model(model), int(max_iters), float(1e-3 * self._vs() if tol is None else tol), float(reserved))
        st, it = _U8P(), _U8P(); out, res, nrm, moved = _F32P(), _F32P(), _F32P(), _F32P(); vox = C.POINTER(C.c_int64)(); cnt = ProjectCounts()
        self._check(self._fn("project_points")(self.ctx, xyz.ctypes.data_as(_F32P) if n else None, C.c_int64(n), C.byref(p), C.byref(st), C.byref(out), C.byref(res), C.byref(nrm),
                                               C.byref(vox), C.byref(it), C.byref(moved), C.byref(cnt)), "project_points")
        return dict(status=_owned(st, (n,), np.uint8), xyz=_owned(out, (n, 3), np.float32), residual=_owned(res, (n,), np.float32), normal=_owned(nrm, (n, 3), np.float32),
                    voxel=_owned(vox, (n,), np.int64), iterations=_owned(it, (n,), np.uint8), distance=_owned(moved, (n,), np.float32), counts=_counts(cnt))

    def cast_rays(self, origins, directions, t_min=0.0, t_max=None):
        """What the caller's rays hit (psgsdf_cast_rays): origins, directions [n, 3] float32 (the mesh's units; a direction of any length > 0), each
        walked through the renderer's cells from t_min to t_max (None: no limit), lengths along the ray in mesh units.  dict of status [n] uint8
        (0 hit, 1 miss, 2 buried: the ray starts at or below the surface, a hit at t_min, 3 invalid), t [n], xyz [n, 3], normal [n, 3], rgb [n, 3]
        float32 (zeros unless the ray hits), voxel [n] int64 the hit cell (-1: none) and counts, a dict of n, n_valid, n_hits, n_buried.
        Single contexts only."""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3); directions = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(origins) != len(directions):
            raise ValueError("cast_rays: origins and directions differ in length")
        n = len(origins)
        p = RayParams(float(t_min), float("inf") if t_max is None else float(t_max))
        st = _U8P(); t, xyz, nrm, rgb = _F32P(), _F32P(), _F32P(), _F32P(); vox = C.POINTER(C.c_int64)(); cnt = RayCounts()
        self._check(self._fn("cast_rays")(self.ctx, origins.ctypes.data_as(_F32P) if n else None, directions.ctypes.data_as(_F32P) if n else None, C.c_int64(n), C.byref(p),
                                          C.byref(st), C.byref(t), C.byref(xyz), C.byref(nrm), C.byref(rgb), C.byref(vox), C.byref(cnt)), "cast_rays")
        return dict(status=_owned(st, (n,), np.uint8), t=_owned(t, (n,), np.float32), xyz=_owned(xyz, (n, 3), np.float32), normal=_owned(nrm, (n, 3), np.float32),
                    rgb=_owned(rgb, (n, 3), np.float32), voxel=_owned(vox, (n,), np.int64), counts=_counts(cnt))

    # -- curvature of the reconstructed surface (include/psgsdf_curvature.h)
    def curvature_voxels(self, lin):
        """Curvature of the distance field's level set through the centre of each voxel lin[q] (linear indices (k ny + j) nx + i, any order, any
        value; psgsdf_curvature_voxels): dict of valid [n] uint8, mean, gauss, k1, k2 [n] float32 (inverse mesh units; a convex sphere of radius r
        has mean = k1 = k2 = 1 / r) and dir1 [n, 3] float32, the unit direction of k1.  An invalid voxel -- out of range, on a grid face, a stencil
        voxel unobserved, a zero gradient -- holds zeros.  Single contexts only."""
        lin = np.ascontiguousarray(lin, np.int64).reshape(-1)
        n = len(lin)
        vl = _U8P(); ptr = [_F32P() for _ in range(5)]
        self._check(self._fn("curvature_voxels")(self.ctx, lin.ctypes.data_as(C.POINTER(C.c_int64)) if n else None, C.c_int64(n), C.byref(vl), *[C.byref(p) for p in ptr]), "curvature_voxels")
        out = dict(valid=_owned(vl, (n,), np.uint8))
        for name, p in zip(("mean", "gauss", "k1", "k2"), ptr):
            out[name] = _owned(p, (n,), np.float32)
        out["dir1"] = _owned(ptr[4], (n, 3), np.float32)
        return out

    def extract_mesh_curvature(self):
        """The welded mesh with the curvature of its vertices (psgsdf_extract_mesh_curvature): dict of xyz, normals, rgb, faces (extract_mesh_indexed's
        arrays) and valid [V] uint8 (how many of the vertex's end voxels are valid: 2, 1 or 0), mean, gauss, k1, k2 [V] float32, interpolated between
        the end voxels' results with the vertex's own parameter; zeros where valid == 0.  Single contexts only."""
        m, vl, ptr = _MeshHead(), _U8P(), [_F32P() for _ in range(4)]
        self._check(self._fn("extract_mesh_curvature")(self.ctx, *m.refs(), C.byref(vl), *[C.byref(p) for p in ptr]), "extract_mesh_curvature")
        out = dict(m.arrays(), valid=_owned(vl, (m.n_vertices,), np.uint8))
        for name, p in zip(("mean", "gauss", "k1", "k2"), ptr):
            out[name] = _owned(p, (m.n_vertices,), np.float32)
        return out

    def bake_lod_curvature(self, cell, res, reach=None, min_faces=0, min_area=0.0, keep_largest=0):
        """bake_lod's dict for the same arguments (bit for bit) plus the mean curvature of every hit texel's voxel (psgsdf_bake_lod_curvature):
        mean [H, W] float32, valid [H, W] uint8 (0 / 0 on missed, buried and padding texels) and n_valid.  Single contexts only."""
        b = BakeCurvature()
        out = self._bake("bake_lod_curvature", (min_faces, min_area, keep_largest), cell, res, reach, None, b)
        H, W = out["height"], out["width"]
        out.update(mean=_owned(b.mean, (H, W), np.float32), valid=_owned(b.valid, (H, W), np.uint8), n_valid=int(b.n_valid))
        return out

    # -- unobserved voxels filled, and the closed mesh of the filled state (include/psgsdf_fill.h)
    def fill_voxels(self, rounds, sweeps=4):
        """The unobserved voxels within `rounds` city-block steps of an observed one, filled by front propagation of the first-order model
        d + g . dx and relaxed by `sweeps` Jacobi sweeps (psgsdf_fill_voxels): dict of lin [n] int64 (ascending), dist [n], grad [n, 3], rgb [n, 3]
        float32 and round [n] uint8 (the round a voxel was reached in, 1 .. rounds).  The context's state does not change.  Single contexts only."""
        lin = C.POINTER(C.c_int64)(); ptr = [_F32P() for _ in range(3)]; rnd = _U8P(); n = C.c_int64()
        self._check(self._fn("fill_voxels")(self.ctx, C.c_int32(int(rounds)), C.c_int32(int(sweeps)), C.byref(lin), *[C.byref(p) for p in ptr], C.byref(rnd), C.byref(n)), "fill_voxels")
        n = n.value
        return dict(lin=_owned(lin, (n,), np.int64), dist=_owned(ptr[0], (n,), np.float32), grad=_owned(ptr[1], (n, 3), np.float32), rgb=_owned(ptr[2], (n, 3), np.float32),
                    round=_owned(rnd, (n,), np.uint8))

    def extract_mesh_filled(self, rounds, sweeps=4, min_faces=0, min_area=0.0, keep_largest=0):
        """extract_mesh_components' dict for the state with its unobserved voxels filled as fill_voxels(rounds, sweeps) fills them
        (psgsdf_extract_mesh_filled), plus vertex_filled [V] uint8: how many of the vertex's end voxels are filled, 0, 1 or 2.  rounds = 0 gives
        extract_mesh_components' arrays bit for bit.  Single contexts only."""
        vf = _U8P()
        out = self._mesh_components("extract_mesh_filled", [C.c_int32(int(rounds)), C.c_int32(int(sweeps)), _ref(_mesh_filter(min_faces, min_area, keep_largest))], [C.byref(vf)])
        out["vertex_filled"] = _owned(vf, (len(out["xyz"]),), np.uint8)
        return out

    # -- the albedo texture solved from the keyframes (include/psgsdf_photo.h)
    def bake_lod_photo(self, cell, res, reach=None, bias=None, cos_min=0.2, shade_min=0.05, status=False, min_faces=0, min_area=0.0, keep_largest=0):
        """bake_lod's dict for the same arguments (bit for bit) plus the albedo of every texel solved from the keyframes that see it
        (psgsdf_bake_lod_photo): photo [H, W, 3] float32 (unclamped), photo_rgb [H, W, 3] uint8, n_obs [H, W] int32 (keyframes used), status
        [n_frames, H, W] uint8 (PHOTO_USED, _OUTSIDE, _GRAZING, _OCCLUDED, _DARK, _NO_SAMPLE) or None unless `status`, and counts, a dict of
        n_samples, n_pairs, n_used, n_outside, n_grazing, n_occluded, n_buried, n_dark, n_texels_solved.  A keyframe counts for a texel if the
        texel projects into it, its normal makes a cosine > cos_min with the direction to the camera, the ray towards the camera (lifted off the
        surface by `bias`; None: 1 voxel) is free, and the model's shading is >= shade_min.  After init; single contexts only."""
        vs = self._vs()
        b, p = BakePhoto(), PhotoParams(float(vs if bias is None else bias), float(cos_min), float(shade_min), 1 if status else 0, 0)
        out = self._bake("bake_lod_photo", (min_faces, min_area, keep_largest), cell, res, reach, p, b)
        H, W = out["height"], out["width"]
        out.update(photo=_owned(b.photo, (H, W, 3), np.float32), photo_rgb=_owned(b.photo_rgb, (H, W, 3), np.uint8), n_obs=_owned(b.n_obs, (H, W), np.int32),
                   status=_owned(b.status, (b.n_frames, H, W), np.uint8) if status else None, counts=_counts(b.counts))
        return out

    # -- comparison with a reference mesh or cloud (include/psgsdf_compare.h)
    def compare_reference(self, ref_xyz, ref_faces=None, max_dist=None, tau=None, grid_cell=0.0, min_faces=0, min_area=0.0, keep_largest=0):
        """Two-sided nearest distances between the welded mesh (with a filter: its kept components, as extract_mesh_components) and a reference
        (psgsdf_compare_reference): ref_xyz [n, 3] float32 in the mesh's units, ref_faces [f, 3] int32 or None for a cloud.  A pair farther apart
        than max_dist (None: 8 voxels) is no match; tau (None: 1 voxel) is the threshold of precision and recall; grid_cell sizes the search grid
        (0: the engine's choice; no result depends on it).  dict of numpy copies: the compared mesh xyz, normals, rgb, faces; vertex_dist [V] float32
        (inf: unmatched), vertex_nearest [V] int32 (a reference face or point, -1: none), vertex_side [V] int8; ref_dist, ref_nearest (a face of the
        mesh), ref_side [n] the other way; to_reference and to_reconstruction, dicts of psgsdf_compare_side's fields (hist: [16] int64); precision,
        recall, fscore.  Single contexts only."""
        ref_xyz, faces, ref = _reference(ref_xyz, ref_faces)
        vs = self._vs()
        p = CompareParams(float(8 * vs if max_dist is None else max_dist), float(vs if tau is None else tau), float(grid_cell), (C.c_int32 * 2)(0, 0))
        r = Compare()
        self._check(self._fn("compare_reference")(self.ctx, _ref(_mesh_filter(min_faces, min_area, keep_largest)), *ref, C.byref(p), C.byref(r)), "compare_reference")
        V, n = r.n_vertices, len(ref_xyz)
        out = dict(_mesh_arrays(r), vertex_dist=_owned(r.vertex_dist, (V,), np.float32), vertex_nearest=_owned(r.vertex_nearest, (V,), np.int32),
                   vertex_side=_owned(r.vertex_side, (V,), np.int8), ref_dist=_owned(r.ref_dist, (n,), np.float32), ref_nearest=_owned(r.ref_nearest, (n,), np.int32),
                   ref_side=_owned(r.ref_side, (n,), np.int8), precision=float(r.precision), recall=float(r.recall), fscore=float(r.fscore))
        for name in ("to_reference", "to_reconstruction"):
            s = getattr(r, name)
            out[name] = {k: (np.array(s.hist, np.int64) if k == "hist" else getattr(s, k)) for k, _ in CompareSide._fields_}
        return out

    # -- rigid alignment of a reference to the welded mesh (include/psgsdf_align.h)
    def align_reference(self, ref_xyz, ref_faces=None, init=None, max_dist=None, min_dist=None, shrink=1.0, directions=3, max_iters=30, eps_rot=1e-5, eps_trans=None, grid_cell=0.0,
                        min_faces=0, min_area=0.0, keep_largest=0):
        """Point-to-plane ICP of a reference onto the welded mesh (with a filter: its kept components) on the device (psgsdf_align_reference):
        ref_xyz [n, 3] float32, ref_faces [f, 3] int32 or None for a cloud; init a rigid 4x4 taking reference units to mesh units (None: identity).
        The matching radius of iteration k is max(min_dist, max_dist shrink^k) (None: 8 voxels and 1 voxel); directions 1: reference points ->
        mesh faces, 2: mesh vertices -> reference, 3: both; the loop stops after a step with |omega| <= eps_rot and |v| <= eps_trans (None: 1e-3
        voxels) or after max_iters steps.  dict of numpy copies: transform [4, 4] float64, centre [3], status (ALIGN_*), n_iters, iters (a list of
        dicts: radius, rms, n_pairs, min_pivot, step [6]; after TOO_FEW / DEGENERATE one more entry, the state that refused), system0 [28],
        final (a dict like iters'), aligned_xyz [n, 3] float32 (the reference under transform) and the compared mesh xyz, normals, rgb, faces.
        Single contexts only."""
        ref_xyz, faces, ref = _reference(ref_xyz, ref_faces)
        vs = self._vs()
        T = np.eye(4) if init is None else np.ascontiguousarray(init, np.float64).reshape(4, 4)
        p = AlignParams((C.c_double * 16)(*T.ravel()), float(8 * vs if max_dist is None else max_dist), float(vs if min_dist is None else min_dist), float(shrink), float(eps_rot),
                        float(1e-3 * vs if eps_trans is None else eps_trans), float(grid_cell), int(directions), int(max_iters), (C.c_int32 * 2)(0, 0))
        r = Align()
        self._check(self._fn("align_reference")(self.ctx, _ref(_mesh_filter(min_faces, min_area, keep_largest)), *ref, C.byref(p), C.byref(r)), "align_reference")
        shown = r.n_iters + (1 if r.status in (ALIGN_DEGENERATE, ALIGN_TOO_FEW) and r.n_iters < 64 and p.max_iters > 0 else 0)
        return dict(transform=np.array(r.transform, np.float64).reshape(4, 4), centre=np.array(r.centre, np.float64), status=int(r.status), n_iters=int(r.n_iters),
                    iters=[r.iters[k].as_dict() for k in range(shown)], system0=np.array(r.system0, np.float64), final=r.final.as_dict(),
                    aligned_xyz=_owned(r.aligned_xyz, (len(ref_xyz), 3), np.float32), **_mesh_arrays(r))

    # -- the photometric fit resolved over the surface (include/psgsdf_fit.h)
    def band_fit(self):
        """Per band row, in download_band's order (psgsdf_band_fit): dict of n_obs [n_band] int32 (the observations the energy counts), loss [n_band]
        float64 (the row's share of the sum behind energy()[0]: sum(loss) / n_band is E_ps), sum_r2 [n_band, 3] float32 (squared residuals per channel).
        Single contexts only."""
        no = _I32P(); ls = C.POINTER(C.c_double)(); r2 = _F32P(); n = C.c_int64()
        self._check(self._fn("band_fit")(self.ctx, C.byref(no), C.byref(ls), C.byref(r2), C.byref(n)), "band_fit")
        S = n.value
        return dict(n_obs=_owned(no, (S,), np.int32), loss=_owned(ls, (S,), np.float64), sum_r2=_owned(r2, (S, 3), np.float32))

    def extract_mesh_fit(self):
        """The welded mesh with the fit of its vertices (psgsdf_extract_mesh_fit): dict of xyz, normals, rgb, faces (extract_mesh_indexed's arrays) and
        n_obs [V] int32, rms [V] float32, loss [V] float32 -- the observations of the vertex's end voxels, their rms residual and mean robust loss; zeros
        where nothing was observed.  Single contexts only."""
        m, no, rms, ls = _MeshHead(), _I32P(), _F32P(), _F32P()
        self._check(self._fn("extract_mesh_fit")(self.ctx, *m.refs(), C.byref(no), C.byref(rms), C.byref(ls)), "extract_mesh_fit")
        V = m.n_vertices
        return dict(m.arrays(), n_obs=_owned(no, (V,), np.int32), rms=_owned(rms, (V,), np.float32), loss=_owned(ls, (V,), np.float32))

    def extract_pointcloud(self, which=0):
        """(xyz_nxyz [n, 6] float32, rgb [n, 3] int32); which = 0: the band voxels, 1: every fused voxel (psgsdf_extract_pointcloud)"""
        pn, col, n = _F32P(), _I32P(), C.c_int64()
        self._check(self._fn("extract_pointcloud")(self.ctx, C.c_int(which), C.byref(pn), C.byref(col), C.byref(n)), "extract_pointcloud")
        return _owned(pn, (n.value, 6), np.float32), _owned(col, (n.value, 3), np.int32)

    def extract_sdf(self):
        """(lo [3], dim [3], -dist block [dim2, dim1, dim0]) of the crop box |d| <= sqrt(3) vs (psgsdf_extract_sdf)"""
        lo = (C.c_int32 * 3)(); dim = (C.c_int32 * 3)(); v = _F32P()
        self._check(self._fn("extract_sdf")(self.ctx, lo, dim, C.byref(v)), "extract_sdf")
        d = list(dim)
        mi = self.mg_info()      # a slab of a multi-rank run gets the planes of the (global) box it owns
        own = max(0, min(lo[2] + d[2], mi["z1"]) - max(lo[2], mi["z0"])) if mi["n_ranks"] > 1 else d[2]
        empty = d[0] == 0 or own == 0
        return list(lo), d, _owned(v, (0, max(d[1], 0), max(d[0], 0)) if empty else (own, d[1], d[0]), np.float32)

    def download_band(self, n=None):
        """one rank: the whole band.  A slab of a multi-rank run: pass n = row1 - row0 of mg_info (its own band voxels)"""
        if n is None:
            n = self.info().n_band
        b = np.empty(max(n, 1), np.int32)
        self._check(self._fn("download_band")(self.ctx, b.ctypes.data_as(C.c_void_p)), "download_band")
        return b[:n]

    def download_poses(self):
        i = self.info()
        p = np.empty((i.n_frames, 16), np.float32)
        self._check(self._fn("download_poses")(self.ctx, p.ctypes.data_as(C.c_void_p)), "download_poses")
        return p

    def download_light(self):
        i = self.info()
        shape = (3,) if self._settings.model == LED else (i.n_frames, i.light_stride)
        l = np.empty(shape, np.float32)
        self._check(self._fn("download_light")(self.ctx, l.ctypes.data_as(C.c_void_p)), "download_light")
        return l

    def upload_light(self, light):
        a, p = _fp(light)
        self._check(self._fn("upload_light")(self.ctx, p), "upload_light")

    # -- multi-GPU: attach the context to a rank (before load_scene / init); afterwards every call is collective
    def comm_init(self, rank, n_ranks, unique_id=None):
        """unique_id: the 128 bytes rank 0 got from comm_unique_id() (RCCL)"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id)) if unique_id is not None else None
        self._check(self._fn("comm_init")(self.ctx, buf, C.c_int(rank), C.c_int(n_ranks)), "comm_init")

    def comm_init_ext(self, ops, rank, n_ranks):
        """ops: a CommOps struct (caller-supplied transport); the caller keeps it (and its callbacks) alive"""
        self._comm_ops = ops
        self._check(self._fn("comm_init_ext")(self.ctx, C.byref(ops), C.c_int(rank), C.c_int(n_ranks)), "comm_init_ext")

    def debug_overlap_probe(self, reps=10):
        """ms of {distance sweep alone, solve alone, back to back, solve started beside the sweep on a second stream}"""
        out = (C.c_double * 4)()
        self._check(self._fn("debug_overlap_probe")(self.ctx, C.c_int(reps), out), "debug_overlap_probe")
        return list(out)

    def debug_normals_cache(self, width, height):
        """the FALS estimator's per-resolution cache as the device computed it: [9, height, width] float32"""
        out = np.empty((9, height, width), np.float32)
        self._check(self._fn("debug_normals_cache")(self.ctx, C.c_int(width), C.c_int(height), out.ctypes.data_as(C.c_void_p)), "debug_normals_cache")
        return out

    def comm_init_sockets(self, peer_fds, rank, n_ranks):
        """the built-in node-local transport: peer_fds[r] = fileno of a connected stream socket to rank r (the caller keeps the sockets open)"""
        fds = (C.c_int * n_ranks)(*[int(f) for f in peer_fds])
        self._check(self._fn("comm_init_sockets")(self.ctx, fds, C.c_int(rank), C.c_int(n_ranks)), "comm_init_sockets")

    def comm_allreduce_host(self, values):
        """sum over the ranks of a host vector of doubles (collective)"""
        a = np.ascontiguousarray(values, np.float64).copy()
        self._check(self._fn("comm_allreduce_host")(self.ctx, a.ctypes.data_as(C.c_void_p), C.c_int(a.size)), "comm_allreduce_host")
        return a

    def comm_stats(self):
        n = C.c_int64()
        self._check(self._fn("comm_stats")(self.ctx, C.byref(n)), "comm_stats")
        return n.value

    def set_stream(self, stream_ptr):
        self._check(self._fn("set_stream")(self.ctx, C.c_void_p(stream_ptr)), "set_stream")

    def mg_info(self):
        """{S (whole volume), rows held, row0, row1, halo, F, rank, n_ranks, need_lo, need_hi, z0, z1} of a context attached to a rank"""
        out = (C.c_int32 * 12)()
        self._check(self._fn("mg_info")(self.ctx, out), "mg_info")
        return dict(zip(self._MG_INFO_NAMES, list(out)))

    _MG_INFO_NAMES = ["S", "rows", "row0", "row1", "halo", "F", "rank", "n_ranks", "need_lo", "need_hi", "z0", "z1"]

    def get_tuning(self):
        """psgsdf_get_tuning: which environment knobs were set when the context was created, which dev-only ones this build ignores, what they resolved to"""
        import json
        f = getattr(self._lib, self._p + "get_tuning"); f.restype = C.c_int
        n = f(self.ctx, None, C.c_size_t(0))
        if n < 0:
            self._check(n, "get_tuning")
        buf = C.create_string_buffer(n + 1)
        f(self.ctx, buf, C.c_size_t(n + 1))
        return json.loads(buf.value.decode())

    # -- measurement
    def set_profiling(self, on):
        self._check(self._fn("set_profiling")(self.ctx, C.c_int(1 if on else 0)), "set_profiling")

    def watch_kernel(self, name):
        self._check(self._fn("watch_kernel")(self.ctx, name.encode() if name else None), "watch_kernel")

    def reset_kernel_times(self):
        self._check(self._fn("reset_kernel_times")(self.ctx), "reset_kernel_times")

    def kernel_times(self):
        cap = 64
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); n = (C.c_int64 * cap)()
        f = getattr(self._lib, self._p + "kernel_times"); f.restype = C.c_int
        k = f(self.ctx, names, ms, n, C.c_int(cap))
        return {names[i].decode(): (ms[i], n[i]) for i in range(k)}

    # -- test hooks
    def debug_dist_system(self, x=None):
        S = self.info().n_band
        diag = np.empty(S, np.float32); rhs = np.empty(S, np.float32)
        y = np.empty(S, np.float32) if x is not None else None
        xa = np.ascontiguousarray(x, np.float32) if x is not None else None
        self._check(self._fn("debug_dist_system")(self.ctx, diag.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p),
                                                   xa.ctypes.data_as(C.c_void_p) if x is not None else None,
                                                   y.ctypes.data_as(C.c_void_p) if x is not None else None), "debug_dist_system")
        return diag, rhs, y

    def debug_time_pcg_pass(self, blocks=0, rows=2, ablate=0, reps=50, stamps=False):
        ms = C.c_double(0)
        st = np.zeros((max(blocks, 1), 8), np.int64) if stamps else None
        self._check(self._fn("debug_time_pcg_pass")(self.ctx, C.c_int(blocks), C.c_int(rows), C.c_int(ablate | (1024 if stamps else 0)), C.c_int(reps), C.byref(ms),
                                                     st.ctypes.data_as(C.c_void_p) if stamps else None), "debug_time_pcg_pass")
        return (ms.value, st) if stamps else ms.value

    def debug_time_pcg_solve(self, passes=16, reps=5):
        ms = C.c_double(0); shape = (C.c_int32 * 2)(); st = (C.c_double * 16)()
        self._check(self._fn("debug_time_pcg_solve")(self.ctx, C.c_int(passes), C.c_int(reps), C.byref(ms), shape, st), "debug_time_pcg_solve")
        return ms.value, (shape[0], shape[1]), [x for x in st]

    def debug_sync_stats(self):
        out = (C.c_int64 * 8)()
        self._check(self._fn("debug_sync_stats")(self.ctx, out), "debug_sync_stats")
        return dict(readbacks_checked=out[0], readbacks_late=out[1], persist_fallbacks=out[2] % 1000000, keyframes_compacted=out[2] // 1000000, speculative_starts=out[3] // 1000000, speculative_undos=out[3] % 1000000,
                    cross_rank_ready=out[4] % 10, halo_pushes=out[4] // 10, cross_rank_solves=out[5], cross_rank_mem_kind=out[6], probe_stale=out[7] // 1000000, probe_timeouts=out[7] % 1000000)

    def debug_rare_rows(self):
        r = C.c_int64(); w = C.c_int64()
        self._check(self._fn("debug_rare_rows")(self.ctx, C.byref(r), C.byref(w)), "debug_rare_rows")
        return r.value, w.value

    def debug_frame_system(self, block):
        i = self.info()
        if block == LIGHT:
            n = i.light_stride; nb = 1 if self._settings.model == LED else i.n_frames
        else:
            n = 6; nb = i.n_frames
        H = np.empty((nb, n, n), np.float64); b = np.empty((nb, n), np.float64)
        self._check(self._fn("debug_frame_system")(self.ctx, C.c_int(block), H.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)), "debug_frame_system")
        return H, b

    def set_frame_solver(self, mode):
        """0 = every frame's light / pose block solved directly (LDL^T in double; the engine's default), 1 = the reference's solver: ONE Eigen-style float
        Jacobi-PCG over the block-diagonal system of all frames (include/psgsdf.h psgsdf_set_frame_solver; the oracle: orc_set_frame_solver = its solver_mode)"""
        self._check(self._fn("set_frame_solver")(self.ctx, C.c_int(mode)), "set_frame_solver")

    def frame_solver_stats(self, block):
        it = C.c_int32(); err = C.c_double(); ok = C.c_int32(); ap = C.c_int32()
        self._check(self._fn("get_frame_solver_stats")(self.ctx, C.c_int(block), C.byref(it), C.byref(err), C.byref(ok), C.byref(ap)), "get_frame_solver_stats")
        return {"cg_iters": it.value, "cg_error": err.value, "cg_converged": ok.value, "applied": ap.value}

    def debug_frame_cg(self, H, b, max_it=0):
        """the mode-1 frame solver alone on the block-diagonal system H [nb][n][n], b [nb][n] -> (x [nb][n], iterations, error, converged)"""
        H = np.ascontiguousarray(H, np.float32); b = np.ascontiguousarray(b, np.float32)
        nb, n = b.shape
        x = np.empty((nb, n), np.float32); it = C.c_int32(); err = C.c_double(); ok = C.c_int32()
        self._check(self._fn("debug_frame_cg")(self.ctx, C.c_int(nb), C.c_int(n), H.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                               C.c_int(max_it), C.byref(it), C.byref(err), C.byref(ok)), "debug_frame_cg")
        return x, it.value, err.value, bool(ok.value)

    def debug_albedo_system(self):
        S = self.info().n_band
        H = np.empty((S, 3), np.float32); b = np.empty((S, 3), np.float32)
        self._check(self._fn("debug_albedo_system")(self.ctx, H.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)), "debug_albedo_system")
        return H, b


class CommXfer(C.Structure):
    _fields_ = [("ptr_dev", C.c_void_p), ("bytes", C.c_size_t), ("peer", C.c_int)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(CommXfer), C.c_int, C.POINTER(CommXfer), C.c_int, C.c_void_p)


class CommOps(C.Structure):
    """psgsdf_comm_ops: a caller-supplied transport for psgsdf_comm_init_ext"""
    _fields_ = [("user", C.c_void_p), ("allreduce_f64", ALLREDUCE_FN), ("sendrecv", SENDRECV_FN)]


def comm_unique_id() -> bytes:
    """psgsdf_comm_unique_id (ncclGetUniqueId): call on rank 0, hand the bytes to every rank's comm_init"""
    buf = (C.c_uint8 * 128)()
    f = engine_lib().psgsdf_comm_unique_id; f.restype = C.c_int
    rc = f(buf)
    if rc != 0:
        raise PsgsdfError(f"psgsdf_comm_unique_id failed rc={rc} (librccl could not be loaded?)")
    return bytes(buf)


def grid_of(sc) -> GridDesc:
    g = GridDesc()
    g.dim[:] = [int(x) for x in sc.dim]
    g.voxel_size = float(sc.voxel_size)
    g.shift[:] = [float(x) for x in sc.shift]
    g.truncation = float(sc.truncation)
    return g


_engine_lib = {}


def engine_lib(dev: bool = False) -> C.CDLL:
    """dlopen the HIP engine; raises (no fallback) if it has not been built.  dev: the development build with the fault-injection knobs (tests / tools)."""
    path = ENGINE_LIB_DEV if dev else ENGINE_LIB
    if path not in _engine_lib:
        if not os.path.exists(path):
            raise PsgsdfError(f"HIP engine {path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _engine_lib[path] = C.CDLL(path)
    return _engine_lib[path]


def load_engine(sc_or_grid, K, settings: Settings, device: int = 0, dev: bool = False) -> Api:
    grid = sc_or_grid if isinstance(sc_or_grid, GridDesc) else grid_of(sc_or_grid)
    return Api(engine_lib(dev or os.environ.get("PSGSDF_USE_DEV_LIB") == "1"), "psgsdf_", grid, K, settings, device)
