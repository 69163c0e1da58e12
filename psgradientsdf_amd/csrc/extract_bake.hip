// extract_bake.hip -- the C ABI of include/psgsdf_bake.h: detail maps of the level-of-detail mesh (kernel: bake.hip; DESIGN.md "Baked detail maps"),
// of include/psgsdf_occlusion.h: ambient occlusion at the caller's points and as a map of the bake (occlusion.hip; "Ambient occlusion"),
// and of include/psgsdf_photo.h: the bake's albedo solved again from the keyframes, per texel (photo.hip; "Photometric albedo texture").
// The texture coordinates and the direction table are computed on the host and compared bit for bit: no FMA contraction.
#pragma clang fp contract(off)
#include "mesh_stages.h"
#include "../../include/psgsdf_bake.h"
#include "../../include/psgsdf_occlusion.h"
#include "../../include/psgsdf_photo.h"
#include "bake.h"
#include "occlusion.h"
#include "photo.h"

using namespace psge;

// ---- the bake (kernel: bake.hip k_bake).  The clusters' device arrays are the kernel's mesh (lod_from_device hands them out: nothing is uploaded
// again), the brick map comes from the renderer's prepare path.
namespace psge {
// ---- stage 4 (mesh_stages.h)
int bake_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach) {
    if (int rc = lod_ready(c, me, filter, cell)) return rc;
    if (res < 1) return fail(c, PSGSDF_ERR_ARG, "%s: res %d (at least 1)", me, res);
    if (!(reach > 0.0) || std::isinf(reach)) return fail(c, PSGSDF_ERR_ARG, "%s: the reach must be a finite length > 0", me);
    return PSGSDF_OK;
}
// the bake of both calls, its results in their pinned host slots (the stream has been waited for); dev (if asked for): the kernel's arguments, the
// atlas's device planes among them (dev->nf == 0: an empty level-of-detail mesh, nothing was baked).  max_texels (if not 0): a larger atlas is refused
// like one beyond 16384, before it is allocated
int bake_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out, psg::BakeArgs* dev,
                long long max_texels) {
    *out = psgsdf_bake{};
    MeshView lod;
    if (int rc = lod_stages(c, mem, me, filter, cell, LodOut{&out->xyz, &out->normals, &out->rgb, &out->n_vertices, &out->faces, &out->n_faces, &out->vertex_map,
                                                            &out->n_vertices_in, &out->n_faces_in}, &lod)) { *out = psgsdf_bake{}; return rc; }
    if (lod.nf <= 0) return PSGSDF_OK;      // an empty level-of-detail mesh: all sizes 0
    auto give_up = [&](int code, const char* what) { *out = psgsdf_bake{}; return fail(c, code, "%s: %s (%d faces, res %d)", me, what, lod.nf, res); };
    // the atlas: two faces per block of (R + 1)^2 texels, the blocks in a near-square grid
    psg::BakeArgs a{};
    const long long B = (long long)res + 1, nblk = ((long long)lod.nf + 1) / 2;
    long long bpr = (long long)sqrt((double)nblk);
    while (bpr * bpr < nblk) ++bpr;
    while (bpr > 1 && (bpr - 1) * (bpr - 1) >= nblk) --bpr;
    const long long W = bpr * B, H = (nblk + bpr - 1) / bpr * B;
    if (W > psg::kBakeMaxSide || H > psg::kBakeMaxSide) return give_up(PSGSDF_ERR_UNSUPPORTED, "the atlas would be larger than 16384 texels along a side");
    if (max_texels && W * H > max_texels) return give_up(PSGSDF_ERR_UNSUPPORTED, "the atlas has more texels than the call's per-keyframe status plane may hold (2^30 bytes in all)");
    { RenderArgs ra; int rc = render_prepare(c, mem, ra, me); if (rc) { *out = psgsdf_bake{}; return rc; } a.r = ra; }
    a.has_band = c->inited ? 1 : 0;
    a.xyz = lod.xyz; a.nrm = lod.nrm; a.rgb = lod.rgb; a.faces = lod.faces; a.nf = lod.nf;
    a.res = res; a.bpr = (int)bpr; a.nblk = (int)nblk; a.W = (int)W; a.H = (int)H;
    a.reach = reach; a.vs = (double)c->grid.vs;
    const size_t px = (size_t)W * (size_t)H;
    if (!mem.get(&a.albedo, 3 * px) || !mem.get(&a.normal, 3 * px) || !mem.get(&a.disp, px) || !mem.get(&a.voxel, px) || !mem.get(&a.face, px) || !mem.get(&a.counts, (size_t)psg::kBakeCounts))
        return give_up(PSGSDF_ERR_DEVICE, "out of memory");
    if (hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * psg::kBakeCounts, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "memset");
    timed(c, "bake", [&] { psg::launch_bake(a, c->stream); });
    // the texture coordinates: integers over 6 W / 6 H, one division each
    void* hu = nullptr;
    if (int rc = host_out(c, XO_BAKE_UV, sizeof(float) * 6 * (size_t)lod.nf, &hu)) { *out = psgsdf_bake{}; return rc; }
    float* uv = (float*)hu;
    const long long R6 = 6 * (long long)res;
    for (long long f = 0; f < lod.nf; ++f) {
        const long long q = f >> 1, x0 = 6 * (q % bpr) * B, y0 = 6 * (q / bpr) * B;
        const long long even[3][2] = {{1, 1}, {R6 + 7, 1}, {1, R6 + 7}}, odd[3][2] = {{R6 + 5, R6 + 5}, {-1, R6 + 5}, {R6 + 5, -1}};
        for (int k = 0; k < 3; ++k) {
            const long long* m = (f & 1) ? odd[k] : even[k];
            uv[6 * f + 2 * k] = (float)((double)(x0 + m[0]) / (double)(6 * W));
            uv[6 * f + 2 * k + 1] = (float)((double)(y0 + m[1]) / (double)(6 * H));
        }
    }
    unsigned long long cnt[psg::kBakeCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "download of the counts");
    if (int rc = download(c, me, {{XO_BAKE_ALBEDO, a.albedo, 3 * px, &out->albedo}, {XO_BAKE_NORMAL, a.normal, sizeof(float) * 3 * px, &out->normal},
                                  {XO_BAKE_DISPLACEMENT, a.disp, sizeof(float) * px, &out->displacement}, {XO_BAKE_VOXEL, a.voxel, sizeof(int) * px, &out->voxel},
                                  {XO_BAKE_FACE, a.face, sizeof(int) * px, &out->face}})) { *out = psgsdf_bake{}; return rc; }
    out->uv = uv; out->width = (int32_t)W; out->height = (int32_t)H;
    out->n_texels = (int64_t)cnt[psg::BK_OWNED]; out->n_hits = (int64_t)cnt[psg::BK_HITS]; out->n_hits_off_band = (int64_t)cnt[psg::BK_OFF_BAND]; out->n_buried = (int64_t)cnt[psg::BK_BURIED];
    out->n_misses = out->n_texels - out->n_hits - out->n_buried;
    if (dev) *dev = a;
    return PSGSDF_OK;
}
}  // namespace psge

namespace {
// ---- ambient occlusion (kernel: occlusion.hip k_occlusion): K short rays per sample through the renderer's walk, the
// samples either the caller's points or the texels of a bake, whose planes are still on the device when the rays start from them.
int ao_bad_params(psgsdf_ctx* c, const char* me, const psgsdf_ao_params* p) {
    if (!p) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if ((p->n_dirs != 8 && p->n_dirs != 16 && p->n_dirs != 32 && p->n_dirs != 64) || p->reserved != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: n_dirs %d, reserved %d (8, 16, 32 or 64 directions; reserved 0)", me, p->n_dirs, p->reserved);
    if (!(p->radius > 0.0) || std::isinf(p->radius) || !(p->bias > 0.0) || std::isinf(p->bias)) return fail(c, PSGSDF_ERR_ARG, "%s: radius and bias must be finite lengths > 0", me);
    return PSGSDF_OK;
}
// the direction table into its pinned slot (the definition's arithmetic, in double)
int ao_dirs(psgsdf_ctx* c, int K, const double** dirs) {
    void* h = nullptr;
    if (int rc = host_out(c, XO_AO_DIRS, sizeof(double) * 3 * (size_t)K, &h)) return rc;
    double* D = (double*)h;
    const double g = 0.6180339887498949, pi = 3.141592653589793;
    for (int i = 0; i < K; ++i) {
        const double u = ((double)i + 0.5) / (double)K, r = sqrt(u), z = sqrt(1.0 - u), phi = 2.0 * pi * ((double)i * g - floor((double)i * g));
        D[3 * i] = r * cos(phi); D[3 * i + 1] = r * sin(phi); D[3 * i + 2] = z;
    }
    *dirs = D;
    return PSGSDF_OK;
}
// the arguments both providers share (a.n and the provider's own arrays are set by the caller before): brick map, table, results, counts; launch; download
int ao_run(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_ao_params& p, const double* dirs_host, psg::OcclusionArgs& a, bool bake, XoSlot s_mask, XoSlot s_occ,
           const uint64_t** mask, const uint8_t** occlusion, psgsdf_ao_counts* counts) {
    const int K = p.n_dirs;
    a.K = K; a.log2K = K == 8 ? 3 : K == 16 ? 4 : K == 32 ? 5 : 6;
    a.radius = p.radius; a.bias = p.bias; a.vs = (double)c->grid.vs;
    a.t_max = (float)p.radius;      // rounded up if the conversion rounded down: no hit within the radius is cut off
    if ((double)a.t_max < p.radius) a.t_max = nextafterf(a.t_max, INFINITY);
    if (!c->knob.ao_cut) a.t_max = FLT_MAX;      // (PSGSDF_AO_CUT=0; tools/time_mesh.py: what the cut buys -- the same bits)
    double* d_dirs = nullptr;
    const size_t n = (size_t)a.n;
    if (!mem.get(&d_dirs, 3 * (size_t)K) || !mem.get(&a.mask, n) || !mem.get(&a.occ, n) || !mem.get(&a.counts, (size_t)psg::kAoCounts))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld samples)", me, a.n);
    a.dirs = d_dirs;
    if (hipMemcpyAsync(d_dirs, dirs_host, sizeof(double) * 3 * (size_t)K, hipMemcpyHostToDevice, c->stream) != hipSuccess
        || hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * psg::kAoCounts, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    hipError_t launched = hipSuccess;
    timed(c, "occlusion", [&] { launched = psg::launch_occlusion(a, bake, c->stream); });
    if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld rays: %s", me, a.n * K, hipGetErrorString(launched));
    unsigned long long cnt[psg::kAoCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the counts", me);
    if (int rc = download(c, me, {{s_mask, a.mask, sizeof(uint64_t) * n, mask}, {s_occ, a.occ, n, occlusion}})) return rc;
    counts->n_samples = (int64_t)cnt[psg::AO_SAMPLES]; counts->n_valid = (int64_t)cnt[psg::AO_VALID]; counts->n_rays = (int64_t)K * counts->n_valid;
    counts->n_occluded = (int64_t)cnt[psg::AO_OCCLUDED]; counts->n_buried = (int64_t)cnt[psg::AO_BURIED];
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_bake_lod(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out) {
    const char* me = "bake_lod";
    if (!out) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    DevMem mem(c);
    return bake_device(c, mem, me, filter, cell, res, reach, out);
}

extern "C" int psgsdf_occlusion_points(psgsdf_ctx* c, const float* xyz, const float* normals, int64_t n, const psgsdf_ao_params* params,
                                       const uint64_t** mask, const uint8_t** occlusion, const double** dirs, psgsdf_ao_counts* counts) {
    const char* me = "occlusion_points";
    if (!mask || !occlusion || !dirs || !counts || (n > 0 && (!xyz || !normals))) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own planes of the volume")) return rc;
    if (int rc = ao_bad_params(c, me, params)) return rc;
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld points", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *mask = nullptr; *occlusion = nullptr; *dirs = nullptr; *counts = psgsdf_ao_counts{};
    const double* D = nullptr;
    if (int rc = ao_dirs(c, params->n_dirs, &D)) return rc;
    if (n > 0) {
        DevMem mem(c);
        psg::OcclusionArgs a{};
        { RenderArgs ra; int rc = render_prepare(c, mem, ra, me); if (rc) return rc; a.r = ra; }
        a.n = (long long)n;
        float *d_xyz = nullptr, *d_nrm = nullptr;
        if (!mem.get(&d_xyz, 3 * (size_t)n) || !mem.get(&d_nrm, 3 * (size_t)n)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld points)", me, (long long)n);
        if (hipMemcpyAsync(d_xyz, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess
            || hipMemcpyAsync(d_nrm, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
        a.pts = d_xyz; a.pts_n = d_nrm;
        psgsdf_ao_counts cn{};
        if (int rc = ao_run(c, mem, me, *params, D, a, false, XO_AO_MASK, XO_AO_OCCLUSION, mask, occlusion, &cn)) { *mask = nullptr; *occlusion = nullptr; return rc; }
        *counts = cn;
    }
    *dirs = D;
    return PSGSDF_OK;
}

extern "C" int psgsdf_bake_lod_ao(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, const psgsdf_ao_params* params, psgsdf_bake_ao* out) {
    const char* me = "bake_lod_ao";
    if (!out) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    if (int rc = ao_bad_params(c, me, params)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_bake_ao{};
    DevMem mem(c);
    psg::BakeArgs b{};
    if (int rc = bake_device(c, mem, me, filter, cell, res, reach, &out->bake, &b)) return rc;
    const double* D = nullptr;
    if (int rc = ao_dirs(c, params->n_dirs, &D)) { *out = psgsdf_bake_ao{}; return rc; }
    out->n_dirs = params->n_dirs;
    if (b.nf > 0) {
        psg::OcclusionArgs a{};
        a.r = b.r; a.n = (long long)b.W * b.H;
        a.xyz = b.xyz; a.nrm = b.nrm; a.faces = b.faces; a.res = b.res; a.W = b.W;
        a.normal = b.normal; a.disp = b.disp; a.voxel = b.voxel; a.face = b.face;
        if (int rc = ao_run(c, mem, me, *params, D, a, true, XO_BAKE_AO_MASK, XO_BAKE_AO_OCCLUSION, &out->mask, &out->occlusion, &out->counts)) { *out = psgsdf_bake_ao{}; return rc; }
    }
    out->dirs = D;
    return PSGSDF_OK;
}

// ---- the albedo texture solved from the keyframes (kernels: photo.hip k_photo_pairs, k_photo_solve): the bake as above, its planes still on the
// device; then per pass one launch over the (texel, keyframe) pairs, whose status bytes go to the caller's plane or to a bounded scratch buffer,
// and one over the texels.
extern "C" int psgsdf_bake_lod_photo(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, const psgsdf_photo_params* p, psgsdf_bake_photo* out) {
    const char* me = "bake_lod_photo";
    if (!out || !p) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    if (!(p->bias > 0.0) || std::isinf(p->bias)) return fail(c, PSGSDF_ERR_ARG, "%s: the bias must be a finite length > 0", me);
    if (!(p->cos_min >= -1.0) || !(p->cos_min < 1.0)) return fail(c, PSGSDF_ERR_ARG, "%s: cos_min %g (-1 <= cos_min < 1)", me, p->cos_min);
    if (!(p->shade_min > 0.0) || std::isinf(p->shade_min)) return fail(c, PSGSDF_ERR_ARG, "%s: shade_min must be finite and > 0", me);
    if ((p->want_status != 0 && p->want_status != 1) || p->reserved != 0) return fail(c, PSGSDF_ERR_ARG, "%s: want_status %d, reserved %d (0 or 1; reserved 0)", me, p->want_status, p->reserved);
    if (!c || !c->inited || !c->have_frames) return fail(c, PSGSDF_ERR_STATE, "%s: init first (the keyframes, their poses and lights are read)", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_bake_photo{};
    DevMem mem(c);
    psg::BakeArgs b{};
    const bool keep = p->want_status != 0;      // the caller's status plane: at most kPhotoChunk bytes, refused before the atlas is allocated
    if (int rc = bake_device(c, mem, me, filter, cell, res, reach, &out->bake, &b, keep ? psg::kPhotoChunk / c->F : 0)) { *out = psgsdf_bake_photo{}; return rc; }
    out->n_frames = c->F;
    if (b.nf <= 0) return PSGSDF_OK;
    auto give_up = [&](int code, const char* what) { *out = psgsdf_bake_photo{}; return fail(c, code, "%s: %s (%d x %d texels, %d keyframes)", me, what, b.W, b.H, c->F); };
    psg::PhotoArgs a{};
    a.n = (long long)b.W * b.H;
    const SweepArgs e = make_args(c, 0);      // the energy's own view of the keyframes
    a.r = b.r; a.im = e.im; a.cam = e.cam; a.rob = e.rob; a.F = e.F; a.model = e.model;
    a.bias = p->bias; a.cos_min = p->cos_min; a.shade_min = (float)p->shade_min; a.vs = (double)c->grid.vs;
    for (int k = 0; k < 3; ++k) a.origin[k] = (double)c->grid.origin[k];
    a.xyz = b.xyz; a.nrm = b.nrm; a.faces = b.faces; a.res = b.res; a.W = b.W;
    a.albedo = b.albedo; a.normal = b.normal; a.disp = b.disp; a.voxel = b.voxel; a.face = b.face;
    a.scratch = !keep; a.stride = a.n; a.base = 0;
    const size_t n = (size_t)a.n, n_status = (size_t)c->F * (size_t)psg::photo_pass_texels(a.n, c->F, a.scratch);
    if (!mem.get(&a.photo, 3 * n) || !mem.get(&a.photo_rgb, 3 * n) || !mem.get(&a.n_obs, n) || !mem.get(&a.status, n_status) || !mem.get(&a.counts, (size_t)psg::kPhotoCounts))
        return give_up(PSGSDF_ERR_DEVICE, "out of memory");
    if (hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * psg::kPhotoCounts, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "memset");
    hipError_t launched = hipSuccess;
    for (long long j0 = 0; j0 < a.n && launched == hipSuccess; j0 += psg::photo_pass_texels(a.n, a.F, a.scratch)) {
        psg::photo_pass(a, j0);
        timed(c, "k_photo_pairs", [&] { launched = psg::launch_photo_pairs(a, c->stream); });
        if (launched == hipSuccess) timed(c, "k_photo_solve", [&] { launched = psg::launch_photo_solve(a, c->stream); });
    }
    if (launched != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, hipGetErrorString(launched));
    unsigned long long cnt[psg::kPhotoCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "download of the counts");
    if (int rc = download(c, me, {{XO_PHOTO, a.photo, sizeof(float) * 3 * n, &out->photo}, {XO_PHOTO_RGB, a.photo_rgb, 3 * n, &out->photo_rgb},
                                  {XO_PHOTO_NOBS, a.n_obs, sizeof(int) * n, &out->n_obs}, {XO_PHOTO_STATUS, a.status, keep ? n_status : 0, &out->status}})) { *out = psgsdf_bake_photo{}; return rc; }
    psgsdf_photo_counts& k = out->counts;
    k.n_samples = (int64_t)cnt[psg::PH_SAMPLES]; k.n_pairs = k.n_samples * c->F; k.n_used = (int64_t)cnt[psg::PH_USED]; k.n_outside = (int64_t)cnt[psg::PH_OUTSIDE];
    k.n_grazing = (int64_t)cnt[psg::PH_GRAZING]; k.n_occluded = (int64_t)cnt[psg::PH_OCCLUDED]; k.n_buried = (int64_t)cnt[psg::PH_BURIED]; k.n_dark = (int64_t)cnt[psg::PH_DARK];
    k.n_texels_solved = (int64_t)cnt[psg::PH_SOLVED];
    return PSGSDF_OK;
}
