// extract_query.hip -- the C ABI of include/psgsdf_query.h: the field at the caller's points, their projections onto the surface and the caller's
// rays (kernels: query.hip; DESIGN.md 22 "Field queries").  The caller's arrays go to the device whole, the results come back through the
// extraction calls' one download path into the XO_QUERY_* slots, which the three calls share: a result is valid until the next extraction call.
#include "extract_internal.h"
#include "../../include/psgsdf_query.h"
#include "query.h"

using namespace psge;

namespace {
psg::QueryField query_field(const psgsdf_ctx* c) {
    psg::QueryField f{};
    f.dist = c->dense.dist; f.weight = c->dense.weight;
    for (int a = 0; a < 3; ++a) { f.g[a] = c->dense.g[a]; f.rho[a] = c->dense.rho[a]; f.dim[a] = c->grid.dim[a]; }
    f.vs = (double)c->grid.vs;
    return f;
}
bool bad_model(int32_t model) { return model != PSGSDF_Q_CELL && model != PSGSDF_Q_TRILINEAR; }
// n x 3 floats of the caller's on the device
int query_upload(psgsdf_ctx* c, DevMem& mem, const char* me, const float* host, int64_t n, const float** dev) {
    float* d = nullptr;
    if (!mem.get(&d, 3 * (size_t)n)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, (long long)n);
    if (hipMemcpyAsync(d, host, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    *dev = d;
    return PSGSDF_OK;
}
// the zeroed counts of a call on the device, and back
int query_counts_new(psgsdf_ctx* c, DevMem& mem, const char* me, int k, unsigned long long** counts) {
    if (!mem.get(counts, (size_t)k)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me);
    if (hipMemsetAsync(*counts, 0, sizeof(unsigned long long) * (size_t)k, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    return PSGSDF_OK;
}
// Every call below copies its counts asynchronously into an array on its stack (`cnt`) and reads them only after download(), which waits for the
// stream; on an early return the call's DevMem waits for it before the array goes out of scope.  Reading `cnt` before download() returns is a bug.
}  // namespace

extern "C" int psgsdf_query_points(psgsdf_ctx* c, const float* xyz, int64_t n, int32_t model, const uint8_t** status, const float** dist, const float** normal,
                                   const float** rgb, const float** weight, const int64_t** voxel, psgsdf_query_counts* counts) {
    const char* me = "query_points";
    if (!status || !dist || !normal || !rgb || !weight || !voxel || !counts || (n > 0 && !xyz)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own planes of the volume")) return rc;
    if (bad_model(model)) return fail(c, PSGSDF_ERR_ARG, "%s: model %d (0 cell, 1 trilinear)", me, model);
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld points", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    auto clear = [&] { *status = nullptr; *dist = nullptr; *normal = nullptr; *rgb = nullptr; *weight = nullptr; *voxel = nullptr; *counts = psgsdf_query_counts{}; };
    clear();
    if (n == 0) return PSGSDF_OK;
    DevMem mem(c);
    psg::QueryArgs a{};
    a.f = query_field(c); a.n = (long long)n;
    if (int rc = query_upload(c, mem, me, xyz, n, &a.pts)) return rc;
    if (int rc = query_counts_new(c, mem, me, psg::kQueryCounts, &a.counts)) return rc;
    const size_t N = (size_t)n;
    if (!mem.get(&a.status, N) || !mem.get(&a.dist, N) || !mem.get(&a.normal, 3 * N) || !mem.get(&a.rgb, 3 * N) || !mem.get(&a.weight, N) || !mem.get(&a.voxel, N))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld points)", me, (long long)n);
    hipError_t launched = hipSuccess;
    timed(c, "k_query_points", [&] { launched = psg::launch_query_points(a, model, c->knob.query_chunk, c->stream); });
    if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld points: %s", me, (long long)n, hipGetErrorString(launched));
    unsigned long long cnt[psg::kQueryCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the counts", me);
    if (int rc = download(c, me, {{XO_QUERY_STATUS, a.status, N, status}, {XO_QUERY_DIST, a.dist, sizeof(float) * N, dist}, {XO_QUERY_NORMAL, a.normal, sizeof(float) * 3 * N, normal},
                                  {XO_QUERY_RGB, a.rgb, sizeof(float) * 3 * N, rgb}, {XO_QUERY_WEIGHT, a.weight, sizeof(float) * N, weight},
                                  {XO_QUERY_VOXEL, a.voxel, sizeof(int64_t) * N, voxel}})) { clear(); return rc; }
    counts->n = n; counts->n_ok = (int64_t)cnt[psg::QC_OK]; counts->n_outside = (int64_t)cnt[psg::QC_OUTSIDE];
    counts->n_unobserved = (int64_t)cnt[psg::QC_UNOBSERVED]; counts->n_invalid = (int64_t)cnt[psg::QC_INVALID];
    return PSGSDF_OK;
}

extern "C" int psgsdf_project_points(psgsdf_ctx* c, const float* xyz, int64_t n, const psgsdf_project_params* p, const uint8_t** status, const float** out_xyz,
                                     const float** residual, const float** normal, const int64_t** voxel, const uint8_t** iterations, const float** distance,
                                     psgsdf_project_counts* counts) {
    const char* me = "project_points";
    if (!p || !status || !out_xyz || !residual || !normal || !voxel || !iterations || !distance || !counts || (n > 0 && !xyz)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own planes of the volume")) return rc;
    if (bad_model(p->model)) return fail(c, PSGSDF_ERR_ARG, "%s: model %d (0 cell, 1 trilinear)", me, p->model);
    if (p->max_iters < 1 || p->max_iters > 64) return fail(c, PSGSDF_ERR_ARG, "%s: max_iters %d (1 .. 64)", me, p->max_iters);
    if (!(p->tol >= 0.0) || std::isinf(p->tol)) return fail(c, PSGSDF_ERR_ARG, "%s: tol must be a finite length >= 0", me);
    if (!(p->reserved == 0.0)) return fail(c, PSGSDF_ERR_ARG, "%s: reserved must be 0", me);
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld points", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    auto clear = [&] { *status = nullptr; *out_xyz = nullptr; *residual = nullptr; *normal = nullptr; *voxel = nullptr; *iterations = nullptr; *distance = nullptr; *counts = psgsdf_project_counts{}; };
    clear();
    if (n == 0) return PSGSDF_OK;
    DevMem mem(c);
    psg::QueryArgs a{};
    a.f = query_field(c); a.n = (long long)n; a.max_iters = p->max_iters; a.tol = p->tol;
    if (int rc = query_upload(c, mem, me, xyz, n, &a.pts)) return rc;
    if (int rc = query_counts_new(c, mem, me, psg::kQueryCounts, &a.counts)) return rc;
    const size_t N = (size_t)n;
    if (!mem.get(&a.status, N) || !mem.get(&a.xyz, 3 * N) || !mem.get(&a.dist, N) || !mem.get(&a.normal, 3 * N) || !mem.get(&a.voxel, N) || !mem.get(&a.iters, N) || !mem.get(&a.moved, N))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld points)", me, (long long)n);
    hipError_t launched = hipSuccess;
    timed(c, "k_query_project", [&] { launched = psg::launch_query_project(a, p->model, c->knob.query_chunk, c->stream); });
    if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld points: %s", me, (long long)n, hipGetErrorString(launched));
    unsigned long long cnt[psg::kQueryCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the counts", me);
    if (int rc = download(c, me, {{XO_QUERY_STATUS, a.status, N, status}, {XO_QUERY_XYZ, a.xyz, sizeof(float) * 3 * N, out_xyz}, {XO_QUERY_DIST, a.dist, sizeof(float) * N, residual},
                                  {XO_QUERY_NORMAL, a.normal, sizeof(float) * 3 * N, normal}, {XO_QUERY_VOXEL, a.voxel, sizeof(int64_t) * N, voxel},
                                  {XO_QUERY_ITERS, a.iters, N, iterations}, {XO_QUERY_MOVED, a.moved, sizeof(float) * N, distance}})) { clear(); return rc; }
    counts->n = n; counts->n_converged = (int64_t)cnt[psg::QC_OK]; counts->n_left = (int64_t)(cnt[psg::QC_OUTSIDE] + cnt[psg::QC_UNOBSERVED]);
    counts->n_not_converged = (int64_t)cnt[psg::QC_NOT_CONVERGED]; counts->n_invalid = (int64_t)cnt[psg::QC_INVALID];
    return PSGSDF_OK;
}

extern "C" int psgsdf_cast_rays(psgsdf_ctx* c, const float* origins, const float* directions, int64_t n, const psgsdf_ray_params* p, const uint8_t** status, const float** t,
                                const float** xyz, const float** normal, const float** rgb, const int64_t** voxel, psgsdf_ray_counts* counts) {
    const char* me = "cast_rays";
    if (!p || !status || !t || !xyz || !normal || !rgb || !voxel || !counts || (n > 0 && (!origins || !directions))) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own planes of the volume")) return rc;
    if (!(p->t_min >= 0.0) || std::isinf(p->t_min)) return fail(c, PSGSDF_ERR_ARG, "%s: t_min must be finite and >= 0", me);
    if (!(p->t_max > p->t_min)) return fail(c, PSGSDF_ERR_ARG, "%s: t_max must be > t_min", me);
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld rays", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    auto clear = [&] { *status = nullptr; *t = nullptr; *xyz = nullptr; *normal = nullptr; *rgb = nullptr; *voxel = nullptr; *counts = psgsdf_ray_counts{}; };
    clear();
    if (n == 0) return PSGSDF_OK;
    DevMem mem(c);
    psg::QueryRayArgs a{};
    { RenderArgs ra; int rc = render_prepare(c, mem, ra, me); if (rc) return rc; a.r = ra; }
    a.n = (long long)n; a.t_min = p->t_min; a.span = p->t_max - p->t_min; a.vs = (double)c->grid.vs;
    a.t_cut = a.span >= (double)FLT_MAX ? FLT_MAX : (float)a.span;      // (an infinite t_max: no cut)
    if (int rc = query_upload(c, mem, me, origins, n, &a.org)) return rc;
    if (int rc = query_upload(c, mem, me, directions, n, &a.dir)) return rc;
    if (int rc = query_counts_new(c, mem, me, psg::kQueryRayCounts, &a.counts)) return rc;
    const size_t N = (size_t)n;
    if (!mem.get(&a.status, N) || !mem.get(&a.t, N) || !mem.get(&a.xyz, 3 * N) || !mem.get(&a.normal, 3 * N) || !mem.get(&a.rgb, 3 * N) || !mem.get(&a.voxel, N))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld rays)", me, (long long)n);
    hipError_t launched = hipSuccess;
    timed(c, "k_query_rays", [&] { launched = psg::launch_query_rays(a, c->knob.query_chunk, c->stream); });
    if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld rays: %s", me, (long long)n, hipGetErrorString(launched));
    unsigned long long cnt[psg::kQueryRayCounts] = {};
    if (hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the counts", me);
    if (int rc = download(c, me, {{XO_QUERY_STATUS, a.status, N, status}, {XO_QUERY_DIST, a.t, sizeof(float) * N, t}, {XO_QUERY_XYZ, a.xyz, sizeof(float) * 3 * N, xyz},
                                  {XO_QUERY_NORMAL, a.normal, sizeof(float) * 3 * N, normal}, {XO_QUERY_RGB, a.rgb, sizeof(float) * 3 * N, rgb},
                                  {XO_QUERY_VOXEL, a.voxel, sizeof(int64_t) * N, voxel}})) { clear(); return rc; }
    counts->n = n; counts->n_valid = (int64_t)cnt[psg::QR_VALID]; counts->n_hits = (int64_t)cnt[psg::QR_HITS]; counts->n_buried = (int64_t)cnt[psg::QR_BURIED];
    return PSGSDF_OK;
}
