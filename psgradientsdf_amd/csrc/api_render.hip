// api_render.hip -- the C ABI of include/psgsdf_render.h: one view (psgsdf_render) or the stats of every keyframe in one pass
// (psgsdf_render_report).  Kernels: render.hip.
#include "engine_internal.h"
#include "../../include/psgsdf_render.h"

using namespace psge;

namespace {

// per-call device memory: brick map, bbox, planes, partials, folded sums (freed on every exit path)
struct RenderMem {
    std::vector<void*> p;
    ~RenderMem() { for (void* q : p) hipFree(q); }
    template <class T> hipError_t get(T** out, size_t bytes) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes < 8 ? 8 : bytes);
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
};

int render_ready(psgsdf_ctx* c, const char* what) {
    if (!c) return PSGSDF_ERR_ARG;
    if (c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: a multi-rank context holds a slab of the volume only", what);
    if (!c->inited || !c->have_frames) return fail(c, PSGSDF_ERR_STATE, "%s: init first", what);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->deferred.empty() || c->pending_fold.n) { int rc = flush(c); if (rc) return rc; }
    launch_band_scatter(c->dense, c->band, c->stream);      // the band's state back into the dense planes (as psgsdf_extract_mesh does)
    return 0;
}

// everything but the view: dense planes, band state, frames, images, the brick map of this call
int render_args(psgsdf_ctx* c, RenderMem& m, RenderArgs& a) {
    a = RenderArgs{};
    a.d = c->dense;
    for (int k = 0; k < 3; ++k) a.vp[k] = c->band.vp[k];
    a.grid = c->grid;
    a.frames = c->frames;
    a.im.f32 = c->img; a.im.u8 = c->img8; a.im.scale = c->img_scale;
    a.img_w = c->cam.W; a.img_h = c->cam.H;
    a.rob.loss = c->set.loss; a.rob.lambda = c->set.lambda; a.rob.lambda_sq = c->set.lambda * c->set.lambda; a.rob.inv_lambda = 1.0f / c->set.lambda;
    for (int k = 0; k < 3; ++k) a.nb[k] = (c->grid.dim[k] + kRenderBrick - 1) / kRenderBrick;
    unsigned char* bricks = nullptr; int* bbox = nullptr;
    HIPCHK(c, m.get(&bricks, (size_t)a.nb[0] * a.nb[1] * a.nb[2]));
    HIPCHK(c, m.get(&bbox, 6 * sizeof(int)));
    HIPCHK(c, hipMemsetAsync(bbox, 0x7f, 6 * sizeof(int), c->stream));
    const float thr = (float)(0.5 * sqrt(3.0) * (double)c->grid.vs * (1.0 + 1e-3));
    timed(c, "k_render_bricks", [&] { launch_render_bricks(c->dense, c->grid, thr, bricks, bbox, c->stream); });
    a.bricks = bricks; a.bbox = bbox;
    return 0;
}

void fill_stats(const double* v, int64_t n_pixels, psgsdf_render_stats* st) {
    st->n_pixels = n_pixels;
    st->n_hits = (int64_t)v[0]; st->n_hits_off_band = (int64_t)v[1];
    for (int k = 0; k < 3; ++k) { st->sum_r2[k] = v[2 + k]; st->sum_abs_r[k] = v[5 + k]; }
    st->robust = v[8];
}

constexpr int kPlaneCh[RP_COUNT] = {1, 3, 3, 1, 3, 3, 1};

}  // namespace

extern "C" {

int psgsdf_render_size(psgsdf_ctx* c, const psgsdf_view* v, int32_t* width, int32_t* height) {
    if (!c || !v || !width || !height) return fail(c, PSGSDF_ERR_ARG, "render_size: null argument");
    if (v->frame >= 0) {
        if (!c->have_frames) return fail(c, PSGSDF_ERR_STATE, "render_size: no keyframes");
        if (v->frame >= c->F) return fail(c, PSGSDF_ERR_ARG, "render_size: keyframe %d of %d", v->frame, c->F);
        *width = c->cam.W; *height = c->cam.H;
    } else { *width = v->width; *height = v->height; }
    return PSGSDF_OK;
}

int psgsdf_render(psgsdf_ctx* c, const psgsdf_view* v, uint32_t channels, float* out_host, psgsdf_render_stats* st) {
    if (!c || !v) return fail(c, PSGSDF_ERR_ARG, "render: null argument");
    if (channels >> RP_COUNT) return fail(c, PSGSDF_ERR_ARG, "render: unknown channel bits 0x%x", channels);
    if (channels && !out_host) return fail(c, PSGSDF_ERR_ARG, "render: channels asked for and no output array");
    { int rc = render_ready(c, "render"); if (rc) return rc; }
    const bool key = v->frame >= 0;
    if (key && v->frame >= c->F) return fail(c, PSGSDF_ERR_ARG, "render: keyframe %d of %d", v->frame, c->F);
    if (!key) {
        if (v->light_frame < 0 || v->light_frame >= c->F) return fail(c, PSGSDF_ERR_ARG, "render: light_frame %d of %d", v->light_frame, c->F);
        if (v->width <= 0 || v->height <= 0 || (int64_t)v->width * v->height > ((int64_t)1 << 28)) return fail(c, PSGSDF_ERR_ARG, "render: view size %d x %d", v->width, v->height);
        if (!(v->fx != 0.f) || !(v->fy != 0.f)) return fail(c, PSGSDF_ERR_ARG, "render: zero focal length");
        if (channels & PSGSDF_R_RESIDUAL) return fail(c, PSGSDF_ERR_ARG, "render: a residual needs a keyframe view");
    }
    RenderMem m;
    RenderArgs a;
    { int rc = render_args(c, m, a); if (rc) return rc; }
    if (key) { a.cam = c->cam; a.frame = v->frame; a.light_frame = v->frame; }
    else {
        a.cam.fx = v->fx; a.cam.fy = v->fy; a.cam.cx = v->cx; a.cam.cy = v->cy; a.cam.W = v->width; a.cam.H = v->height;
        a.frame = -1; a.light_frame = v->light_frame;
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) a.pose.R[i * 3 + j] = v->pose[i * 4 + j]; a.pose.t[i] = v->pose[i * 4 + 3]; }
    }
    a.tiles_x = (a.cam.W + kRenderTile - 1) / kRenderTile; a.tiles_y = (a.cam.H + kRenderTile - 1) / kRenderTile;
    const int tiles = a.tiles_x * a.tiles_y;
    const size_t HW = (size_t)a.cam.W * a.cam.H;
    size_t nplanes = 0;
    for (int q = 0; q < RP_COUNT; ++q) if (channels & (1u << q)) nplanes += kPlaneCh[q];
    float* planes = nullptr; double* sums = nullptr;
    if (nplanes) {
        HIPCHK(c, m.get(&planes, sizeof(float) * nplanes * HW));
        size_t off = 0;
        for (int q = 0; q < RP_COUNT; ++q) if (channels & (1u << q)) { a.planes[q] = planes + off * HW; off += kPlaneCh[q]; }
    }
    HIPCHK(c, m.get(&a.part, sizeof(double) * kRenderStats * (size_t)tiles));
    HIPCHK(c, m.get(&sums, sizeof(double) * kRenderStats));
    timed(c, "k_render", [&] { launch_render(a, c->set.model, c->stream); });
    timed(c, "k_render_fold", [&] { launch_render_fold(a.part, tiles, 1, sums, c->stream); });
    HIPCHK(c, hipGetLastError());
    double v9[kRenderStats];
    HIPCHK(c, hipMemcpyAsync(v9, sums, sizeof(v9), hipMemcpyDeviceToHost, c->stream));
    if (nplanes) HIPCHK(c, hipMemcpyAsync(out_host, planes, sizeof(float) * nplanes * HW, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (st) fill_stats(v9, (int64_t)HW, st);
    return PSGSDF_OK;
}

int psgsdf_render_report(psgsdf_ctx* c, psgsdf_render_stats* per_keyframe) {
    if (!c || !per_keyframe) return fail(c, PSGSDF_ERR_ARG, "render_report: null argument");
    { int rc = render_ready(c, "render_report"); if (rc) return rc; }
    RenderMem m;
    RenderArgs a;
    { int rc = render_args(c, m, a); if (rc) return rc; }
    a.cam = c->cam; a.frame = -1; a.light_frame = 0;
    a.tiles_x = (a.cam.W + kRenderTile - 1) / kRenderTile; a.tiles_y = (a.cam.H + kRenderTile - 1) / kRenderTile;
    const int tiles = a.tiles_x * a.tiles_y;
    double* sums = nullptr;
    HIPCHK(c, m.get(&a.part, sizeof(double) * kRenderStats * (size_t)tiles * c->F));
    HIPCHK(c, m.get(&sums, sizeof(double) * kRenderStats * c->F));
    timed(c, "k_render_report", [&] { launch_render_report(a, c->set.model, c->F, c->stream); });
    timed(c, "k_render_fold", [&] { launch_render_fold(a.part, tiles, c->F, sums, c->stream); });
    HIPCHK(c, hipGetLastError());
    std::vector<double> h((size_t)kRenderStats * c->F);
    HIPCHK(c, hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < c->F; ++f) fill_stats(h.data() + (size_t)kRenderStats * f, (int64_t)c->cam.W * c->cam.H, per_keyframe + f);
    return PSGSDF_OK;
}

}  // extern "C"
