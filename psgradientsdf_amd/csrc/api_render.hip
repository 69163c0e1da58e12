// api_render.hip -- the C ABI of include/psgsdf_render.h: one view (psgsdf_render) or the stats of every keyframe in one pass
// (psgsdf_render_report).  Kernels: render.hip.
// On a multi-rank context both are collective calls ("Multi-rank contexts"): every rank traces its own slab, and three sum all-reduces over the
// context's communicator (brick marks + the call's checksum, per-pixel hit masks, the winners' records) give every rank the single-rank result.
#include "extract_internal.h"
#include "../../include/psgsdf_render.h"

using namespace psge;

namespace {

int oom(psgsdf_ctx* c) { return fail(c, PSGSDF_ERR_DEVICE, "render: out of device memory"); }
constexpr size_t kRenderChunkBytes = (size_t)256 << 20;     // multi-rank report: per-pixel exchange buffers of one chunk of keyframes

int render_ready(psgsdf_ctx* c, const char* what) {
    if (!c) return PSGSDF_ERR_ARG;
    if (!c->inited || !c->have_frames) return fail(c, PSGSDF_ERR_STATE, "%s: init first", what);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->deferred.empty() || c->pending_fold.n) { int rc = flush(c); if (rc) return rc; }
    launch_band_scatter(c->dense, c->band, c->stream);      // the band's state back into the dense planes (as psgsdf_extract_mesh does)
    return 0;
}

// the checksum every rank puts into the first exchange: a 32-bit FNV-1a over what decides the call (exact in a double; -1: this rank's arguments were refused)
struct CallHash {
    uint32_t h = 2166136261u;
    template <class T> CallHash& add(const T& v) { const unsigned char* b = (const unsigned char*)&v; for (size_t i = 0; i < sizeof(T); ++i) { h ^= b[i]; h *= 16777619u; } return *this; }
};
double view_hash(const psgsdf_view* v, uint32_t channels) {
    CallHash k; k.add(1).add(channels).add(v->frame);
    if (v->frame < 0) { for (int i = 0; i < 16; ++i) k.add(v->pose[i]); k.add(v->fx).add(v->fy).add(v->cx).add(v->cy).add(v->width).add(v->height).add(v->light_frame); }
    return (double)k.h;
}

// all-reduce of n doubles in pieces the transports take (int counts)
int allreduce_big(psgsdf_ctx* c, double* buf, size_t n) {
    constexpr size_t kPiece = (size_t)1 << 28;
    for (size_t o = 0; o < n; o += kPiece) { int rc = comm_allreduce(c, buf + o, (int)std::min(kPiece, n - o)); if (rc) return rc; }
    return 0;
}

// everything but the view: dense planes, band state, frames, images, the brick map of this call.
// Multi-rank: each rank marks the bricks of the planes it owns (global brick coordinates); the first exchange sums the marks together with every
// rank's z0 (-> this rank's place in the z order, a.slab) and checksum `tag` of the call; the map and box then come from the merged marks.
// err_local: this rank's own argument error (reported once the exchange shows every rank that the call failed).
int render_args(psgsdf_ctx* c, DevMem& m, RenderArgs& a, double tag, const char* what, const char* err_local) {
    a = RenderArgs{};
    a.d = c->dense;
    for (int k = 0; k < 3; ++k) a.vp[k] = c->band.vp[k];
    a.grid = c->grid;
    a.grid.dim[2] = c->gdim[2];
    a.frames = c->frames;
    a.im.f32 = c->img; a.im.u8 = c->img8; a.im.scale = c->img_scale;
    a.img_w = c->cam.W; a.img_h = c->cam.H;
    a.rob.loss = c->set.loss; a.rob.lambda = c->set.lambda; a.rob.lambda_sq = c->set.lambda * c->set.lambda; a.rob.inv_lambda = 1.0f / c->set.lambda;
    for (int k = 0; k < 3; ++k) a.nb[k] = (a.grid.dim[k] + kRenderBrick - 1) / kRenderBrick;
    const size_t nbr = (size_t)a.nb[0] * a.nb[1] * a.nb[2];
    unsigned char* bricks = nullptr; int* bbox = nullptr;
    if (!m.get(&bricks, nbr)) return oom(c);
    if (!m.get(&bbox, 6)) return oom(c);
    HIPCHK(c, hipMemsetAsync(bbox, 0x7f, 6 * sizeof(int), c->stream));
    const float thr = (float)(0.5 * sqrt(3.0) * (double)c->grid.vs * (1.0 + 1e-3));
    a.bricks = bricks; a.bbox = bbox;
    a.zr[0] = c->z0; a.zr[1] = c->z1;
    if (c->n_ranks <= 1) {
        a.zr[0] = 0; a.zr[1] = a.grid.dim[2];
        timed(c, "k_render_bricks", [&] { launch_render_bricks(c->dense, a.grid, thr, 0, a.grid.dim[2], bricks, bbox, nullptr, c->stream); });
        return 0;
    }
    const int R = c->n_ranks;
    double* marks = nullptr;
    if (!m.get(&marks, nbr + 2 * R)) return oom(c);
    timed(c, "k_render_bricks", [&] { launch_render_bricks(c->dense, a.grid, thr, c->z0, c->z1, nullptr, nullptr, marks, c->stream); });
    std::vector<double> tail(2 * R, 0.0);
    tail[c->rank] = (double)c->z0; tail[R + c->rank] = err_local ? -1.0 : tag;
    HIPCHK(c, hipMemcpyAsync(marks + nbr, tail.data(), sizeof(double) * tail.size(), hipMemcpyHostToDevice, c->stream));
    { int rc = allreduce_big(c, marks, nbr + 2 * R); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(tail.data(), marks + nbr, sizeof(double) * tail.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err_local) return fail(c, PSGSDF_ERR_ARG, "%s", err_local);
    for (int r = 0; r < R; ++r)
        if (tail[R + r] != tag) return fail(c, PSGSDF_ERR_ARG, "%s: rank %d made another call (a collective call: the same view on every rank)", what, r);
    a.slab = 0;
    for (int r = 0; r < R; ++r) if (tail[r] < (double)c->z0) ++a.slab;
    timed(c, "k_render_box", [&] { launch_render_box(marks, a.nb, bricks, bbox, c->stream); });
    return 0;
}

void fill_stats(const double* v, int64_t n_pixels, psgsdf_render_stats* st) {
    st->n_pixels = n_pixels;
    st->n_hits = (int64_t)v[0]; st->n_hits_off_band = (int64_t)v[1];
    for (int k = 0; k < 3; ++k) { st->sum_r2[k] = v[2 + k]; st->sum_abs_r[k] = v[5 + k]; }
    st->robust = v[8];
}

constexpr int kPlaneCh[RP_COUNT] = {1, 3, 3, 1, 3, 3, 1};

// multi-rank: the record fields a call carries (stats: the off-band flag always, the rendered colour whenever there is a residual)
void carry_fields(RenderArgs& a, uint32_t channels, bool key) {
    for (int q = 0; q < RF_COUNT; ++q) a.rf[q] = -1;
    a.n_rf = 0;
    auto carry = [&](int q0, int n) { for (int q = q0; q < q0 + n; ++q) a.rf[q] = a.n_rf++; };
    if (channels & PSGSDF_R_DEPTH) carry(RF_DEPTH, 1);
    if (channels & PSGSDF_R_NORMAL) carry(RF_NORMAL, 3);
    if (channels & PSGSDF_R_ALBEDO) carry(RF_ALBEDO, 3);
    if (channels & PSGSDF_R_SHADING) carry(RF_SHADING, 1);
    if (key || (channels & (PSGSDF_R_RENDERED | PSGSDF_R_RESIDUAL))) carry(RF_RENDERED, 3);
    if (channels & PSGSDF_R_VOXEL) carry(RF_VOXEL, 1);
    carry(RF_OFF_BAND, 1);
}

// multi-rank: records of `chunk` views (a.f0 .. for the report), mask exchange, non-winners' records zeroed, record exchange, composite
int render_ranks_pass(psgsdf_ctx* c, RenderArgs& a, bool report, int chunk) {
    const size_t npx = (size_t)a.rec_px;
    timed(c, "k_render_ranks", [&] { launch_render_ranks(a, c->set.model, report, chunk, c->stream); });
    { int rc = allreduce_big(c, a.mask, npx); if (rc) return rc; }
    timed(c, "k_render_keep", [&] { launch_render_keep(a, c->stream); });
    { int rc = allreduce_big(c, a.rec, npx * a.n_rf); if (rc) return rc; }
    timed(c, "k_render_composite", [&] { launch_render_composite(a, report, chunk, c->stream); });
    return 0;
}

}  // namespace

namespace psge {
int render_prepare(psgsdf_ctx* c, DevMem& m, RenderArgs& a, const char* what) { return render_args(c, m, a, 0.0, what, nullptr); }
}  // namespace psge

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
    const bool mr = c->n_ranks > 1;
    // the argument checks: on one rank the first failure returns; on a multi-rank context it is carried into the first exchange, so that every
    // rank returns PSGSDF_ERR_ARG (and none waits for a rank that left)
    char err[256] = {0};
    auto bad = [&](const char* msg) { if (!err[0]) snprintf(err, sizeof(err), "%s", msg); };
    char msg[160];
    if (channels >> RP_COUNT) { snprintf(msg, sizeof(msg), "render: unknown channel bits 0x%x", channels); bad(msg); }
    if (channels && !out_host) bad("render: channels asked for and no output array");
    if (err[0] && !mr) return fail(c, PSGSDF_ERR_ARG, "%s", err);
    { int rc = render_ready(c, "render"); if (rc) return rc; }
    const bool key = v->frame >= 0;
    if (key && v->frame >= c->F) { snprintf(msg, sizeof(msg), "render: keyframe %d of %d", v->frame, c->F); bad(msg); }
    if (!key) {
        if (v->light_frame < 0 || v->light_frame >= c->F) { snprintf(msg, sizeof(msg), "render: light_frame %d of %d", v->light_frame, c->F); bad(msg); }
        if (v->width <= 0 || v->height <= 0 || (int64_t)v->width * v->height > ((int64_t)1 << 28)) { snprintf(msg, sizeof(msg), "render: view size %d x %d", v->width, v->height); bad(msg); }
        if (!(v->fx != 0.f) || !(v->fy != 0.f)) bad("render: zero focal length");
        if (channels & PSGSDF_R_RESIDUAL) bad("render: a residual needs a keyframe view");
    }
    if (err[0] && !mr) return fail(c, PSGSDF_ERR_ARG, "%s", err);
    DevMem m;      // per-call device memory: brick map, bbox, planes, partials, folded sums
    RenderArgs a;
    { int rc = render_args(c, m, a, view_hash(v, channels), "render", err[0] ? err : nullptr); if (rc) return rc; }
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
        if (!m.get(&planes, nplanes * HW)) return oom(c);
        size_t off = 0;
        for (int q = 0; q < RP_COUNT; ++q) if (channels & (1u << q)) { a.planes[q] = planes + off * HW; off += kPlaneCh[q]; }
    }
    if (!m.get(&a.part, kRenderStats * (size_t)tiles)) return oom(c);
    if (!m.get(&sums, kRenderStats)) return oom(c);
    if (mr) {
        carry_fields(a, channels, key);
        a.rec_px = (long long)HW;
        if (!m.get(&a.mask, HW)) return oom(c);
        if (!m.get(&a.mine, HW)) return oom(c);
        if (!m.get(&a.rec, HW * a.n_rf)) return oom(c);
        { int rc = render_ranks_pass(c, a, false, 1); if (rc) return rc; }
    } else timed(c, "k_render", [&] { launch_render(a, c->set.model, c->stream); });
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
    if (!c || (!per_keyframe && c->n_ranks <= 1)) return fail(c, PSGSDF_ERR_ARG, "render_report: null argument");
    { int rc = render_ready(c, "render_report"); if (rc) return rc; }
    DevMem m;      // per-call device memory: brick map, bbox, planes, partials, folded sums
    RenderArgs a;
    const double tag = (double)CallHash{}.add(2).h;
    { int rc = render_args(c, m, a, tag, "render_report", per_keyframe ? nullptr : "render_report: null argument"); if (rc) return rc; }
    a.cam = c->cam; a.frame = -1; a.light_frame = 0;
    a.tiles_x = (a.cam.W + kRenderTile - 1) / kRenderTile; a.tiles_y = (a.cam.H + kRenderTile - 1) / kRenderTile;
    const int tiles = a.tiles_x * a.tiles_y;
    double* sums = nullptr;
    if (!m.get(&a.part, kRenderStats * (size_t)tiles * c->F)) return oom(c);
    if (!m.get(&sums, kRenderStats * c->F)) return oom(c);
    if (c->n_ranks > 1) {
        // keyframes in chunks: mask, hit byte and records (rendered colour, off-band flag) of every pixel of a chunk within kRenderChunkBytes
        carry_fields(a, 0, true);
        const size_t HW = (size_t)a.cam.W * a.cam.H, per_frame = HW * (sizeof(double) * (1 + a.n_rf) + 1);
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->F, kRenderChunkBytes / per_frame));
        if (!m.get(&a.mask, HW * chunk)) return oom(c);
        if (!m.get(&a.mine, HW * chunk)) return oom(c);
        if (!m.get(&a.rec, HW * chunk * a.n_rf)) return oom(c);
        for (int f0 = 0; f0 < c->F; f0 += chunk) {
            const int n = std::min(chunk, c->F - f0);
            a.f0 = f0; a.rec_px = (long long)(HW * n);
            int rc = render_ranks_pass(c, a, true, n); if (rc) return rc;
        }
    } else timed(c, "k_render_report", [&] { launch_render_report(a, c->set.model, c->F, c->stream); });
    timed(c, "k_render_fold", [&] { launch_render_fold(a.part, tiles, c->F, sums, c->stream); });
    HIPCHK(c, hipGetLastError());
    std::vector<double> h((size_t)kRenderStats * c->F);
    HIPCHK(c, hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < c->F; ++f) fill_stats(h.data() + (size_t)kRenderStats * f, (int64_t)c->cam.W * c->cam.H, per_keyframe + f);
    return PSGSDF_OK;
}

}  // extern "C"
