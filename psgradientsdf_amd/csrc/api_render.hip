// api_render.hip -- the C ABI of include/psgsdf_render.h: one view (psgsdf_render) or the stats of every keyframe in one pass
// (psgsdf_render_report), and of include/psgsdf_relight.h: one view under the caller's lights (psgsdf_relight).  Kernels: render.hip, relight.hip.
// On a multi-rank context the two of psgsdf_render.h are collective calls (psgsdf_relight is refused there) ("Multi-rank contexts"): every rank traces its own slab, and three sum all-reduces over the
// context's communicator (brick marks + the call's checksum, per-pixel hit masks, the winners' records) give every rank the single-rank result.
#include "extract_internal.h"
#include "../../include/psgsdf_render.h"
#include "../../include/psgsdf_relight.h"
#include "relight.h"

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

// the rules of a view (psgsdf_render, psgsdf_relight); true: one is broken, its text in msg.  with_light: light_frame is read
bool view_bad(const psgsdf_ctx* c, const psgsdf_view* v, const char* what, bool with_light, char* msg, size_t n) {
    if (v->frame >= 0) {
        if (v->frame >= c->F) { snprintf(msg, n, "%s: keyframe %d of %d", what, v->frame, c->F); return true; }
        return false;
    }
    if (with_light && (v->light_frame < 0 || v->light_frame >= c->F)) { snprintf(msg, n, "%s: light_frame %d of %d", what, v->light_frame, c->F); return true; }
    if (v->width <= 0 || v->height <= 0 || (int64_t)v->width * v->height > ((int64_t)1 << 28)) { snprintf(msg, n, "%s: view size %d x %d", what, v->width, v->height); return true; }
    if (!(v->fx != 0.f) || !(v->fy != 0.f)) { snprintf(msg, n, "%s: zero focal length", what); return true; }
    return false;
}
// camera, pose, light and tiles of a checked view into the kernels' arguments (light_frame: of a caller's camera; a keyframe view has its own)
void view_into(const psgsdf_ctx* c, const psgsdf_view* v, int light_frame, RenderArgs& a) {
    if (v->frame >= 0) { a.cam = c->cam; a.frame = v->frame; a.light_frame = v->frame; }
    else {
        a.cam.fx = v->fx; a.cam.fy = v->fy; a.cam.cx = v->cx; a.cam.cy = v->cy; a.cam.W = v->width; a.cam.H = v->height;
        a.frame = -1; a.light_frame = light_frame;
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) a.pose.R[i * 3 + j] = v->pose[i * 4 + j]; a.pose.t[i] = v->pose[i * 4 + 3]; }
    }
    a.tiles_x = (a.cam.W + kRenderTile - 1) / kRenderTile; a.tiles_y = (a.cam.H + kRenderTile - 1) / kRenderTile;
}

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
    if (view_bad(c, v, "render", true, msg, sizeof(msg))) bad(msg);
    if (!key && (channels & PSGSDF_R_RESIDUAL)) bad("render: a residual needs a keyframe view");
    if (err[0] && !mr) return fail(c, PSGSDF_ERR_ARG, "%s", err);
    DevMem m;      // per-call device memory: brick map, bbox, planes, partials, folded sums
    RenderArgs a;
    { int rc = render_args(c, m, a, view_hash(v, channels), "render", err[0] ? err : nullptr); if (rc) return rc; }
    view_into(c, v, v->light_frame, a);
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

// ---- relighting (include/psgsdf_relight.h; kernel: relight.hip k_relight): the primary hit by k_render itself, its planes left on
// the device; then one launch of shadow rays per light over those planes, each light's four planes downloaded behind its launch.
int psgsdf_relight(psgsdf_ctx* c, const psgsdf_view* v, const psgsdf_light* lights, const psgsdf_relight_params* p, float* out_host, float* geometry_host,
                   psgsdf_relight_counts* per_light) {
    const char* me = "relight";
    if (!c || !v || !lights || !p || !out_host) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own planes of the volume")) return rc;
    if (!c->inited || !c->have_frames) return fail(c, PSGSDF_ERR_STATE, "%s: init first", me);
    if (!(p->bias > 0.0) || std::isinf(p->bias) || !(p->reach >= 0.0) || std::isinf(p->reach)) return fail(c, PSGSDF_ERR_ARG, "%s: the bias must be a finite length > 0, the reach one >= 0", me);
    if (p->n_lights < 1 || p->n_lights > PSGSDF_RELIGHT_MAX_LIGHTS || p->reserved != 0) return fail(c, PSGSDF_ERR_ARG, "%s: n_lights %d, reserved %d (1 to 64 lights; reserved 0)", me, p->n_lights, p->reserved);
    auto nonneg = [](const float* x, int n) { for (int k = 0; k < n; ++k) if (!(x[k] >= 0.f) || std::isinf(x[k])) return false; return true; };
    auto finite = [](const float* x, int n) { for (int k = 0; k < n; ++k) if (!std::isfinite(x[k])) return false; return true; };
    for (int l = 0; l < p->n_lights; ++l) {
        const psgsdf_light& L = lights[l];
        const char* why = nullptr;
        if (!nonneg(L.colour, 3) || !nonneg(L.ambient, 3) || !nonneg(&L.spread, 1)) why = "colour, ambient and spread must be finite and >= 0";
        else if (L.kind == PSGSDF_LIGHT_SH) {
            if ((L.n_sh != 4 && L.n_sh != 9) || !finite(L.sh, L.n_sh)) why = "an SH light has 4 or 9 finite coefficients";
            else if (L.n_shadow != 0 || L.spread != 0.f) why = "an SH light has no shadow rays and no spread";
        } else if (L.kind == PSGSDF_LIGHT_DIRECTIONAL || L.kind == PSGSDF_LIGHT_POINT) {
            const int K = L.n_shadow;
            if (L.n_sh != 0) why = "n_sh is 0 unless the light is an SH light";
            else if (!finite(L.vec, 3)) why = "vec must be finite";
            else if (L.kind == PSGSDF_LIGHT_DIRECTIONAL && L.vec[0] == 0.f && L.vec[1] == 0.f && L.vec[2] == 0.f) why = "a direction of length zero";
            else if (K != 1 && K != 8 && K != 16 && K != 32 && K != 64) why = "n_shadow is 1, 8, 16, 32 or 64";
            else if (L.spread > 0.f && K < 8) why = "a spread > 0 needs at least 8 shadow rays";
        } else why = "unknown kind";
        if (why) return fail(c, PSGSDF_ERR_ARG, "%s: light %d: %s", me, l, why);
    }
    { int rc = render_ready(c, me); if (rc) return rc; }
    char msg[160];
    if (view_bad(c, v, me, false, msg, sizeof(msg))) return fail(c, PSGSDF_ERR_ARG, "%s", msg);
    {   // one light's rays (at most 64 per pixel) stay within 2^30
        const int64_t W = v->frame >= 0 ? c->cam.W : v->width, H = v->frame >= 0 ? c->cam.H : v->height;
        if (W * H > ((int64_t)1 << 24)) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: a view of %lld x %lld pixels (at most 2^24)", me, (long long)W, (long long)H);
    }
    DevMem m(c);      // per-call device memory: brick map, bbox, the view's planes, partials, one light's planes, the tables and counts
    psg::RelightArgs a{};
    { int rc = render_args(c, m, a.r, 0.0, me, nullptr); if (rc) return rc; }
    RenderArgs& r = a.r;
    view_into(c, v, 0, r);
    const size_t HW = (size_t)r.cam.W * r.cam.H;
    const int tiles = r.tiles_x * r.tiles_y, nl = p->n_lights;
    // the primary pass: k_render as psgsdf_render launches it, writing the four geometry planes (in the order of geometry_host)
    float* planes = nullptr;
    double* tables = nullptr;
    unsigned long long* counts = nullptr;
    if (!m.get(&planes, 8 * HW) || !m.get(&r.part, kRenderStats * (size_t)tiles) || !m.get(&a.out, 4 * HW) || !m.get(&tables, (size_t)3 * (1 + 8 + 16 + 32 + 64))
        || !m.get(&counts, (size_t)psg::kRelightCounts * nl)) return oom(c);
    r.planes[RP_DEPTH] = planes; r.planes[RP_NORMAL] = planes + HW; r.planes[RP_ALBEDO] = planes + 4 * HW; r.planes[RP_VOXEL] = planes + 7 * HW;
    timed(c, "k_render", [&] { launch_render(r, c->set.model, c->stream); });
    HIPCHK(c, hipGetLastError());
    if (geometry_host) HIPCHK(c, hipMemcpyAsync(geometry_host, planes, sizeof(float) * 8 * HW, hipMemcpyDeviceToHost, c->stream));
    // the sample tables of every K, one after the other: DESIGN.md 15's direction table (K = 1: the centre alone)
    std::vector<double> D;
    size_t table_of[65] = {0};
    for (int K : {1, 8, 16, 32, 64}) {
        table_of[K] = D.size();
        const double g = 0.6180339887498949, pi = 3.141592653589793;
        for (int i = 0; i < K; ++i) {
            const double u = ((double)i + 0.5) / (double)K, rr = sqrt(u), z = sqrt(1.0 - u), phi = 2.0 * pi * ((double)i * g - floor((double)i * g));
            if (K == 1) { D.push_back(0.0); D.push_back(0.0); D.push_back(1.0); }
            else { D.push_back(rr * cos(phi)); D.push_back(rr * sin(phi)); D.push_back(z); }
        }
    }
    HIPCHK(c, hipMemcpyAsync(tables, D.data(), sizeof(double) * D.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(unsigned long long) * psg::kRelightCounts * nl, c->stream));
    a.bias = p->bias; a.limit = p->reach > 0.0 ? p->reach : (double)INFINITY; a.vs = (double)c->grid.vs;
    for (int k = 0; k < 3; ++k) a.origin[k] = (double)c->grid.origin[k];
    for (int l = 0; l < nl; ++l) {
        const psgsdf_light& L = lights[l];
        a.kind = L.kind; a.n_sh = L.n_sh;
        a.K = L.kind == PSGSDF_LIGHT_SH ? 1 : L.n_shadow;
        a.log2K = a.K == 1 ? 0 : a.K == 8 ? 3 : a.K == 16 ? 4 : a.K == 32 ? 5 : 6;
        for (int k = 0; k < 9; ++k) a.sh[k] = L.sh[k];
        for (int k = 0; k < 3; ++k) { a.vec[k] = (double)L.vec[k]; a.colour[k] = L.colour[k]; a.ambient[k] = L.ambient[k]; }
        if (L.kind == PSGSDF_LIGHT_DIRECTIONAL) {      // wc = unit(vec)
            const double len = sqrt((a.vec[0] * a.vec[0] + a.vec[1] * a.vec[1]) + a.vec[2] * a.vec[2]);
            for (int k = 0; k < 3; ++k) a.vec[k] /= len;
        }
        a.spread = (double)L.spread;
        a.dirs = tables + table_of[a.K];
        a.counts = counts + (size_t)psg::kRelightCounts * l;
        hipError_t launched = hipSuccess;
        timed(c, "k_relight", [&] { launched = psg::launch_relight(a, c->stream); });
        if (launched != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of light %d: %s", me, l, hipGetErrorString(launched));
        HIPCHK(c, hipMemcpyAsync(out_host + (size_t)l * 4 * HW, a.out, sizeof(float) * 4 * HW, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<unsigned long long> cnt((size_t)psg::kRelightCounts * nl);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), counts, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (per_light)
        for (int l = 0; l < nl; ++l) {
            const unsigned long long* q = cnt.data() + (size_t)psg::kRelightCounts * l;
            const int K = lights[l].kind == PSGSDF_LIGHT_SH ? 0 : lights[l].n_shadow;
            per_light[l].n_hits = (int64_t)q[psg::RL_HITS]; per_light[l].n_lit = (int64_t)q[psg::RL_LIT]; per_light[l].n_rays = (int64_t)K * per_light[l].n_lit;
            per_light[l].n_occluded = (int64_t)q[psg::RL_OCCLUDED]; per_light[l].n_buried = (int64_t)q[psg::RL_BURIED];
        }
    return PSGSDF_OK;
}

}  // extern "C"
