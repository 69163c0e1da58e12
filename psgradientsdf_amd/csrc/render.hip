// render.hip -- view rendering of the engine's state (include/psgsdf_render.h):
//   k_render_bricks   the empty-space map: bricks of 8^3 voxels that may hold a hit, and their bounding box (the rays' clip interval)
//   k_render          one view: one wavefront per 8 x 8 pixel tile, one ray per lane, the planes asked for + per-tile stat partials
//   k_render_report   the same traversal for every keyframe at once (keyframe = blockIdx.y), partials only
//   k_render_fold     the partials of each view summed in one fixed order (one workgroup per view: strided per-thread sums, then an LDS tree):
//                     reproducible sums, the same for a single view and for its row of the report
// Multi-rank (z-slab) contexts ("Multi-rank contexts"), between exchanges over the context's communicator:
//   k_render_bricks   marks of the planes the rank owns, in global brick coordinates;  k_render_box: map and box of the merged marks
//   k_render_ranks    the same traversal restricted to the owned planes: a hit record per pixel (the fields as float bits) + the rank's hit bit
//   k_render_keep     the records of the pixels whose first hit lies in another rank's slab zeroed (winner: the first slab with a hit along the ray)
//   k_render_composite the planes and the per-tile partials from the composited records, through the same per-pixel stat code as k_render
#include "device_common.h"
#include "render_trace.h"

namespace psg {

// A cell can only hold a hit when phi can reach zero inside it: |p - x_v| <= (sqrt(3) / 2) vs and |g| = 1, so d_v <= (sqrt(3) / 2) vs.  The host
// passes that bound with a relative margin of 1e-3: a brick is skipped only when no voxel of it can be hit, whatever the rounding.
__global__ void __launch_bounds__(kBlock) k_render_bricks(DenseView d, GridP g, float thr, int nb0, int nb1, int nb2, int z0, int z1,
                                                          unsigned char* __restrict__ bricks, int* __restrict__ bbox, double* __restrict__ marks) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (b >= (long long)nb0 * nb1 * nb2) return;                     // (wavefront-uniform)
    const int bz = (int)(b / ((long long)nb0 * nb1)), rest = (int)(b - (long long)bz * nb0 * nb1);
    const int by = rest / nb0, bx = rest - by * nb0;
    const int y = by * kRenderBrick + (lane & 7), z = bz * kRenderBrick + (lane >> 3);
    bool occ = false;
    if (y < g.dim[1] && z >= z0 && z < z1) {
        const long long row = ((long long)(z - g.koff) * g.dim[1] + y) * g.dim[0];
        for (int i = 0; i < kRenderBrick; ++i) {
            const int x = bx * kRenderBrick + i;
            if (x < g.dim[0]) occ |= d.weight[row + x] > 0.f && d.dist[row + x] <= thr;
        }
    }
    const bool any = __ballot(occ) != 0ull;
    if (lane == 0) {
        if (marks) { marks[b] = any ? 1.0 : 0.0; return; }
        bricks[b] = any ? 1 : 0;
        if (any) {
            atomicMin(bbox + 0, bx); atomicMin(bbox + 1, by); atomicMin(bbox + 2, bz);
            atomicMin(bbox + 3, -bx); atomicMin(bbox + 4, -by); atomicMin(bbox + 5, -bz);
        }
    }
}
void launch_render_bricks(const DenseView& d, const GridP& g, float thr, int z0, int z1, unsigned char* bricks, int* bbox, double* marks, hipStream_t s) {
    int nb[3];
    for (int k = 0; k < 3; ++k) nb[k] = (g.dim[k] + kRenderBrick - 1) / kRenderBrick;
    const long long n = (long long)nb[0] * nb[1] * nb[2];
    hipLaunchKernelGGL(k_render_bricks, dim3((unsigned)((n + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, s, d, g, thr, nb[0], nb[1], nb[2], z0, z1, bricks, bbox, marks);
}

// the map and box of the ranks' merged marks (every rank runs it on the same sums: the same map and box everywhere, the single-rank ones)
__global__ void __launch_bounds__(kBlock) k_render_box(const double* __restrict__ marks, int nb0, int nb1, long long n, unsigned char* __restrict__ bricks, int* __restrict__ bbox) {
    const long long b = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= n) return;
    const bool occ = marks[b] > 0.0;
    bricks[b] = occ ? 1 : 0;
    if (occ) {
        const int bz = (int)(b / ((long long)nb0 * nb1)), rest = (int)(b - (long long)bz * nb0 * nb1);
        const int by = rest / nb0, bx = rest - by * nb0;
        atomicMin(bbox + 0, bx); atomicMin(bbox + 1, by); atomicMin(bbox + 2, bz);
        atomicMin(bbox + 3, -bx); atomicMin(bbox + 4, -by); atomicMin(bbox + 5, -bz);
    }
}
void launch_render_box(const double* marks, const int* nb, unsigned char* bricks, int* bbox, hipStream_t s) {
    const long long n = (long long)nb[0] * nb[1] * nb[2];
    hipLaunchKernelGGL(k_render_box, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, marks, nb[0], nb[1], n, bricks, bbox);
}

// The stats of one hit pixel (st[0..8]) and its residual: the one definition k_render, k_render_report and k_render_composite share.
template <int IMG>
__device__ __forceinline__ void render_pixel_stats(const RenderArgs& a, int frame, int x, int y, bool off_band, const float* ren, float* res, double* st) {
#pragma clang fp contract(off)
    st[0] = 1.0;
    st[1] = off_band ? 1.0 : 0.0;
    if (frame >= 0) {
        float I[3];
        const size_t px = ((size_t)frame * a.img_h + y) * a.img_w + x;
        if (IMG == 1) unpack_rgb8(a.im.u8[px], a.im.scale, I);
        else { I[0] = a.im.f32[3 * px]; I[1] = a.im.f32[3 * px + 1]; I[2] = a.im.f32[3 * px + 2]; }
        float rob = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            res[k] = I[k] - ren[k];
            st[2 + k] = (double)(res[k] * res[k]);
            st[5 + k] = (double)fabsf(res[k]);
            rob += robust_loss<-1>(a.rob, res[k]);
        }
        st[8] = (double)rob;
    }
}

// the planes asked for at pixel (x, y) (a miss: zeros, voxel -1)
__device__ __forceinline__ void render_write_planes(const RenderArgs& a, int x, int y, bool hit, float t, long long lin, const float* n, const float* rho,
                                                    float shade, const float* ren, const float* res) {
    const size_t HW = (size_t)a.cam.W * a.cam.H, px = (size_t)y * a.cam.W + x;
    if (a.planes[RP_DEPTH]) a.planes[RP_DEPTH][px] = hit ? t : 0.f;
    if (a.planes[RP_SHADING]) a.planes[RP_SHADING][px] = shade;
    if (a.planes[RP_VOXEL]) a.planes[RP_VOXEL][px] = __int_as_float(hit ? (int)lin : -1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.planes[RP_NORMAL]) a.planes[RP_NORMAL][k * HW + px] = n[k];
        if (a.planes[RP_ALBEDO]) a.planes[RP_ALBEDO][k * HW + px] = rho[k];
        if (a.planes[RP_RENDERED]) a.planes[RP_RENDERED][k * HW + px] = ren[k];
        if (a.planes[RP_RESIDUAL]) a.planes[RP_RESIDUAL][k * HW + px] = res[k];
    }
}

// the tile's partials (lane order of an 8 x 8 tile, wave_sum) into part slot `slot`
__device__ __forceinline__ void render_tile_sums(const RenderArgs& a, const double* st, long long slot) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kRenderStats; ++k) {
        const double v = wave_sum(st[k]);
        if (lane == 0) a.part[slot * kRenderStats + k] = v;
    }
}

// One 8 x 8 tile of view `frame` (-1: the caller's camera a.pose, light of a.light_frame); partials of the tile into part slot `slot`.
// k_render and k_render_report run exactly this code, so that the report's rows equal the single views' stats bit for bit.
// MR: the traversal of the owned planes, and instead of planes and partials the pixel's hit bit and record (record frame `rf` of the chunk).
template <int MODEL, int IMG, bool MR>
__device__ __forceinline__ void render_tile(const RenderArgs& a, int frame, int tile, long long slot, int rf) {
#pragma clang fp contract(off)
    constexpr int NB = ModelTraits<MODEL>::NB;
    const int lane = threadIdx.x & 63;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = tx * kRenderTile + (lane & 7), y = ty * kRenderTile + (lane >> 3);
    const bool inside = x < a.cam.W && y < a.cam.H;
    FrameP fp = frame >= 0 ? a.frames[frame] : a.pose;
    const int lf = frame >= 0 ? frame : a.light_frame;
#pragma unroll
    for (int i = 0; i < 9; ++i) fp.l[i] = a.frames[lf].l[i];
    const float dc[3] = {((float)x - a.cam.cx) / a.cam.fx, ((float)y - a.cam.cy) / a.cam.fy, 1.f};
    float w[3]; mul3(fp.R, dc, w);
    float uo[3], uw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { uo[k] = (fp.t[k] - a.grid.origin[k]) / a.grid.vs + 0.5f; uw[k] = w[k] / a.grid.vs; }
    float t = 0.f; long long lin = -1;
    const bool hit = inside && render_trace<MR>(a, uo, uw, t, lin);
    float n[3] = {0.f, 0.f, 0.f}, rho[3] = {0.f, 0.f, 0.f}, ren[3] = {0.f, 0.f, 0.f}, res[3] = {0.f, 0.f, 0.f}, shade = 0.f;
    bool off = false;
    double st[kRenderStats];
#pragma unroll
    for (int k = 0; k < kRenderStats; ++k) st[k] = 0.0;
    if (hit) {
        const long long li = MR ? lin - (long long)a.grid.koff * a.grid.dim[0] * a.grid.dim[1] : lin;
        const int row = a.d.row_of[li];
        if (row >= 0) {      // band voxel: what the energy renders with (Band::vp: nfd, rho)
            const float4 v0 = a.vp[0][row], v1 = a.vp[1][row], v2 = a.vp[2][row];
            n[0] = v2.x; n[1] = v2.y; n[2] = v2.z;
            rho[0] = v0.w; rho[1] = v1.w; rho[2] = v2.w;
        } else {             // fused voxel outside the band: normalised stored gradient, fused colour
            const float gr[3] = {a.d.g[0][li], a.d.g[1][li], a.d.g[2][li]};
            normalized3(gr, n);
#pragma unroll
            for (int k = 0; k < 3; ++k) rho[k] = a.d.rho[k][li];
            off = true;
        }
        Proj pr{};
#pragma unroll
        for (int k = 0; k < 3; ++k) pr.p[k] = t * dc[k];
        float shb[NB];
        SH<NB>(n, shb);
        rendered<MODEL>(fp, pr, n, shb, rho, ren);
        // the scalar shading: the same forward model with unit albedo (and unit LED intensity)
        const float one[3] = {1.f, 1.f, 1.f};
        float o[3];
        if (ModelTraits<MODEL>::LED) { FrameP fu = fp; fu.l[0] = fu.l[1] = fu.l[2] = 1.f; rendered<MODEL>(fu, pr, n, shb, one, o); }
        else rendered<MODEL>(fp, pr, n, shb, one, o);
        shade = o[0];
        if (!MR) render_pixel_stats<IMG>(a, frame, x, y, off, ren, res, st);
    }
    if (MR) {
        if (!inside) return;
        const size_t i = (size_t)rf * a.cam.W * a.cam.H + (size_t)y * a.cam.W + x;
        a.mask[i] = hit ? (double)(1ull << a.slab) : 0.0;
        a.mine[i] = hit ? (uw[2] < 0.f ? 2 : 1) : 0;
        const float f[RF_COUNT] = {t, n[0], n[1], n[2], rho[0], rho[1], rho[2], shade, ren[0], ren[1], ren[2], __int_as_float((int)lin), off ? 1.f : 0.f};
#pragma unroll
        for (int q = 0; q < RF_COUNT; ++q)
            if (a.rf[q] >= 0) a.rec[(size_t)a.rf[q] * a.rec_px + i] = hit ? (double)__float_as_uint(f[q]) : 0.0;
        return;
    }
    if (inside) render_write_planes(a, x, y, hit, t, lin, n, rho, shade, ren, res);
    render_tile_sums(a, st, slot);
}

template <int MODEL, int IMG>
__global__ void __launch_bounds__(64) k_render(RenderArgs a) {
    render_tile<MODEL, IMG, false>(a, a.frame, blockIdx.x, blockIdx.x, 0);
}
template <int MODEL, int IMG>
__global__ void __launch_bounds__(64) k_render_report(RenderArgs a) {
    render_tile<MODEL, IMG, false>(a, blockIdx.y, blockIdx.x, (long long)blockIdx.y * gridDim.x + blockIdx.x, 0);
}
// multi-rank: one view (report == 0) or keyframes a.f0 + blockIdx.y of the report
template <int MODEL, int IMG>
__global__ void __launch_bounds__(64) k_render_ranks(RenderArgs a, int report) {
    render_tile<MODEL, IMG, true>(a, report ? a.f0 + (int)blockIdx.y : a.frame, blockIdx.x, 0, blockIdx.y);
}

#define PSG_RENDER_LAUNCH(K, grid, a, model, ...) do { \
        const bool u8_ = (a).im.u8 != nullptr; \
        if ((model) == 0) { if (u8_) hipLaunchKernelGGL((K<0, 1>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); else hipLaunchKernelGGL((K<0, 0>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); } \
        else if ((model) == 1) { if (u8_) hipLaunchKernelGGL((K<1, 1>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); else hipLaunchKernelGGL((K<1, 0>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); } \
        else { if (u8_) hipLaunchKernelGGL((K<2, 1>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); else hipLaunchKernelGGL((K<2, 0>), grid, dim3(64), 0, s, a, ##__VA_ARGS__); } \
    } while (0)

void launch_render(const RenderArgs& a, int model, hipStream_t s) {
    PSG_RENDER_LAUNCH(k_render, dim3(a.tiles_x * a.tiles_y), a, model);
}
void launch_render_report(const RenderArgs& a, int model, int F, hipStream_t s) {
    PSG_RENDER_LAUNCH(k_render_report, dim3(a.tiles_x * a.tiles_y, F), a, model);
}
void launch_render_ranks(const RenderArgs& a, int model, bool report, int chunk, hipStream_t s) {
    PSG_RENDER_LAUNCH(k_render_ranks, dim3(a.tiles_x * a.tiles_y, chunk), a, model, report ? 1 : 0);
}

// After the exchange of the hit masks: the winner of a pixel is the first slab with a hit in the direction of its ray's z (a ray with
// uw[2] == 0 stays in one plane: one slab at most can hit); every other rank zeroes its record, so the sum of the records is the winner's.
__global__ void __launch_bounds__(kBlock) k_render_keep(RenderArgs a) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.rec_px) return;
    const int m = a.mine[i];
    if (!m) return;
    const unsigned long long hits = (unsigned long long)a.mask[i], me = 1ull << a.slab;
    const bool win = m == 1 ? (hits & (me - 1)) == 0ull : (hits >> (a.slab + 1)) == 0ull;
    if (win) return;
    for (int q = 0; q < a.n_rf; ++q) a.rec[(size_t)q * a.rec_px + i] = 0.0;
}
void launch_render_keep(const RenderArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_render_keep, dim3((unsigned)((a.rec_px + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
}

// After the exchange of the records: the pixels of one 8 x 8 tile in k_render's lane order, the planes and the stats through the same per-pixel
// code, the tile's partials into the slot k_render / k_render_report use.
template <int IMG>
__global__ void __launch_bounds__(64) k_render_composite(RenderArgs a, int report) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x;
    const int frame = report ? a.f0 + (int)blockIdx.y : a.frame;
    const long long slot = report ? (long long)frame * gridDim.x + tile : tile;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = tx * kRenderTile + (lane & 7), y = ty * kRenderTile + (lane >> 3);
    const bool inside = x < a.cam.W && y < a.cam.H;
    const size_t i = (size_t)blockIdx.y * a.cam.W * a.cam.H + (size_t)y * a.cam.W + x;
    const bool hit = inside && a.mask[i] != 0.0;
    float f[RF_COUNT];
#pragma unroll
    for (int q = 0; q < RF_COUNT; ++q) f[q] = hit && a.rf[q] >= 0 ? __uint_as_float((unsigned)a.rec[(size_t)a.rf[q] * a.rec_px + i]) : 0.f;
    float res[3] = {0.f, 0.f, 0.f};
    double st[kRenderStats];
#pragma unroll
    for (int k = 0; k < kRenderStats; ++k) st[k] = 0.0;
    if (hit) render_pixel_stats<IMG>(a, frame, x, y, f[RF_OFF_BAND] != 0.f, f + RF_RENDERED, res, st);
    if (inside) render_write_planes(a, x, y, hit, f[RF_DEPTH], __float_as_int(f[RF_VOXEL]), f + RF_NORMAL, f + RF_ALBEDO, f[RF_SHADING], f + RF_RENDERED, res);
    render_tile_sums(a, st, slot);
}
void launch_render_composite(const RenderArgs& a, bool report, int chunk, hipStream_t s) {
    const dim3 grid(a.tiles_x * a.tiles_y, chunk);
    if (a.im.u8) hipLaunchKernelGGL(k_render_composite<1>, grid, dim3(64), 0, s, a, report ? 1 : 0);
    else hipLaunchKernelGGL(k_render_composite<0>, grid, dim3(64), 0, s, a, report ? 1 : 0);
}

__global__ void __launch_bounds__(kBlock) k_render_fold(const double* __restrict__ part, int tiles, double* __restrict__ out) {
    __shared__ double red[kBlock];
    const size_t base = (size_t)blockIdx.x * tiles;
    for (int k = 0; k < kRenderStats; ++k) {
        double v = 0.0;
        for (int i = threadIdx.x; i < tiles; i += kBlock) v += part[(base + i) * kRenderStats + k];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * kRenderStats + k] = red[0];
        __syncthreads();
    }
}
void launch_render_fold(const double* part, int tiles, int F, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_render_fold, dim3(F), dim3(kBlock), 0, s, part, tiles, out);
}

}  // namespace psg
