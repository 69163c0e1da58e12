// relight.hip -- one view under a light of the caller's, with cast shadows (include/psgsdf_relight.h):
//   k_relight<KIND>   launched once per light over the planes k_render left on the device (depth, normal, albedo, voxel).  One lane per shadow ray,
//            K = 1 / 8 / 16 / 32 / 64 rays per pixel, so a wavefront covers 64 / K consecutive pixels in 8 x 8-tile order: its lanes start in
//            neighbouring cells.  Every lane sets its pixel up itself (occlusion.hip's reasoning: the K lanes of a pixel run the same instructions on
//            the same addresses, which costs what one lane would), turns sample i of the host's table into the frame of the light's centre direction
//            in double and walks it through the renderer's own cells (render_trace.h) with the walk cut at the ray's limit.  A pixel's count is the
//            popcount of the wavefront's ballot of `occluded` shifted down to the pixel's K lanes: no loop over rays, no reduction, no LDS.  Plain
//            stores by the pixel's first lane; the four counts as integer atomics of one lane per wavefront (integers: the same totals in whatever
//            order).  Lanes of missed and unlit pixels idle.
//   KIND: RL_SH has no rays (one lane per pixel, the irradiance in float as the forward model sums it); RL_DIRECTIONAL and RL_POINT differ in the
//   centre direction, the fall-off and the ray's limit.  Three instances, so that none carries the others' registers.
#include "device_common.h"
#include "render_trace.h"
#include "bake.h"
#include "relight.h"

namespace psg {

template <int KIND>
__global__ void __launch_bounds__(64) k_relight(RelightArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long g = a.g0 + (long long)blockIdx.x * 64 + lane;      // the ray
    const long long p = g >> a.log2K;                           // its pixel, in tile order
    const int i = (int)(g & (a.K - 1));                         // its sample
    const long long tile = p >> 6;
    const int in = (int)(p & 63);
    const int ty = (int)(tile / a.r.tiles_x), tx = (int)(tile - (long long)ty * a.r.tiles_x);
    const int x = tx * kRenderTile + (in & 7), y = ty * kRenderTile + (in >> 3);
    const bool inside = ty < a.r.tiles_y && x < a.r.cam.W && y < a.r.cam.H;
    const size_t HW = (size_t)a.r.cam.W * a.r.cam.H, px = inside ? (size_t)y * a.r.cam.W + x : 0;
    const bool hit = inside && __float_as_int(a.r.planes[RP_VOXEL][px]) >= 0;
    bool lit = false, occluded = false, buried = false;
    float n[3] = {0.f, 0.f, 0.f}, irr = 0.f;
    double shade = 0.0;                                          // cosv * fall of a lit pixel
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = a.r.planes[RP_NORMAL][k * HW + px];
        if (KIND == RL_SH) {
            float shb[9];
            if (a.n_sh == 9) { SH<9>(n, shb); irr = dotn<9>(a.sh, shb); }
            else { SH<4>(n, shb); irr = dotn<4>(a.sh, shb); }
            lit = true;
        } else {
            double m[3] = {(double)n[0], (double)n[1], (double)n[2]};
            const bool has_normal = bake_unit(m);
            // the hit point from the public planes: the renderer's float ray direction (render_tile's w = R dc, here without contraction, so that the
            // definition names every rounding: the two differ by an ulp of w at most, 1e-7 of the depth), the depth
            const FrameP& fp = a.r.frame >= 0 ? a.r.frames[a.r.frame] : a.r.pose;
            const float dc[3] = {((float)x - a.r.cam.cx) / a.r.cam.fx, ((float)y - a.r.cam.cy) / a.r.cam.fy, 1.f};
            float w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = (fp.R[3 * k] * dc[0] + fp.R[3 * k + 1] * dc[1]) + fp.R[3 * k + 2] * dc[2];
            const double t = (double)a.r.planes[RP_DEPTH][px];
            double q[3], wc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = (double)fp.t[k] + t * (double)w[k];
            double fall = 1.0;
            bool reachable = true;
            if (KIND == RL_POINT) {
#pragma unroll
                for (int k = 0; k < 3; ++k) wc[k] = a.vec[k] - q[k];
                const double r2 = (wc[0] * wc[0] + wc[1] * wc[1]) + wc[2] * wc[2];
                reachable = bake_unit(wc);
                fall = 1.0 / r2;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) wc[k] = a.vec[k];      // (the host has made it a unit vector)
            }
            const double cosv = (m[0] * wc[0] + m[1] * wc[1]) + m[2] * wc[2];
            lit = has_normal && reachable && cosv > 0.0;
            if (lit) {
                shade = cosv * fall;
                // the frame of wc (t1, t2, wc); sg + wc[2] is never zero
                const double sg = copysign(1.0, wc[2]), fa = -1.0 / (sg + wc[2]), fb = wc[0] * wc[1] * fa;
                const double t1[3] = {1.0 + sg * wc[0] * wc[0] * fa, sg * fb, -sg * wc[0]}, t2[3] = {fb, sg + wc[1] * wc[1] * fa, -wc[1]};
                const double da = a.dirs[3 * i], db = a.dirs[3 * i + 1];
                double o[3], d[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[k] = q[k] + a.bias * m[k];
                    const double e = da * t1[k] + db * t2[k];
                    d[k] = KIND == RL_POINT ? (a.vec[k] + a.spread * e) - o[k] : wc[k] + a.spread * e;
                }
                const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                if (len > 0.0) {      // (a point light's target in the ray's origin: not occluded)
                    const double limit = KIND == RL_POINT ? fmin(a.limit, len) : a.limit;
                    float t_max = (float)limit;      // rounded up if the conversion rounded down: no hit within the limit is cut off
                    if ((double)t_max < limit) t_max = nextafterf(t_max, INFINITY);
                    float uo[3], uw[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { uo[k] = (float)((o[k] - a.origin[k]) / a.vs + 0.5); uw[k] = (float)((d[k] / len) / a.vs); }
                    float th = 0.f; long long lin = -1;
                    const bool found = render_trace<false, true>(a.r, uo, uw, th, lin, t_max);
                    occluded = found && (double)th <= limit;
                    buried = found && th == 0.f;
                }
            }
        }
    }
    const unsigned long long b_occ = __ballot(occluded), b_bur = __ballot(buried), b_hit = __ballot(hit && i == 0), b_lit = __ballot(lit && i == 0);
    if (inside && i == 0) {
        const unsigned long long mk = (b_occ >> (lane & ~(a.K - 1))) & (a.K == 64 ? ~0ull : (1ull << a.K) - 1ull);
        const int c = __popcll(mk);
        const float vis = KIND == RL_SH ? (hit ? 1.f : 0.f) : lit ? (float)(a.K - c) / (float)a.K : 0.f;
        const double s = KIND == RL_SH ? (double)irr : lit ? shade * (double)vis : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double rho = hit ? (double)a.r.planes[RP_ALBEDO][k * HW + px] : 0.0;
            a.out[k * HW + px] = hit ? (float)(rho * ((double)a.ambient[k] + (double)a.colour[k] * s)) : 0.f;
        }
        a.out[3 * HW + px] = vis;
    }
    if (lane == 0) {
        if (b_hit) atomicAdd(a.counts + RL_HITS, (unsigned long long)__popcll(b_hit));
        if (b_lit) atomicAdd(a.counts + RL_LIT, (unsigned long long)__popcll(b_lit));
        if (b_occ) atomicAdd(a.counts + RL_OCCLUDED, (unsigned long long)__popcll(b_occ));
        if (b_bur) atomicAdd(a.counts + RL_BURIED, (unsigned long long)__popcll(b_bur));
    }
}

// the rays of the view's tiles (whole 8 x 8 tiles: a multiple of 64 pixels) in launches of at most kRelightChunk, so that no pixel and no wavefront
// straddles two launches and no dispatch passes 2^32 work-items however the view is shaped
hipError_t launch_relight(RelightArgs a, hipStream_t s) {
    const long long rays = (long long)a.r.tiles_x * a.r.tiles_y * 64 * a.K;
    for (a.g0 = 0; a.g0 < rays; a.g0 += kRelightChunk) {
        const unsigned blocks = (unsigned)(std::min(rays - a.g0, kRelightChunk) / 64);
        if (a.kind == RL_SH) hipLaunchKernelGGL(k_relight<RL_SH>, dim3(blocks), dim3(64), 0, s, a);
        else if (a.kind == RL_POINT) hipLaunchKernelGGL(k_relight<RL_POINT>, dim3(blocks), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_relight<RL_DIRECTIONAL>, dim3(blocks), dim3(64), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace psg
