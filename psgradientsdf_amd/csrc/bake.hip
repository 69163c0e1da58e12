// bake.hip -- detail maps of a level-of-detail mesh (include/psgsdf_bake.h):
//   k_bake   one wavefront per 8 x 8 texel tile of the atlas, one texel per lane: texel -> face and sample point by integer arithmetic, a short
//            ray from the coarse triangle along its interpolated normal through the renderer's own walk (render_trace.h), the band's normal and
//            albedo at the hit -- what render_tile gathers for a hit pixel -- and the signed displacement.  Plain stores; the five counts as
//            integer atomics of one lane per wavefront (integers: the same totals in whatever order).
#include "device_common.h"
#include "render_trace.h"
#include "bake.h"

namespace psg {

__device__ __forceinline__ unsigned char bake_byte(float c) { return (unsigned char)(int)floorf(255.0f * fminf(fmaxf(c, 0.0f), 1.0f) + 0.5f); }      // (mesh.hip colour_byte)

__global__ void __launch_bounds__(64) k_bake(BakeArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int tiles_x = (a.W + kRenderTile - 1) / kRenderTile;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int X = tx * kRenderTile + (lane & 7), Y = ty * kRenderTile + (lane >> 3);
    const bool inside = X < a.W && Y < a.H;
    const int R = a.res, B = R + 1;
    // texel -> face and sample indices (ta, tb); f = -1: padding
    int f = -1, ta = 0, tb = 0;
    if (inside) {
        const int bc = X / B, i = X - bc * B, br = Y / B, j = Y - br * B;
        const int q = br * a.bpr + bc;
        const bool even = i + j <= R;
        const long long ff = 2ll * q + (even ? 0 : 1);
        if (q < a.nblk && ff < a.nf) { f = (int)ff; ta = even ? i : R - i; tb = even ? j : R - j; }
    }
    const bool owned = f >= 0;
    float nout[3] = {0.f, 0.f, 0.f}, disp = 0.f;
    unsigned char col[3] = {0, 0, 0};
    int vox = -1;
    bool hit = false, buried = false, off = false;
    if (owned) {
        double w0, w1, w2, p[3], n[3];
        int v0, v1, v2;
        const bool ray = bake_sample(a.xyz, a.nrm, a.faces, f, ta, tb, R, w0, w1, w2, v0, v1, v2, p, n);
        float t = 0.f; long long lin = -1;
        if (ray) {
            float uo[3], uw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double o = p[k] + a.reach * n[k]; uo[k] = (float)(o / a.vs + 0.5); uw[k] = (float)(-n[k] / a.vs); }
            const bool found = render_trace<false>(a.r, uo, uw, t, lin);
            hit = found && t > 0.f && (double)t <= 2.0 * a.reach;
            buried = found && t == 0.f;
        }
        if (hit) {      // what render_tile gathers for a hit
            float nh[3], rho[3];
            const int row = a.has_band ? a.r.d.row_of[lin] : -1;
            if (row >= 0) {
                const float4 c0 = a.r.vp[0][row], c1 = a.r.vp[1][row], c2 = a.r.vp[2][row];
                nh[0] = c2.x; nh[1] = c2.y; nh[2] = c2.z;
                rho[0] = c0.w; rho[1] = c1.w; rho[2] = c2.w;
            } else {
                const float gr[3] = {a.r.d.g[0][lin], a.r.d.g[1][lin], a.r.d.g[2][lin]};
                normalized3(gr, nh);
#pragma unroll
                for (int k = 0; k < 3; ++k) rho[k] = a.r.d.rho[k][lin];
                off = true;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { nout[k] = nh[k]; col[k] = bake_byte(rho[k]); }
            disp = (float)(a.reach - (double)t);
            vox = (int)lin;
        } else {        // a miss or a buried texel: the coarse mesh's own interpolated values
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                nout[k] = (float)n[k];
                const double c = (w0 * (double)a.rgb[3 * (size_t)v0 + k] + w1 * (double)a.rgb[3 * (size_t)v1 + k]) + w2 * (double)a.rgb[3 * (size_t)v2 + k];
                col[k] = (unsigned char)(int)floor(c + 0.5);
            }
        }
    }
    if (inside) {
        const size_t px = (size_t)Y * a.W + X;
#pragma unroll
        for (int k = 0; k < 3; ++k) { a.albedo[3 * px + k] = col[k]; a.normal[3 * px + k] = nout[k]; }
        a.disp[px] = disp; a.voxel[px] = vox; a.face[px] = f;
    }
    const unsigned long long m_owned = __ballot(owned), m_hit = __ballot(hit), m_off = __ballot(hit && off), m_bur = __ballot(buried);
    if (lane == 0) {
        if (m_owned) atomicAdd(a.counts + BK_OWNED, (unsigned long long)__popcll(m_owned));
        if (m_hit) atomicAdd(a.counts + BK_HITS, (unsigned long long)__popcll(m_hit));
        if (m_off) atomicAdd(a.counts + BK_OFF_BAND, (unsigned long long)__popcll(m_off));
        if (m_bur) atomicAdd(a.counts + BK_BURIED, (unsigned long long)__popcll(m_bur));
    }
}

void launch_bake(const BakeArgs& a, hipStream_t s) {
    const int tiles_x = (a.W + kRenderTile - 1) / kRenderTile, tiles_y = (a.H + kRenderTile - 1) / kRenderTile;
    hipLaunchKernelGGL(k_bake, dim3((unsigned)(tiles_x * tiles_y)), dim3(64), 0, s, a);
}

}  // namespace psg
