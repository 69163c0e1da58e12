// render_trace.h -- the renderer's cell walk and first-order surface model, shared by the kernels that trace rays through the
// reconstruction: render.hip (one ray per pixel of a view), bake.hip (one ray per texel of a level-of-detail mesh's atlas) and occlusion.hip (K short rays per sample).  One copy of the
// arithmetic: whatever traces through this function meets the same cells, crossings and hit parameters.
#pragma once
#include "device_common.h"

namespace psg {

// The ray u(t) = uo + t uw in voxel units shifted by one half (cell of voxel c: c <= u < c + 1, VoxelGrid::world2voxel), t = camera z.
// Returns the first t at which phi_v(p) = d_v + g_v.(p - x_v) <= 0 inside an observed cell, and that cell's voxel (global linear index).  Every
// boundary crossing is computed from uo and uw directly (no accumulated increments), the same arithmetic as the plain restatement in
// tests/_render_ref.py.
// MR (a slab of a multi-rank context): the same walk over the same global brick map -- the same cells, crossings and t -- but only cells of the
// owned planes a.zr are evaluated (dense planes at the local index lin - koff nx ny), and the walk ends once the ray has left them in its direction
// of travel.  Along a ray z is monotonic, so the single-rank hit is the hit of the first slab (in the direction of travel) that has one.
// CUT (occlusion.hip: short rays): the walk ends once a cell's entry parameter is beyond t_max.  t never decreases along the walk and a hit's parameter
// is at least its cell's entry parameter, so every hit with t <= t_max is still found, with the same t and cell.  Without CUT the test is not
// compiled: the renderer's and the bake's instantiations are the ones they were.
template <bool MR, bool CUT = false>
__device__ __forceinline__ bool render_trace(const RenderArgs& a, const float* uo, const float* uw, float& t_hit, long long& lin_hit, const float t_max = FLT_MAX) {
#pragma clang fp contract(off)
    // the occupied-brick box, validated BEFORE any arithmetic on it: with no occupied brick the six words keep their 0x7f7f7f7f fill (bbox[k] >= nb[k]),
    // and only a box of brick indices inside [0, nb) turns into cell bounds inside [0, dim)
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int b0 = a.bbox[k], b1 = -a.bbox[3 + k];
        if (b0 < 0 || b0 >= a.nb[k] || b1 < b0 || b1 >= a.nb[k]) return false;
        lo[k] = b0 * kRenderBrick; hi[k] = min((b1 + 1) * kRenderBrick, a.grid.dim[k]);
    }
    float t0 = 0.f, t1 = FLT_MAX, inv[3];
    int step[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (uw[k] == 0.f) {
            if (!(uo[k] >= (float)lo[k] && uo[k] < (float)hi[k])) return false;
            inv[k] = 0.f; step[k] = 0;
        } else {
            inv[k] = 1.f / uw[k]; step[k] = uw[k] > 0.f ? 1 : -1;
            const float ta = ((float)lo[k] - uo[k]) * inv[k], tb = ((float)hi[k] - uo[k]) * inv[k];
            t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
        }
    }
    if (!(t0 < t1)) return false;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = min(max((int)floorf(uo[k] + t0 * uw[k]), lo[k]), hi[k] - 1);
    float t = t0;
    const int nx = a.grid.dim[0];
    const long long nxy = (long long)a.grid.dim[0] * a.grid.dim[1];
    const int max_steps = (hi[0] - lo[0]) + (hi[1] - lo[1]) + (hi[2] - lo[2]) + 8;
    for (int it = 0; it < max_steps; ++it) {
        if (CUT && t > t_max) return false;
        if (MR && (step[2] > 0 ? c[2] >= a.zr[1] : step[2] < 0 ? c[2] < a.zr[0] : (c[2] < a.zr[0] || c[2] >= a.zr[1]))) return false;   // past the owned planes
        const int bc[3] = {c[0] / kRenderBrick, c[1] / kRenderBrick, c[2] / kRenderBrick};
        if (!a.bricks[bc[0] + a.nb[0] * (bc[1] + a.nb[1] * bc[2])]) {
            // empty brick: on to the first cell behind its exit face
            float tb = FLT_MAX; int ax = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (!step[k]) continue;
                const float bound = (float)((bc[k] + (step[k] > 0 ? 1 : 0)) * kRenderBrick);
                const float tt = (bound - uo[k]) * inv[k];
                if (tt < tb) { tb = tt; ax = k; }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == ax) c[k] = step[k] > 0 ? (bc[k] + 1) * kRenderBrick : bc[k] * kRenderBrick - 1;
                else {
                    const int b0 = bc[k] * kRenderBrick;
                    c[k] = min(max((int)floorf(uo[k] + tb * uw[k]), max(b0, lo[k])), min(b0 + kRenderBrick, hi[k]) - 1);
                }
            }
            if (c[ax] < lo[ax] || c[ax] >= hi[ax]) return false;
            t = fmaxf(t, tb);
            continue;
        }
        float te = FLT_MAX; int ax = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!step[k]) continue;
            const float tt = ((float)(c[k] + (step[k] > 0 ? 1 : 0)) - uo[k]) * inv[k];
            if (tt < te) { te = tt; ax = k; }
        }
        const long long lin = (long long)c[0] + (long long)c[1] * nx + (long long)c[2] * nxy;
        const long long li = MR ? lin - (long long)a.grid.koff * nxy : lin;
        if ((!MR || (c[2] >= a.zr[0] && c[2] < a.zr[1])) && a.d.weight[li] > 0.f) {
            const float gr[3] = {a.d.g[0][li], a.d.g[1][li], a.d.g[2][li]};
            float gn[3]; normalized3(gr, gn);
            float loc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) loc[k] = (uo[k] + t * uw[k]) - ((float)c[k] + 0.5f);
            const float phi0 = a.d.dist[li] + a.grid.vs * dot3(gn, loc);
            if (phi0 <= 0.f) { t_hit = t; lin_hit = lin; return true; }
            const float s = a.grid.vs * dot3(gn, uw);
            if (s < 0.f) {
                const float th = t - phi0 / s;
                if (th <= te) { t_hit = th; lin_hit = lin; return true; }
            }
        }
        c[ax] += step[ax];
        if (c[ax] < lo[ax] || c[ax] >= hi[ax]) return false;
        t = fmaxf(t, te);
    }
    return false;
}

}  // namespace psg
