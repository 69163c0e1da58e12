// occlusion.hip -- ambient occlusion of the reconstructed surface (include/psgsdf_occlusion.h):
//   k_occlusion<BAKE>   one lane per ray, K = 8 / 16 / 32 / 64 rays per sample, so a wavefront covers 64 / K consecutive samples.  Every lane sets its
//            sample up itself (see below), turns direction i of the host's table into the sample's frame in double and walks it through the
//            renderer's own cells (render_trace.h) with the walk cut at the radius.  A sample's mask is the wavefront's ballot of `occluded` shifted
//            down to the sample's K lanes: no loop over rays, no reduction, no LDS.  Plain stores by the sample's first lane; the four counts as
//            integer atomics of one lane per wavefront (integers: the same totals in whatever order).  Launched in chunks of 2^30 rays.
//   Two sample providers feed the one traced body: BAKE = false the caller's points and normals, BAKE = true the texels of a bake's atlas, set up
//   again from the bake's own planes and the level-of-detail mesh (bake.h bake_sample: k_bake's arithmetic).
//   Set-up per lane, not per sample: the K lanes of a sample run the same instructions on the same addresses, which costs the SIMD what one lane
//   would (the others would idle) and the memory system one request; handing the nine doubles of (q, m) from a first lane to the others would add
//   eighteen cross-lane moves and save nothing.
#include "device_common.h"
#include "render_trace.h"
#include "bake.h"
#include "occlusion.h"

namespace psg {

// the sample of point j: false if one of its six floats is not finite or the normal is zero
__device__ __forceinline__ bool occlusion_point(const OcclusionArgs& a, long long j, double* q, double* m) {
#pragma clang fp contract(off)
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = a.pts[3 * j + k], y = a.pts_n[3 * j + k];
        finite = finite && isfinite(x) && isfinite(y);
        q[k] = (double)x; m[k] = (double)y;
    }
    return finite && bake_unit(m);
}

// the sample of texel j of the atlas, from the bake's planes; owned: not padding.  false: padding, or an owned texel without a ray
__device__ __forceinline__ bool occlusion_texel(const OcclusionArgs& a, long long j, double* q, double* m, bool& owned) {
#pragma clang fp contract(off)
    const int f = a.face[j];
    owned = f >= 0;
    if (!owned) return false;
    const int R = a.res, B = R + 1;
    const int Y = (int)(j / a.W), X = (int)(j - (long long)Y * a.W);
    const int li = X % B, lj = Y % B;
    const bool even = !(f & 1);
    double w0, w1, w2, p[3], n[3];
    int v0, v1, v2;
    if (!bake_sample(a.xyz, a.nrm, a.faces, f, even ? li : R - li, even ? lj : R - lj, R, w0, w1, w2, v0, v1, v2, p, n)) return false;
    if (a.voxel[j] >= 0) {      // a hit texel: the point on the reconstructed surface and the normal stored there
        const double d = (double)a.disp[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] = p[k] + d * n[k]; m[k] = (double)a.normal[3 * j + k]; }
        if (!bake_unit(m)) { m[0] = n[0]; m[1] = n[1]; m[2] = n[2]; }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] = p[k]; m[k] = n[k]; }
    }
    return true;
}

template <bool BAKE>
__global__ void __launch_bounds__(64) k_occlusion(OcclusionArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long g = a.g0 + (long long)blockIdx.x * 64 + lane;      // the ray
    const long long j = g >> a.log2K;                           // its sample
    const int i = (int)(g & (a.K - 1));                         // its direction
    const bool live = j < a.n;
    bool owned = live, valid = false, occluded = false, buried = false;
    double q[3], m[3];
    if (live) valid = BAKE ? occlusion_texel(a, j, q, m, owned) : occlusion_point(a, j, q, m);
    if (valid) {
        // the frame of m (t1, t2, m); sg + m[2] is never zero
        const double sg = copysign(1.0, m[2]), fa = -1.0 / (sg + m[2]), fb = m[0] * m[1] * fa;
        const double t1[3] = {1.0 + sg * m[0] * m[0] * fa, sg * fb, -sg * m[0]}, t2[3] = {fb, sg + m[1] * m[1] * fa, -m[1]};
        const double D[3] = {a.dirs[3 * i], a.dirs[3 * i + 1], a.dirs[3 * i + 2]};
        float uo[3], uw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double o = q[k] + a.bias * m[k], w = (D[0] * t1[k] + D[1] * t2[k]) + D[2] * m[k];
            uo[k] = (float)(o / a.vs + 0.5); uw[k] = (float)(w / a.vs);
        }
        float t = 0.f; long long lin = -1;
        const bool found = render_trace<false, true>(a.r, uo, uw, t, lin, a.t_max);
        occluded = found && (double)t <= a.radius;
        buried = found && t == 0.f;
    }
    const unsigned long long b_occ = __ballot(occluded), b_bur = __ballot(buried), b_valid = __ballot(valid && i == 0), b_own = __ballot(owned && i == 0);
    if (live && i == 0) {
        const unsigned long long mk = (b_occ >> (lane & ~(a.K - 1))) & (a.K == 64 ? ~0ull : (1ull << a.K) - 1ull);
        const int c = __popcll(mk);
        a.mask[j] = mk;
        a.occ[j] = owned ? (unsigned char)((510 * (a.K - c) + a.K) / (2 * a.K)) : (unsigned char)0;      // floor(255 (K - c) / K + 1/2); padding: 0
    }
    if (lane == 0) {
        if (b_own) atomicAdd(a.counts + AO_SAMPLES, (unsigned long long)__popcll(b_own));
        if (b_valid) atomicAdd(a.counts + AO_VALID, (unsigned long long)__popcll(b_valid));
        if (b_occ) atomicAdd(a.counts + AO_OCCLUDED, (unsigned long long)__popcll(b_occ));
        if (b_bur) atomicAdd(a.counts + AO_BURIED, (unsigned long long)__popcll(b_bur));
    }
}

// A dispatch counts its work-items in 32 bits, and K rays per sample pass that where one lane per sample never would (a 16384^2 atlas at K = 16):
// the rays go out in launches of at most kOcclusionChunk (a multiple of 64 and of every K, so no sample and no wavefront straddles two launches).
hipError_t launch_occlusion(OcclusionArgs a, bool bake, hipStream_t s) {
    const long long rays = a.n * a.K;
    for (a.g0 = 0; a.g0 < rays; a.g0 += kOcclusionChunk) {
        const unsigned blocks = (unsigned)((std::min(rays - a.g0, kOcclusionChunk) + 63) / 64);
        if (bake) hipLaunchKernelGGL(k_occlusion<true>, dim3(blocks), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_occlusion<false>, dim3(blocks), dim3(64), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace psg
