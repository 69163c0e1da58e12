// photo.hip -- an albedo texture of the level-of-detail mesh solved from the keyframes at texel resolution (include/psgsdf_photo.h):
//   k_photo_pairs<MODEL>       one lane per (texel, keyframe) pair of a pass, the texel running fastest: the lanes of a wavefront are neighbouring
//            texels of one atlas row -- points next to each other on one coarse triangle -- seen from ONE keyframe, so their rays towards the camera
//            start in neighbouring cells and run nearly parallel (a lane per texel with the frame loop inside would leave a wavefront waiting for
//            its longest walker in every one of F rounds).  Every lane sets its texel up again from the bake's planes (bake.h bake_sample: k_bake's
//            arithmetic; neighbouring lanes read the same face's vertices), projects it with the energy's project, tests the angle, walks relight's
//            point-light ray towards the camera centre through the renderer's cells (render_trace.h, cut at the camera) and shades it with
//            rendered<MODEL>: steps 1 to 4 of the definition, whose outcome is ONE byte, stored at [frame][texel] (coalesced).
//   k_photo_solve<MODEL, IMG>  one thread per texel of the pass: the frames in ascending order -- the definition's summation order -- and for those
//            whose byte says USED the projection and shading again (the same functions on the same inputs: the same bits), the energy's bilinear
//            sample, the robust weight and the two sums in double; then the quotient, its byte and the count.  Plain stores.  The statuses are
//            counted here, from the bytes, per wavefront (integer atomics of one lane: the same totals in whatever order); only `buried`, which no
//            byte carries, is counted by the pair kernel.
//   The frame records are staged in LDS by both (load_frames: F * 96 B; at F = 640 two workgroups a CU, at the bench's F = 50 the registers of the
//   walk decide).  No float atomics.
#include "device_common.h"
#include "render_trace.h"
#include "bake.h"
#include "photo.h"

namespace psg {

struct PhotoSample { double q[3], m[3], xw[3]; float nf[3], xs[3]; };

// the sample of texel j of the atlas, from the bake's planes; false: the texel has none (padding, missed, buried)
__device__ __forceinline__ bool photo_texel(const PhotoArgs& a, long long j, PhotoSample& s) {
#pragma clang fp contract(off)
    const int f = a.face[j];
    if (f < 0 || a.voxel[j] < 0) return false;
    const int R = a.res, B = R + 1;
    const int Y = (int)(j / a.W), X = (int)(j - (long long)Y * a.W);
    const int li = X % B, lj = Y % B;
    const bool even = !(f & 1);
    double w0, w1, w2, p[3], n[3];
    int v0, v1, v2;
    if (!bake_sample(a.xyz, a.nrm, a.faces, f, even ? li : R - li, even ? lj : R - lj, R, w0, w1, w2, v0, v1, v2, p, n)) return false;      // (a hit texel had a ray)
    const double d = (double)a.disp[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) { s.q[k] = p[k] + d * n[k]; s.nf[k] = a.normal[3 * j + k]; s.m[k] = (double)s.nf[k]; }
    if (!bake_unit(s.m)) { s.m[0] = n[0]; s.m[1] = n[1]; s.m[2] = n[2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { s.xw[k] = s.q[k] + a.origin[k]; s.xs[k] = (float)s.xw[k]; }
    return true;
}

// the SH basis of the texel's stored normal (k_band_fit's call) and the shading of frame fp at pr under albedo (1, 1, 1)
template <int MODEL> __device__ __forceinline__ void photo_basis(const float* nf, float* shb) {
    constexpr int NB = ModelTraits<MODEL>::NB;
    if (!ModelTraits<MODEL>::LED) SH<NB == 3 ? 4 : NB>(nf, shb);
}
template <int MODEL> __device__ __forceinline__ void photo_shade(const FrameP& fp, const Proj& pr, const float* nf, const float* shb, float* sh) {
    const float one[3] = {1.f, 1.f, 1.f};
    rendered<MODEL>(fp, pr, nf, shb, one, sh);
}

template <int MODEL>
__global__ void __launch_bounds__(kBlock) k_photo_pairs(PhotoArgs a) {
#pragma clang fp contract(off)
    FrameP* sf = reinterpret_cast<FrameP*>(psg_dyn_smem);   // F records, dynamic LDS
    load_frames(sf, a.r.frames, a.F);
    const unsigned g = blockIdx.x * (unsigned)kBlock + threadIdx.x;      // the pair (a pass has at most 2^30)
    const bool live = g < a.nr * (unsigned)a.F;
    const unsigned f = live ? g / a.nr : 0u, jj = g - f * a.nr;
    const long long j = a.j0 + (long long)jj;
    int st = PHOTO_NO_SAMPLE;
    bool buried = false;
    PhotoSample s;
    if (live && photo_texel(a, j, s)) {
        const FrameP& fp = frame_at(sf, (int)f);
        const Proj pr = project(s.xs, fp, a.cam);
        double wc[3], t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { t[k] = (double)fp.t[k]; wc[k] = t[k] - s.xw[k]; }
        const double lc = sqrt((wc[0] * wc[0] + wc[1] * wc[1]) + wc[2] * wc[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) wc[k] /= lc;
        const double cosv = (s.m[0] * wc[0] + s.m[1] * wc[1]) + s.m[2] * wc[2];
        if (!(pr.p[2] > 0.f && pr.ok)) st = PHOTO_OUTSIDE;
        else if (!(cosv > a.cos_min)) st = PHOTO_GRAZING;
        else {
            double o[3], d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[k] = s.q[k] + a.bias * s.m[k]; d[k] = (t[k] - a.origin[k]) - o[k]; }
            const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            bool occluded = false;
            if (len > 0.0) {      // (the camera centre in the ray's origin: not occluded)
                float t_max = (float)len;      // rounded up if the conversion rounded down: no hit in front of the camera is cut off
                if ((double)t_max < len) t_max = nextafterf(t_max, INFINITY);
                float uo[3], uw[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { uo[k] = (float)(o[k] / a.vs + 0.5); uw[k] = (float)((d[k] / len) / a.vs); }
                float th = 0.f; long long lin = -1;
                const bool found = render_trace<false, true>(a.r, uo, uw, th, lin, t_max);
                occluded = found && (double)th <= len;
                buried = occluded && th == 0.f;
            }
            if (occluded) st = PHOTO_OCCLUDED;
            else {
                float shb[kMaxBasis], sh[3];
                photo_basis<MODEL>(s.nf, shb);
                photo_shade<MODEL>(fp, pr, s.nf, shb, sh);
                st = (sh[0] >= a.shade_min && sh[1] >= a.shade_min && sh[2] >= a.shade_min) ? PHOTO_USED : PHOTO_DARK;
            }
        }
    }
    if (live) a.status[(long long)f * a.stride + (j - a.base)] = (unsigned char)st;
    const unsigned long long b_bur = __ballot(buried);
    if ((threadIdx.x & 63) == 0 && b_bur) atomicAdd(a.counts + PH_BURIED, (unsigned long long)__popcll(b_bur));
}

__device__ __forceinline__ int wave_sumi(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;      // (lane 0 holds the total)
}

template <int MODEL, int IMG>
__global__ void __launch_bounds__(kBlock) k_photo_solve(PhotoArgs a) {
#pragma clang fp contract(off)
    FrameP* sf = reinterpret_cast<FrameP*>(psg_dyn_smem);   // F records, dynamic LDS
    load_frames(sf, a.r.frames, a.F);
    const unsigned jj = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    const bool live = jj < a.nr;
    const long long j = a.j0 + (long long)jj;
    int cnt[5] = {0, 0, 0, 0, 0};      // USED .. DARK
    bool has = false;
    if (live) {
        PhotoSample s;
        has = photo_texel(a, j, s);
        unsigned char byte[3];
        double a0[3], num[3] = {0.0, 0.0, 0.0}, den[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) { byte[c] = a.albedo[3 * j + c]; a0[c] = (double)byte[c] / 255.0; }
        if (has) {
            float shb[kMaxBasis];
            photo_basis<MODEL>(s.nf, shb);
            const unsigned char* st = a.status + (j - a.base);
            for (int f = 0; f < a.F; ++f) {
                const int code = st[(long long)f * a.stride];
#pragma unroll
                for (int q = 0; q < 5; ++q) cnt[q] += code == q;      // (no register array indexed by a variable)
                if (code != PHOTO_USED) continue;
                const FrameP& fp = frame_at(sf, f);
                const Proj pr = project(s.xs, fp, a.cam);
                float I[3], sh[3];
                sample<false, IMG>(a.im, f, a.cam, pr.m, pr.n, I, nullptr, nullptr);
                photo_shade<MODEL>(fp, pr, s.nf, shb, sh);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float r = I[c] - (float)a0[c] * sh[c];
                    const float w = robust_weight(a.rob, r);
                    num[c] += ((double)w * (double)sh[c]) * (double)I[c];
                    den[c] += ((double)w * (double)sh[c]) * (double)sh[c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (cnt[PHOTO_USED] > 0 && den[c] > 0.0) ? (float)(num[c] / den[c]) : (float)a0[c];
            a.photo[3 * j + c] = v;
            a.photo_rgb[3 * j + c] = has ? (unsigned char)(int)floorf(255.0f * fminf(fmaxf(v, 0.0f), 1.0f) + 0.5f) : byte[c];
        }
        a.n_obs[j] = cnt[PHOTO_USED];
    }
    const int totals[kPhotoCounts] = {has ? 1 : 0, cnt[PHOTO_USED], cnt[PHOTO_OUTSIDE], cnt[PHOTO_GRAZING], cnt[PHOTO_OCCLUDED], 0, cnt[PHOTO_DARK], cnt[PHOTO_USED] > 0 ? 1 : 0};
#pragma unroll
    for (int q = 0; q < kPhotoCounts; ++q) {
        if (q == PH_BURIED) continue;
        const int t = wave_sumi(totals[q]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(a.counts + q, (unsigned long long)t);
    }
}

// the solve kernel over the shading models x {float taps at 32-bit offsets, RGBA8 words, the source decides}; the loss is read at run time
#define PSG_LAUNCH_PHOTO_SOLVE(IMG_) do { \
        if (a.model == 0) hipLaunchKernelGGL((k_photo_solve<0, IMG_>), dim3(blocks), dim3(kBlock), lds, s, a); \
        else if (a.model == 1) hipLaunchKernelGGL((k_photo_solve<1, IMG_>), dim3(blocks), dim3(kBlock), lds, s, a); \
        else hipLaunchKernelGGL((k_photo_solve<2, IMG_>), dim3(blocks), dim3(kBlock), lds, s, a); } while (0)

void photo_pass(PhotoArgs& a, long long j0) {
    a.j0 = j0;
    a.nr = (unsigned)std::min(photo_pass_texels(a.n, a.F, a.scratch), a.n - j0);
    if (a.scratch) { a.stride = (long long)a.nr; a.base = j0; }
}
hipError_t launch_photo_pairs(const PhotoArgs& a, hipStream_t s) {
    const size_t lds = (size_t)a.F * sizeof(FrameP);
    const unsigned blocks = (unsigned)(((long long)a.nr * a.F + kBlock - 1) / kBlock);
    if (a.model == 0) hipLaunchKernelGGL(k_photo_pairs<0>, dim3(blocks), dim3(kBlock), lds, s, a);
    else if (a.model == 1) hipLaunchKernelGGL(k_photo_pairs<1>, dim3(blocks), dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL(k_photo_pairs<2>, dim3(blocks), dim3(kBlock), lds, s, a);
    return hipGetLastError();
}
hipError_t launch_photo_solve(const PhotoArgs& a, hipStream_t s) {
    const size_t lds = (size_t)a.F * sizeof(FrameP);
    const unsigned blocks = (a.nr + kBlock - 1) / kBlock;
    const int img = a.im.u8 ? 1 : (a.im.idx32 ? 0 : -1);
    if (img == 0) PSG_LAUNCH_PHOTO_SOLVE(0);
    else if (img == 1) PSG_LAUNCH_PHOTO_SOLVE(1);
    else PSG_LAUNCH_PHOTO_SOLVE(-1);
    return hipGetLastError();
}

}  // namespace psg
