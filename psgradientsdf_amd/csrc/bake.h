// bake.h -- the launcher of bake.hip (psgsdf_bake_lod, include/psgsdf_bake.h; DESIGN.md "Baked detail maps"), called from extract_bake.hip, and the
// texel's sample as a device function.
#pragma once
#include "engine.h"

namespace psg {

enum { BK_OWNED = 0, BK_HITS, BK_OFF_BAND, BK_BURIED, kBakeCounts };
constexpr int kBakeMaxSide = 16384;      // the atlas is at most this wide and high

struct BakeArgs {
    RenderArgs r;                        // the renderer's prepared state: dense planes, Band::vp, grid, brick map and box (nothing of a view is read)
    int has_band;                        // 0: no band exists (row_of is not read: every hit is off-band)
    const float* xyz; const float* nrm; const unsigned char* rgb; const int* faces; int nf;      // the level-of-detail mesh (device)
    int res, bpr, nblk, W, H;            // R, blocks per atlas row, blocks, atlas size
    double reach, vs;
    unsigned char* albedo;               // [H][W][3]
    float* normal;                       // [H][W][3]
    float* disp;                         // [H][W]
    int* voxel; int* face;               // [H][W]
    unsigned long long* counts;          // [kBakeCounts], zeroed
};
void launch_bake(const BakeArgs& a, hipStream_t s);

// v / |v| in double; false (and v untouched) if |v| is zero
__device__ __forceinline__ bool bake_unit(double* v) {
#pragma clang fp contract(off)
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(len > 0.0)) return false;
    v[0] /= len; v[1] /= len; v[2] /= len;
    return true;
}

// The sample of texel (ta, tb) of face f (include/psgsdf_bake.h "Sample"): the weights, the face's vertices, the point p and the unit normal n.
// false: no normal can be had (n is zero).  One copy for k_bake and for the kernel that starts again from its planes (occlusion.hip).
__device__ __forceinline__ bool bake_sample(const float* xyz, const float* nrm, const int* faces, int f, int ta, int tb, int R, double& w0, double& w1, double& w2,
                                            int& v0, int& v1, int& v2, double* p, double* n) {
#pragma clang fp contract(off)
    w1 = (3.0 * ta + 1.0) / (3.0 * (R + 1)); w2 = (3.0 * tb + 1.0) / (3.0 * (R + 1)); w0 = 1.0 - w1 - w2;
    v0 = faces[3 * (size_t)f]; v1 = faces[3 * (size_t)f + 1]; v2 = faces[3 * (size_t)f + 2];
    double x0[3], x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x0[k] = (double)xyz[3 * (size_t)v0 + k]; x1[k] = (double)xyz[3 * (size_t)v1 + k]; x2[k] = (double)xyz[3 * (size_t)v2 + k];
        p[k] = (w0 * x0[k] + w1 * x1[k]) + w2 * x2[k];
        n[k] = (w0 * (double)nrm[3 * (size_t)v0 + k] + w1 * (double)nrm[3 * (size_t)v1 + k]) + w2 * (double)nrm[3 * (size_t)v2 + k];
    }
    bool ray = bake_unit(n);
    if (!ray) {      // the vertex normals cancel: the triangle's own
        const double e1[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, e2[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]};
        n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        ray = bake_unit(n);
        if (!ray) { n[0] = 0.0; n[1] = 0.0; n[2] = 0.0; }
    }
    return ray;
}

}  // namespace psg
