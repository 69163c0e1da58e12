// occlusion.h -- the launchers of occlusion.hip (psgsdf_occlusion_points, psgsdf_bake_lod_ao: include/psgsdf_occlusion.h; DESIGN.md "Ambient
// occlusion"), called from extract_bake.hip.
#pragma once
#include "engine.h"

namespace psg {

enum { AO_SAMPLES = 0, AO_VALID, AO_OCCLUDED, AO_BURIED, kAoCounts };
constexpr long long kOcclusionChunk = 1ll << 30;      // rays per launch (a dispatch's work-items are a 32-bit count)

struct OcclusionArgs {
    RenderArgs r;                        // the renderer's prepared state: dense planes, grid, brick map and box (nothing of a view or of the band is read)
    int K, log2K;                        // rays per sample: 8, 16, 32 or 64
    long long n;                         // samples: points, or the atlas's W H texels
    long long g0;                        // the first ray of this launch (set by the launcher)
    double radius, bias, vs;
    float t_max;                         // the walk's cut: (float) radius, rounded up (FLT_MAX: no cut)
    const double* dirs;                  // [K][3]
    // the samples of psgsdf_occlusion_points
    const float* pts; const float* pts_n;      // [n][3]
    // the samples of psgsdf_bake_lod_ao: the level-of-detail mesh and the bake's planes (device)
    const float* xyz; const float* nrm; const int* faces;
    int res, W;
    const float* normal;                 // [H][W][3]
    const float* disp;                   // [H][W]
    const int* voxel; const int* face;   // [H][W]
    unsigned long long* mask;            // [n]
    unsigned char* occ;                  // [n]
    unsigned long long* counts;          // [kAoCounts], zeroed
};
// bake: the texels' provider, else the points'.  Every launch is checked: the first error is returned
hipError_t launch_occlusion(OcclusionArgs a, bool bake, hipStream_t s);

}  // namespace psg
