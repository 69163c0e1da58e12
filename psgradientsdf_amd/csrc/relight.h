// relight.h -- the launcher of relight.hip (psgsdf_relight: include/psgsdf_relight.h), called from api_render.hip.
#pragma once
#include "engine.h"

namespace psg {

enum { RL_HITS = 0, RL_LIT, RL_OCCLUDED, RL_BURIED, kRelightCounts };
enum { RL_SH = 0, RL_DIRECTIONAL = 1, RL_POINT = 2 };      // psgsdf_light.kind
constexpr long long kRelightChunk = 1ll << 30;      // rays per launch (a dispatch's work-items are a 32-bit count; a multiple of 64 and of every K)

struct RelightArgs {
    RenderArgs r;                        // the view as k_render ran it: prepared state, camera, pose, tiles and the planes depth, normal, albedo, voxel it wrote (device)
    int kind, n_sh;                      // the light
    int K, log2K;                        // rays per lit pixel: 1, 8, 16, 32 or 64 (SH: 1, one lane per pixel and no ray)
    long long g0;                        // the first ray of this launch (set by the launcher)
    float sh[9];
    double vec[3];
    float colour[3], ambient[3];
    double spread, bias, vs;
    double limit;                        // reach, infinity for none
    double origin[3];
    const double* dirs;                  // [K][3]: the occlusion's table (K = 1: one row 0, 0, 1)
    float* out;                          // [4][H][W]: rendered r g b, visibility
    unsigned long long* counts;          // [kRelightCounts], zeroed
};
// one light; every launch is checked: the first error is returned
hipError_t launch_relight(RelightArgs a, hipStream_t s);

}  // namespace psg
