// photo.h -- the launcher of photo.hip (psgsdf_bake_lod_photo: include/psgsdf_photo.h; DESIGN.md "Photometric albedo texture"), called from
// extract_bake.hip.
#pragma once
#include "engine.h"
#include <algorithm>

namespace psg {

enum { PH_SAMPLES = 0, PH_USED, PH_OUTSIDE, PH_GRAZING, PH_OCCLUDED, PH_BURIED, PH_DARK, PH_SOLVED, kPhotoCounts };
enum { PHOTO_USED = 0, PHOTO_OUTSIDE = 1, PHOTO_GRAZING = 2, PHOTO_OCCLUDED = 3, PHOTO_DARK = 4, PHOTO_NO_SAMPLE = 255 };      // psgsdf_photo.h's status bytes
// (texel, keyframe) pairs of one pass = status bytes the pair kernel hands to the solve kernel.  The caller's status plane holds at most 2^30 of
// them (include/psgsdf_photo.h) and is filled in one pass; without one the bytes live in a scratch buffer of at most kPhotoScratch bytes and the
// atlas goes through in ranges of kPhotoScratch / F texels (at least 2^28 / 640 = 419430 texels a pass).  Either way a pass's pairs fit 32 bits.
constexpr long long kPhotoChunk = 1ll << 30;
constexpr long long kPhotoScratch = 1ll << 28;

struct PhotoArgs {
    RenderArgs r;                        // the renderer's prepared state (the walk) and the context's frames
    ImgSrc im; Cam cam; Robust rob;      // the energy's keyframe stack, camera and loss (engine.hip make_args)
    int F, model;
    double bias, cos_min, vs;
    float shade_min;
    double origin[3];                    // psgsdf_info.origin widened: mesh frame + origin = world frame
    const float* xyz; const float* nrm; const int* faces;      // the level-of-detail mesh and the bake's planes (device)
    int res, W;
    const unsigned char* albedo;         // [H][W][3]
    const float* normal;                 // [H][W][3]
    const float* disp;                   // [H][W]
    const int* voxel; const int* face;   // [H][W]
    long long n;                         // W H texels
    long long j0; unsigned nr;           // this pass: texels [j0, j0 + nr) (photo_pass)
    unsigned char* status;               // the byte of (frame f, texel j) is status[f * stride + (j - base)]
    long long stride, base;              // the caller's plane: n, 0; the scratch buffer: the pass's nr, j0 (photo_pass)
    bool scratch;
    float* photo;                        // [H][W][3]
    unsigned char* photo_rgb;            // [H][W][3]
    int* n_obs;                          // [H][W]
    unsigned long long* counts;          // [kPhotoCounts], zeroed
};
// texels of one pass: all of them into the caller's plane, kPhotoScratch / F into the scratch buffer
inline long long photo_pass_texels(long long n, int F, bool scratch) { return scratch ? std::max<long long>(1, std::min(n, kPhotoScratch / F)) : n; }
// the pass that starts at texel j0 (j0, nr and, for the scratch buffer, stride and base); then its two launches, pairs before solve, each checked
void photo_pass(PhotoArgs& a, long long j0);
hipError_t launch_photo_pairs(const PhotoArgs& a, hipStream_t s);
hipError_t launch_photo_solve(const PhotoArgs& a, hipStream_t s);

}  // namespace psg
