// bake.h -- the launcher of bake.hip (psgsdf_bake_lod, include/psgsdf_bake.h; DESIGN.md "Baked detail maps"), called from extract_mesh.hip.
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

}  // namespace psg
