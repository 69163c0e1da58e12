// fill.h -- the launchers of fill.hip (psgsdf_fill_voxels, psgsdf_extract_mesh_filled: include/psgsdf_fill.h; DESIGN.md "Hole filling"), called
// from extract_fill.hip.
#pragma once
#include "engine.h"

namespace psg {

constexpr int kFillVals = 7;      // floats per voxel the filling defines: dist, grad[3], rgb[3]

// the eight float planes of a volume (a single-rank context: local plane 0 is global plane 0)
struct FillPlanes { float* dist; float* g[3]; float* weight; float* rho[3]; };

// what the front rounds work on.  weight0 is the context's own weight plane, the observed set, which nothing here writes; w is the call's working
// copy of the context's planes, which the rounds extend in place; round [nvox] holds 0 or the round a voxel was filled in.  A launch covers the
// box [lo, lo + d) of the grid.
struct FillGrid {
    const float* weight0; FillPlanes w; unsigned char* round;
    int nx, ny, nz; float vs;
    int lo[3], d[3];
};

constexpr int kFillBoxBlocks = 2048;      // workgroups of the box reduction at most: part holds 6 ints per workgroup + 6
// box[0..2] / box[3..5] = min / max voxel index over weight > 0 (min > max: no such voxel)
void launch_fill_box(const float* weight, int nx, int ny, long long nvox, int* part, int* box, hipStream_t s);
// round r over g's box: the voxels outside Known_{r-1} with a neighbour in it get their values, weight 1 and round r
void launch_fill_round(const FillGrid& g, int r, hipStream_t s);
// flag[c] = 1 iff box cell c is filled
void launch_fill_flags(const FillGrid& g, int* flag, hipStream_t s);
// offs: the exclusive scan of the flags; per filled voxel q (ascending lin): lin, round, the seven values val[a n + q] from w, and its neighbours
// nb[e n + q] in the neighbour order: -1 none or unknown, v >= 0 the observed voxel v, -2 - p the filled voxel p of this list
void launch_fill_list(const FillGrid& g, const int* offs, int n, long long* lin, unsigned char* round, int* nb, float* val, hipStream_t s);
// one Jacobi sweep over the list: out from in (filled neighbours) and w (observed neighbours)
void launch_fill_sweep(const FillPlanes& w, const int* nb, int n, const float* in, float* out, hipStream_t s);
// grad [n][3], rgb [n][3] from val (dist [n] is val's first plane as it is)
void launch_fill_pack(const float* val, int n, float* grad, float* rgb, hipStream_t s);
// the list's values into the working copy
void launch_fill_scatter(const FillPlanes& w, const long long* lin, int n, const float* val, hipStream_t s);
// per vertex of the welded mesh (g, num, n_verts: as launch_wmesh_verts takes them) the number of its key's end voxels with round != 0, written at
// the vertex's number, or -- keep != nullptr: the exclusive scan of the kept-vertex flags, n_kept their sum -- at its number among the kept ones
void launch_wmesh_filled(const WMeshGrid& g, const int* num, int n_verts, const unsigned char* round, const int* keep, int n_kept, unsigned char* out, hipStream_t s);

}  // namespace psg
