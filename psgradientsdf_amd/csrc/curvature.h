// curvature.h -- the launchers of curvature.hip (psgsdf_curvature_voxels, psgsdf_extract_mesh_curvature, psgsdf_bake_lod_curvature:
// include/psgsdf_curvature.h; DESIGN.md "Surface curvature"), called from extract_curvature.hip.
#pragma once
#include "engine.h"

namespace psg {

// the dense planes the stencil reads (a single-rank context: local plane 0 is global plane 0) and the voxel size
struct CurvGrid { const float* dist; const float* weight; int nx, ny, nz; float vs; };

// per entry of lin [n] (any value: the range is checked before any load): valid [n], mean, gauss, k1, k2 [n], dir1 [n][3]
void launch_curv_voxels(const CurvGrid& c, const long long* lin, long long n, unsigned char* valid, float* mean, float* gauss, float* k1, float* k2, float* dir1, hipStream_t s);
// per vertex of the welded mesh (g, num, n_verts: as launch_wmesh_verts takes them): v_valid [n_verts] (valid end voxels), the four scalars [n_verts]
void launch_wmesh_curv(const CurvGrid& c, const WMeshGrid& g, const int* num, int n_verts, unsigned char* v_valid, float* v_mean, float* v_gauss, float* v_k1, float* v_k2, hipStream_t s);
// per texel of a bake's voxel plane [n] (-1: no hit): mean [n], valid [n]
void launch_bake_curv(const CurvGrid& c, const int* voxel, long long n, float* mean, unsigned char* valid, hipStream_t s);

}  // namespace psg
