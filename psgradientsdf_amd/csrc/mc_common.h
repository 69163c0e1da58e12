// mc_common.h -- what the two marching-cubes passes share (extract.hip psgsdf_extract_mesh, mesh.hip psgsdf_extract_mesh_indexed): the classic
// table, the corner / edge numbering of the host's marching_cubes.hpp and the reference's edge interpolation.  FMA contraction is off for every
// file that includes it: the vertices must be the host writer's, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace psg {
namespace {

__constant__ signed char kTri[256][16] = {
#include "../host/mc_tritable.inc"
};
__constant__ int kCornerD[8][3] = {{1, 1, 0}, {1, 0, 0}, {0, 0, 0}, {0, 1, 0}, {1, 1, 1}, {1, 0, 1}, {0, 0, 1}, {0, 1, 1}};      // marching_cubes.hpp kCorner (computeLutIndex :511-556)
__constant__ int kEdgeD[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

// MarchingCubes.cpp:559-579 (marching_cubes.hpp interpolate)
__device__ __forceinline__ void mc_interp(float t0, float t1, const float* v0, const float* v1, float* out) {
    const float iso = 0.0f;
    if ((double)fabsf(iso - t0) < 1e-7) { for (int a = 0; a < 3; ++a) out[a] = v0[a]; return; }
    if ((double)fabsf(iso - t1) < 1e-7) { for (int a = 0; a < 3; ++a) out[a] = v1[a]; return; }
    if ((double)fabsf(t0 - t1) < 1e-7) { for (int a = 0; a < 3; ++a) out[a] = v0[a]; return; }
    double mu = (double)((iso - t0) / (t1 - t0));
    if (mu > 1.0) mu = 1.0; else if (mu < 0) mu = 0.0;
    for (int a = 0; a < 3; ++a) out[a] = (float)((double)v0[a] + mu * (double)(v1[a] - v0[a]));
}

}  // namespace
}  // namespace psg
