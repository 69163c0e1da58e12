// fit.hip -- the photometric fit of the reconstruction resolved over the surface (include/psgsdf_fit.h; DESIGN.md "Photometric fit per voxel and vertex"):
//   k_band_fit   one thread per band row: k_energy's loop (sweeps.hip) -- the visible frames in ascending order, project, sample, rendered<MODEL>,
//                robust_loss -- with the row's sums STORED instead of reduced: the counted observations, the robust loss in k_energy's accumulator
//                (obs_acc_t, widened to double) and the float sum of squared residuals per channel.  24 B of plain stores per row; it folds nothing,
//                writes no partial slot and touches no mailbox, so an optimisation step before or after it runs as if it had not been launched.
//   k_wmesh_fit  one thread per key slot of the welded mesh (engine.h WMeshGrid, next to mesh.hip k_wmesh_verts): the sums of the vertex's end voxels
//                -- found through the dense voxel-to-row map; an end voxel outside the band contributes nothing -- and from them the observation count,
//                the rms residual and the mean robust loss of the vertex, in double.
// No atomics: the same bytes on every call.
#include "device_common.h"

namespace psg {

template <int MODEL, int LOSS, int IMG>
__global__ void __launch_bounds__(kBlock) k_band_fit(SweepArgs a, int* __restrict__ n_obs, double* __restrict__ loss, float* __restrict__ sum_r2) {
    constexpr int NB = ModelTraits<MODEL>::NB;
    FrameP* sf = reinterpret_cast<FrameP*>(psg_dyn_smem);   // F records, dynamic LDS
    load_frames(sf, a.frames, a.F);
    const Band& b = a.b;
    const int j = a.row0 + vm_bid(a, 2, true) * blockDim.x + threadIdx.x;      // (k_energy's rows per workgroup: the same gathers meet in the same L2)
    if (j >= a.row1) return;
    Vox v; load_vox(b, j, v);
    float shfd[kMaxBasis];
    if (!ModelTraits<MODEL>::LED) SH<NB == 3 ? 4 : NB>(v.nfd, shfd);
    obs_acc_t Ef = 0; float s2[3] = {0.f, 0.f, 0.f}; int n = 0;
    FOR_EACH_VISIBLE_FRAME(b, j, a.F, f) {
        const FrameP& fp = frame_at(sf, f);
        Proj pr = project(v.xs, fp, a.cam);
        if (!pr.ok) continue;
        float I[3], ren[3];
        sample<false, IMG>(a.im, f, a.cam, pr.m, pr.n, I, nullptr, nullptr);
        rendered<MODEL>(fp, pr, v.nfd, shfd, v.rho, ren);
        float l = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { const float r = I[ch] - ren[ch]; l += robust_loss<LOSS>(a.rob, r); s2[ch] += r * r; }
        Ef += (obs_acc_t)l; n += 1;
    }
    const size_t o = (size_t)(j - a.row0);
    n_obs[o] = n; loss[o] = (double)Ef;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sum_r2[3 * o + ch] = s2[ch];
}
void launch_band_fit(const SweepArgs& a, int* n_obs, double* loss, float* sum_r2, hipStream_t s) {
    if (a.row1 <= a.row0) return;
    dim3 g((a.row1 - a.row0 + kBlock - 1) / kBlock), bl(kBlock);
    PSG_LAUNCH_SWEEP(k_band_fit, a, false, g, bl, a.F * sizeof(FrameP), s, a, n_obs, loss, sum_r2);
}

// Key slot s = 4 * ((kz * d1 + j) * d0 + i) + type of the crop voxel (i, j, kz + zc0): the vertex on its +x / +y / +z edge (type 0, 1, 2: end voxels the
// voxel and that neighbour) or the voxel itself as a snapped corner (type 3: one end).  num: the exclusive scan of the used-key flags, as k_wmesh_verts
// reads it.  The fit arrays hold the band rows [row0, row1).
__global__ void __launch_bounds__(kBlock) k_wmesh_fit(WMeshGrid g, const int* __restrict__ num, int n_verts, const int* __restrict__ row_of, int row0, int row1,
                                                       const int* __restrict__ n_obs, const double* __restrict__ loss, const float* __restrict__ sum_r2,
                                                       int* __restrict__ v_n, float* __restrict__ v_rms, float* __restrict__ v_loss) {
#pragma clang fp contract(off)
    const long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (s >= g.nown) return;
    const int v = num[s];
    if ((s + 1 < g.nown ? num[s + 1] : n_verts) == v) return;      // an unused key
    const int type = (int)(s & 3), q = (int)(s >> 2);
    const int i = q % g.d[0], j = (q / g.d[0]) % g.d[1], k = q / (g.d[0] * g.d[1]) + g.zc0;
    int n = 0; double L = 0.0, Q = 0.0;
    for (int e = 0; e < (type == 3 ? 1 : 2); ++e) {
        const int pi = i + (e && type == 0), pj = j + (e && type == 1), pk = k + (e && type == 2);
        const long long lin = (long long)(pk + g.lo[2] - g.zlo) * g.nx * g.ny + (long long)(pj + g.lo[1]) * g.nx + (pi + g.lo[0]);
        const int r = row_of[lin];
        if (r < row0 || r >= row1) continue;      // (-1: not a band row)
        const size_t o = (size_t)(r - row0);
        n += n_obs[o]; L += loss[o];
        Q += (double)sum_r2[3 * o]; Q += (double)sum_r2[3 * o + 1]; Q += (double)sum_r2[3 * o + 2];
    }
    v_n[v] = n;
    v_rms[v] = n ? (float)sqrt(Q / (3.0 * (double)n)) : 0.0f;
    v_loss[v] = n ? (float)(L / (double)n) : 0.0f;
}
void launch_wmesh_fit(const WMeshGrid& g, const int* num, int n_verts, const int* row_of, int row0, int row1, const int* n_obs, const double* loss, const float* sum_r2,
                      int* v_n, float* v_rms, float* v_loss, hipStream_t s) {
    const unsigned blocks = (unsigned)std::max<long long>(1, (g.nown + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_wmesh_fit, dim3(blocks), dim3(kBlock), 0, s, g, num, n_verts, row_of, row0, row1, n_obs, loss, sum_r2, v_n, v_rms, v_loss);
}

}  // namespace psg
