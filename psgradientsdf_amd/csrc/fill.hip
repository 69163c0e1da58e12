// fill.hip -- unobserved voxels filled from their observed neighbours (include/psgsdf_fill.h; DESIGN.md "Hole filling"):
//   k_fill_box_*   the bounding box of the observed set {weight > 0}, in the style of extract.hip's crop box: per-workgroup partials, then one workgroup
//   k_fill_round   round r, one thread per voxel of the observed box grown by r: a voxel outside Known_{r-1} gathers the first-order extensions
//                  d_v + g_v . (x_u - x_v) of its neighbours in Known_{r-1}.  Membership is weight0 > 0 or 0 < round < r: a voxel filled in THIS
//                  launch shows round 0 or r, neither of which passes, so what a thread reads (values of Known_{r-1}) and what any thread writes
//                  (values of voxels outside it) never overlap and ONE working copy is race-free -- no second copy, no publish step
//   k_fill_flags / k_fill_list   the filled voxels compacted in ascending lin (extract.hip scan_counts in between): lin, round, values, and the six
//                  neighbours resolved ONCE into "observed voxel v" / "entry p of this list" / none, so that a sweep needs no grid arithmetic
//   k_fill_sweep   one Jacobi sweep, one thread per list entry: 6 neighbour codes (coalesced), then up to 6 x 7 floats gathered from the working copy
//                  (observed neighbours) or the previous sweep's buffer (filled neighbours), into the other buffer
//   k_fill_pack / k_fill_scatter   the list's values as the call's arrays / back into the working copy, for the mesh stages
//   k_wmesh_filled one thread per key slot of the welded mesh (engine.h WMeshGrid, next to curvature.hip k_wmesh_curv): filled end voxels per vertex
// Double throughout, no contraction, sums in the neighbour order; no atomics, no LDS beyond the box reduction, plain stores: the same bytes on every call.
#pragma clang fp contract(off)
#include "fill.h"
#include <algorithm>

namespace psg {
namespace {

__global__ void __launch_bounds__(kBlock) k_fill_box_part(const float* __restrict__ weight, int nx, int ny, long long nvox, int* __restrict__ part) {
    int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-(1 << 30), -(1 << 30), -(1 << 30)};
    const long long nxy = (long long)nx * ny;
    for (long long lin = blockIdx.x * (long long)blockDim.x + threadIdx.x; lin < nvox; lin += (long long)gridDim.x * blockDim.x) {
        if (!(weight[lin] > 0.f)) continue;
        const int k = (int)(lin / nxy), rest = (int)(lin - (long long)k * nxy), j = rest / nx, i = rest - j * nx;
        lo[0] = min(lo[0], i); hi[0] = max(hi[0], i); lo[1] = min(lo[1], j); hi[1] = max(hi[1], j); lo[2] = min(lo[2], k); hi[2] = max(hi[2], k);
    }
    __shared__ int s[6][kBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int l = lo[a], h = hi[a];
        for (int o = 32; o > 0; o >>= 1) { l = min(l, __shfl_xor(l, o, 64)); h = max(h, __shfl_xor(h, o, 64)); }
        if (lane == 0) { s[a][w] = l; s[3 + a][w] = h; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int v = s[threadIdx.x][0];
        for (int i = 1; i < kBlock / 64; ++i) v = threadIdx.x < 3 ? min(v, s[threadIdx.x][i]) : max(v, s[threadIdx.x][i]);
        part[blockIdx.x * 6 + threadIdx.x] = v;
    }
}
__global__ void __launch_bounds__(kBlock) k_fill_box_final(const int* __restrict__ part, int nblk, int* __restrict__ box) {
    __shared__ int s[6][kBlock];
    int v[6] = {1 << 30, 1 << 30, 1 << 30, -(1 << 30), -(1 << 30), -(1 << 30)};
    for (int b = threadIdx.x; b < nblk; b += blockDim.x)
        for (int a = 0; a < 6; ++a) v[a] = a < 3 ? min(v[a], part[b * 6 + a]) : max(v[a], part[b * 6 + a]);
    for (int a = 0; a < 6; ++a) s[a][threadIdx.x] = v[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        int r = s[threadIdx.x][0];
        for (int i = 1; i < kBlock; ++i) r = threadIdx.x < 3 ? min(r, s[threadIdx.x][i]) : max(r, s[threadIdx.x][i]);
        box[threadIdx.x] = r;
    }
}

// the sums over a voxel's known neighbours, in the neighbour order
struct Acc {
    double d = 0.0, m[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}; int n = 0;
    // one neighbour: its distance (EXT: extended first-order along axis a over the signed step sh = s h), its normalised gradient, its colour
    template <bool EXT> __device__ __forceinline__ void add(float dist, const float g[3], const float rho[3], int a, double sh) {
        const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
        const double z = (gx * gx + gy * gy) + gz * gz;
        double u[3] = {0.0, 0.0, 0.0};
        if (z > 0.0) { const double rt = sqrt(z); u[0] = gx / rt; u[1] = gy / rt; u[2] = gz / rt; }
        d = d + (EXT ? (double)dist - sh * u[a] : (double)dist);
#pragma unroll
        for (int q = 0; q < 3; ++q) { m[q] = m[q] + u[q]; c[q] = c[q] + (double)rho[q]; }
        n += 1;
    }
    // the seven floats of the voxel (n > 0)
    __device__ __forceinline__ void result(float out[kFillVals]) const {
        const double nn = (double)n;
        out[0] = (float)(d / nn);
        const double z = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
        if (z > 0.0) { const double rt = sqrt(z); out[1] = (float)(m[0] / rt); out[2] = (float)(m[1] / rt); out[3] = (float)(m[2] / rt); }
        else { out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; }
#pragma unroll
        for (int q = 0; q < 3; ++q) out[4 + q] = (float)(c[q] / nn);
    }
};

// box cell c of g -> the voxel; false past the box
__device__ __forceinline__ bool box_voxel(const FillGrid& g, long long c, int& i, int& j, int& k) {
    const long long dxy = (long long)g.d[0] * g.d[1];
    if (c >= dxy * g.d[2]) return false;
    const int kl = (int)(c / dxy), rest = (int)(c - (long long)kl * dxy), jl = rest / g.d[0];
    i = rest - jl * g.d[0] + g.lo[0]; j = jl + g.lo[1]; k = kl + g.lo[2];
    return true;
}
// neighbour e of voxel (i, j, k): its axis and sign, and whether it exists
__device__ __forceinline__ bool neighbour(const FillGrid& g, int i, int j, int k, int e, int& a, int& s, long long& off) {
    a = e >> 1; s = (e & 1) ? 1 : -1;
    const int p = (a == 0 ? i : a == 1 ? j : k) + s, n = a == 0 ? g.nx : a == 1 ? g.ny : g.nz;
    off = a == 0 ? (long long)s : a == 1 ? (long long)s * g.nx : (long long)s * g.nx * g.ny;
    return p >= 0 && p < n;
}

__global__ void __launch_bounds__(kBlock) k_fill_round(FillGrid g, int r) {
    int i, j, k;
    if (!box_voxel(g, blockIdx.x * (long long)blockDim.x + threadIdx.x, i, j, k)) return;
    const long long lin = ((long long)k * g.ny + j) * g.nx + i;
    if (g.weight0[lin] > 0.f || g.round[lin] != 0) return;      // in Known_{r-1}
    const double h = (double)g.vs;
    Acc acc;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        int a, s; long long off;
        if (!neighbour(g, i, j, k, e, a, s, off)) continue;
        const long long v = lin + off;
        const int rv = g.round[v];
        if (!(g.weight0[v] > 0.f || (rv != 0 && rv < r))) continue;
        const float gv[3] = {g.w.g[0][v], g.w.g[1][v], g.w.g[2][v]}, cv[3] = {g.w.rho[0][v], g.w.rho[1][v], g.w.rho[2][v]};
        acc.add<true>(g.w.dist[v], gv, cv, a, (double)s * h);
    }
    if (acc.n == 0) return;
    float out[kFillVals]; acc.result(out);
    g.w.dist[lin] = out[0]; g.w.g[0][lin] = out[1]; g.w.g[1][lin] = out[2]; g.w.g[2][lin] = out[3];
    g.w.rho[0][lin] = out[4]; g.w.rho[1][lin] = out[5]; g.w.rho[2][lin] = out[6];
    g.w.weight[lin] = 1.0f;
    g.round[lin] = (unsigned char)r;
}

__global__ void __launch_bounds__(kBlock) k_fill_flags(FillGrid g, int* __restrict__ flag) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    int i, j, k;
    if (!box_voxel(g, c, i, j, k)) return;
    flag[c] = g.round[((long long)k * g.ny + j) * g.nx + i] != 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_fill_list(FillGrid g, const int* __restrict__ offs, int n, long long* __restrict__ lin_out, unsigned char* __restrict__ round_out,
                                                       int* __restrict__ nb, float* __restrict__ val) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    int i, j, k;
    if (!box_voxel(g, c, i, j, k)) return;
    const long long lin = ((long long)k * g.ny + j) * g.nx + i;
    const unsigned char r = g.round[lin];
    if (r == 0) return;
    const int q = offs[c];
    if (q < 0 || q >= n) return;
    lin_out[q] = lin; round_out[q] = r;
    const float v7[kFillVals] = {g.w.dist[lin], g.w.g[0][lin], g.w.g[1][lin], g.w.g[2][lin], g.w.rho[0][lin], g.w.rho[1][lin], g.w.rho[2][lin]};
#pragma unroll
    for (int a = 0; a < kFillVals; ++a) val[(size_t)a * n + q] = v7[a];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        int a, s; long long off;
        int code = -1;
        if (neighbour(g, i, j, k, e, a, s, off)) {
            const long long v = lin + off;
            if (g.weight0[v] > 0.f) code = (int)v;
            else if (g.round[v] != 0) {      // a filled voxel lies in the box: its cell
                const int p[3] = {i + (a == 0 ? s : 0) - g.lo[0], j + (a == 1 ? s : 0) - g.lo[1], k + (a == 2 ? s : 0) - g.lo[2]};
                if (p[0] >= 0 && p[0] < g.d[0] && p[1] >= 0 && p[1] < g.d[1] && p[2] >= 0 && p[2] < g.d[2]) {
                    const int t = offs[((long long)p[2] * g.d[1] + p[1]) * g.d[0] + p[0]];
                    if (t >= 0 && t < n) code = -2 - t;
                }
            }
        }
        nb[(size_t)e * n + q] = code;
    }
}

__global__ void __launch_bounds__(kBlock) k_fill_sweep(FillPlanes w, const int* __restrict__ nb, int n, const float* __restrict__ in, float* __restrict__ out) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    int code[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) code[e] = nb[(size_t)e * n + q];
    Acc acc;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const int cd = code[e];
        if (cd == -1) continue;
        float d, gv[3], cv[3];
        if (cd >= 0) {
            d = w.dist[cd]; gv[0] = w.g[0][cd]; gv[1] = w.g[1][cd]; gv[2] = w.g[2][cd]; cv[0] = w.rho[0][cd]; cv[1] = w.rho[1][cd]; cv[2] = w.rho[2][cd];
        } else {
            const size_t p = (size_t)(-2 - cd), N = (size_t)n;
            d = in[p]; gv[0] = in[N + p]; gv[1] = in[2 * N + p]; gv[2] = in[3 * N + p]; cv[0] = in[4 * N + p]; cv[1] = in[5 * N + p]; cv[2] = in[6 * N + p];
        }
        acc.add<false>(d, gv, cv, 0, 0.0);
    }
    float v7[kFillVals];
    if (acc.n > 0) acc.result(v7);
    else {      // (a filled voxel always has a known neighbour; should it not, it keeps its values)
#pragma unroll
        for (int a = 0; a < kFillVals; ++a) v7[a] = in[(size_t)a * n + q];
    }
#pragma unroll
    for (int a = 0; a < kFillVals; ++a) out[(size_t)a * n + q] = v7[a];
}

__global__ void __launch_bounds__(kBlock) k_fill_pack(const float* __restrict__ val, int n, float* __restrict__ grad, float* __restrict__ rgb) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) { grad[3 * (size_t)q + a] = val[(size_t)(1 + a) * n + q]; rgb[3 * (size_t)q + a] = val[(size_t)(4 + a) * n + q]; }
}

__global__ void __launch_bounds__(kBlock) k_fill_scatter(FillPlanes w, const long long* __restrict__ lin, int n, const float* __restrict__ val) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const long long l = lin[q]; const size_t N = (size_t)n;
    w.dist[l] = val[q]; w.g[0][l] = val[N + q]; w.g[1][l] = val[2 * N + q]; w.g[2][l] = val[3 * N + q];
    w.rho[0][l] = val[4 * N + q]; w.rho[1][l] = val[5 * N + q]; w.rho[2][l] = val[6 * N + q];
}

// Key slot s = 4 * ((kz * d1 + j) * d0 + i) + type of the crop voxel (i, j, kz + zc0), as in curvature.hip k_wmesh_curv; num: the exclusive scan of
// the used-key flags.
__global__ void __launch_bounds__(kBlock) k_wmesh_filled(WMeshGrid g, const int* __restrict__ num, int n_verts, const unsigned char* __restrict__ round, const int* __restrict__ keep,
                                                          int n_kept, unsigned char* __restrict__ out) {
    const long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (s >= g.nown) return;
    const int v = num[s];
    if ((s + 1 < g.nown ? num[s + 1] : n_verts) == v) return;      // an unused key
    int o = v;
    if (keep) {
        o = keep[v];
        if ((v + 1 < n_verts ? keep[v + 1] : n_kept) == o) return;      // a vertex the filter dropped
    }
    const int type = (int)(s & 3), q = (int)(s >> 2);
    const int i = q % g.d[0], j = (q / g.d[0]) % g.d[1], k = q / (g.d[0] * g.d[1]) + g.zc0;
    const long long dl = (long long)(k + g.lo[2] - g.zlo) * g.nx * g.ny + (long long)(j + g.lo[1]) * g.nx + (i + g.lo[0]);
    const int fl = round[dl] != 0 ? 1 : 0;
    int fh = fl;
    if (type != 3) fh = round[dl + (type == 0 ? 1ll : type == 1 ? (long long)g.nx : (long long)g.nx * g.ny)] != 0 ? 1 : 0;
    out[o] = (unsigned char)(fl + fh);
}

unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + kBlock - 1) / kBlock); }
long long box_cells(const FillGrid& g) { return (long long)g.d[0] * g.d[1] * g.d[2]; }

}  // namespace

void launch_fill_box(const float* weight, int nx, int ny, long long nvox, int* part, int* box, hipStream_t s) {
    const int nblk = (int)std::max<long long>(1, std::min<long long>((nvox + kBlock - 1) / kBlock, kFillBoxBlocks));
    hipLaunchKernelGGL(k_fill_box_part, dim3(nblk), dim3(kBlock), 0, s, weight, nx, ny, nvox, part);
    hipLaunchKernelGGL(k_fill_box_final, dim3(1), dim3(kBlock), 0, s, (const int*)part, nblk, box);
}
void launch_fill_round(const FillGrid& g, int r, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_round, dim3(blocks(box_cells(g))), dim3(kBlock), 0, s, g, r);
}
void launch_fill_flags(const FillGrid& g, int* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_flags, dim3(blocks(box_cells(g))), dim3(kBlock), 0, s, g, flag);
}
void launch_fill_list(const FillGrid& g, const int* offs, int n, long long* lin, unsigned char* round, int* nb, float* val, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_list, dim3(blocks(box_cells(g))), dim3(kBlock), 0, s, g, offs, n, lin, round, nb, val);
}
void launch_fill_sweep(const FillPlanes& w, const int* nb, int n, const float* in, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_sweep, dim3(blocks(n)), dim3(kBlock), 0, s, w, nb, n, in, out);
}
void launch_fill_pack(const float* val, int n, float* grad, float* rgb, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_pack, dim3(blocks(n)), dim3(kBlock), 0, s, val, n, grad, rgb);
}
void launch_fill_scatter(const FillPlanes& w, const long long* lin, int n, const float* val, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_scatter, dim3(blocks(n)), dim3(kBlock), 0, s, w, lin, n, val);
}
void launch_wmesh_filled(const WMeshGrid& g, const int* num, int n_verts, const unsigned char* round, const int* keep, int n_kept, unsigned char* out, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_filled, dim3(blocks(g.nown)), dim3(kBlock), 0, s, g, num, n_verts, round, keep, n_kept, out);
}

}  // namespace psg
