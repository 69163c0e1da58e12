// extract.hip -- the writers' geometry on the device: what voxelPS dumps every third iteration used to cost a
// download of the whole dense volume (7 N^3 floats), a single-threaded marching-cubes pass and a pass over N^3 voxels on the host.  Here:
//   psgsdf_extract_mesh        Optimizer::extract_mesh (OptimizerAux.cpp:278-363) + MarchingCubes::computeIsoSurface / computeTriangles
//                              (third/mesh/MarchingCubes.cpp:314-637): crop box of |d| <= sqrt(3) vs, count -> exclusive scan -> emit, the reference's
//                              cell order (z, y, x) and the classic table's face order, non-indexed vertices
//   psgsdf_extract_pointcloud  Optimizer::save_pointcloud (OptimizerAux.cpp:456-511, band voxels) / VolumetricGradSdf::extract_pc
//                              (VolumetricGradSdf.cpp:320-376, every voxel with weight > 0): flags -> scan -> fill in ascending voxel order
//   psgsdf_extract_sdf         the cropped -dist block of Optimizer::saveSDF / VolumetricGradSdf::saveSDF (OptimizerAux.cpp:513-577)
// The arithmetic is the HOST writers' (psgradientsdf_amd/host/marching_cubes.hpp, ps_optimizer.hpp), operation for operation, with FMA contraction
// off: the files written from these arrays are byte-identical to the ones the host-side pass writes (tests/test_extract_gpu.py).
// Multi-rank contexts (z-slabs): the calls are collective and every rank returns ITS share -- the cells whose lower z-plane it owns, its own band rows /
// voxels / planes of the (global) crop box -- in the single context's order, so that the shares concatenated in rank order ARE the single context's
// arrays (tests/test_extract_gpu.py gathers the slabs' volume into one context and compares).  Two exchanges: the crop box (one all-reduce of 6 R
// numbers) and, for the mesh, the albedo of the upper neighbour's first plane (a cell reaches one plane up; the engine itself only keeps the halo
// planes' DISTANCES current).
#include "engine_internal.h"
#include "mc_common.h"
#include "../../include/psgsdf_mesh.h"
#include "mesh_lod.h"

namespace psg {
namespace {

#pragma clang fp contract(off)

// ---- crop box: min / max voxel index over |d| <= sqrt(3) vs (crop_box, ps_optimizer.hpp; the comparison is the host's: double)
__global__ void __launch_bounds__(kBlock) k_box_part(const float* __restrict__ dist, int nx, int ny, long long nvox, int k0, double lim, int* __restrict__ part) {
    int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-(1 << 30), -(1 << 30), -(1 << 30)};
    const long long nxy = (long long)nx * ny;
    for (long long lin = blockIdx.x * (long long)blockDim.x + threadIdx.x; lin < nvox; lin += (long long)gridDim.x * blockDim.x) {
        if ((double)fabsf(dist[lin]) > lim) continue;
        const int kl = (int)(lin / nxy), rest = (int)(lin - (long long)kl * nxy), j = rest / nx, i = rest - j * nx, k = kl + k0;      // (k0: global z of the first plane looked at)
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
__global__ void __launch_bounds__(kBlock) k_box_final(const int* __restrict__ part, int nblk, int* __restrict__ box) {
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

// ---- exclusive scan of int counts (1024-element tiles; the counts are replaced by their offsets, *total = their sum)
constexpr int kTile = 1024;
__global__ void __launch_bounds__(kBlock) k_cscan_tile(int* __restrict__ v, long long n, int* __restrict__ sums) {
    __shared__ int wsum[kBlock / 64];
    const long long base = (long long)blockIdx.x * kTile + threadIdx.x * 4;
    int f[4]; int loc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = (base + i < n) ? v[base + i] : 0; loc += f[i]; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int woff = 0;
    for (int i = 0; i < w; ++i) woff += wsum[i];
    int excl = woff + inc - loc;
#pragma unroll
    for (int i = 0; i < 4; ++i) { if (base + i < n) v[base + i] = excl; excl += f[i]; }
    if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = woff + inc;
}
__global__ void __launch_bounds__(1024) k_cscan_sums(int* __restrict__ sums, int nb, int* __restrict__ total) {
    __shared__ int wsum[16]; __shared__ int carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int val = i < nb ? sums[i] : 0;
        int inc = val;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < w; ++k) woff += wsum[k];
        const int carry = carry_s;
        if (i < nb) sums[i] = carry + woff + inc - val;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}
__global__ void __launch_bounds__(kBlock) k_cscan_add(int* __restrict__ v, long long n, const int* __restrict__ sums) {
    const long long base = (long long)blockIdx.x * kTile + threadIdx.x * 4;
    const int off = sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i) if (base + i < n) v[base + i] += off;
}

// ---- marching cubes over the cropped grid
struct McGrid {
    const float* dist; const float* weight; const float* rho[3];
    int nx, ny;                 // the dense grid's row / plane strides
    int lo[3], d[3];            // crop box: first voxel and extent (global)
    int zlo;                    // global z of the context's local plane 0 (0 on one rank)
    int zc0;                    // first cell plane of this launch (a slab: the cells whose lower plane it owns)
    float voxel[3], origin[3];  // MarchingCubes ctor: size / dim, and the origin offset that is subtracted (write_mesh: -vs * lo)
    long long total;            // voxels of the cropped grid (the colour look-ups run one / two past it: B10)
};
__device__ __forceinline__ long long dense_lin(const McGrid& g, int i, int j, int k) { return (long long)(k + g.lo[2] - g.zlo) * g.nx * g.ny + (long long)(j + g.lo[1]) * g.nx + (i + g.lo[0]); }
// colour byte of channel ch at CROPPED linear index cl (write_mesh: (unsigned char)int(255 * rgb); at(): 0 past the last voxel)
__device__ __forceinline__ unsigned char colour_at(const McGrid& g, int ch, long long cl) {
    if (cl >= g.total) return 0;
    const int k = (int)(cl / ((long long)g.d[0] * g.d[1])), rest = (int)(cl - (long long)k * g.d[0] * g.d[1]), j = rest / g.d[0], i = rest - j * g.d[0];
    return (unsigned char)(int)(255 * g.rho[ch][dense_lin(g, i, j, k)]);
}
// one cell: its triangles (non-degenerate ones, in table order) -> count, or written at `out_v / out_c` (3 vertices per face)
template <bool EMIT>
__device__ __forceinline__ int mc_cell(const McGrid& g, int x, int y, int z, float* out_v, unsigned char* out_c) {
    long long off[8]; long long dl[8]; bool valid = true; int cs = 0;
    float t[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int i = x + kCornerD[c][0], j = y + kCornerD[c][1], k = z + kCornerD[c][2];
        off[c] = (long long)k * g.d[0] * g.d[1] + (long long)j * g.d[0] + i;
        dl[c] = dense_lin(g, i, j, k);
        if (g.weight[dl[c]] == 0.0f) valid = false;
    }
    if (!valid) return 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) { t[c] = -g.dist[dl[c]]; if (t[c] > 0.0f) cs |= 1 << c; }
    if (cs == 0 || cs == 255) return 0;
    float ep[12][3]; unsigned char ec[12][3]; unsigned have = 0;
    for (int q = 0; q < 16 && kTri[cs][q] >= 0; ++q) {
        const int e = kTri[cs][q];
        if (have & (1u << e)) continue;
        have |= 1u << e;
        const int a = kEdgeD[e][0], b = kEdgeD[e][1];
        float pa[3], pb[3];
        const int base[3] = {x, y, z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ia = base[k] + kCornerD[a][k], ib = base[k] + kCornerD[b][k];
            pa[k] = ia * g.voxel[k] - g.origin[k]; pb[k] = ib * g.voxel[k] - g.origin[k];      // voxelToWorld, :647-651
        }
        mc_interp(t[a], t[b], pa, pb, ep[e]);
        if (EMIT) {
            // getColor :592-608 with the reversed end points of edges 2, 3, 6, 7 and the +1 / +2 index offsets of green / blue (B10)
            const bool rev = e == 2 || e == 3 || e == 6 || e == 7;
            const int c1 = rev ? b : a, c2 = rev ? a : b;
            const long long o1 = off[c1], o2 = off[c2];
            const float ca[3] = {colour_at(g, 0, o1) / 255.0f, colour_at(g, 1, o1 + 1) / 255.0f, colour_at(g, 2, o1 + 2) / 255.0f};
            const float cb[3] = {colour_at(g, 0, o2) / 255.0f, colour_at(g, 1, o2 + 1) / 255.0f, colour_at(g, 2, o2 + 2) / 255.0f};
            float cv[3]; mc_interp(t[c1], t[c2], ca, cb, cv);
            for (int k = 0; k < 3; ++k) ec[e][k] = (unsigned char)(cv[k] * 255.0f);
        }
    }
    int n = 0;
    for (int q = 0; q + 2 < 16 && kTri[cs][q] >= 0; q += 3) {
        const int e0 = kTri[cs][q], e1 = kTri[cs][q + 1], e2 = kTri[cs][q + 2];
        auto same = [&](int p, int r) { return ep[p][0] == ep[r][0] && ep[p][1] == ep[r][1] && ep[p][2] == ep[r][2]; };
        if (same(e0, e1) || same(e0, e2) || same(e1, e2)) continue;   // degenerate, :623
        if (EMIT) {
            const int es[3] = {e0, e1, e2};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { out_v[(n * 3 + v) * 3 + k] = ep[es[v]][k]; out_c[(n * 3 + v) * 3 + k] = ec[es[v]][k]; }
        }
        ++n;
    }
    return n;
}
__global__ void __launch_bounds__(kBlock) k_mc_count(McGrid g, long long ncell, int* __restrict__ cnt) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const int cx = g.d[0] - 2, cy = g.d[1] - 2;
    const int zl = (int)(c / ((long long)cx * cy)), rest = (int)(c - (long long)zl * cx * cy), y = rest / cx, x = rest - y * cx, z = zl + g.zc0;
    cnt[c] = mc_cell<false>(g, x, y, z, nullptr, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_mc_emit(McGrid g, long long ncell, const int* __restrict__ offs, int total, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const int mine = (c + 1 < ncell ? offs[c + 1] : total) - offs[c];
    if (mine <= 0) return;
    const int cx = g.d[0] - 2, cy = g.d[1] - 2;
    const int zl = (int)(c / ((long long)cx * cy)), rest = (int)(c - (long long)zl * cx * cy), y = rest / cx, x = rest - y * cx, z = zl + g.zc0;
    mc_cell<true>(g, x, y, z, xyz + (size_t)offs[c] * 9, rgb + (size_t)offs[c] * 9);
}

// ---- point clouds
// which = 0: the band voxels (ascending) with |d| < sqrt(3) vs;  which = 1: every voxel with weight > 0 and |d| < sqrt(3) vs
__global__ void __launch_bounds__(kBlock) k_pc_flags(const float* __restrict__ dist, const float* __restrict__ weight, const int* __restrict__ band_lin, long long lin0, long long n, double lim, int* __restrict__ flag) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long lin = band_lin ? band_lin[i] : i + lin0;      // (lin0: the first voxel of the planes the context owns)
    flag[i] = ((double)fabsf(dist[lin]) < lim && (band_lin || weight[lin] > 0)) ? 1 : 0;
}
__global__ void __launch_bounds__(kBlock) k_pc_fill(DenseView d, int nx, int ny, int zlo, float vs, const int* __restrict__ band_lin, long long lin0, long long n, double lim, const int* __restrict__ offs,
                                                    float* __restrict__ pn, int* __restrict__ col) {
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= n) return;
    const long long lin = band_lin ? band_lin[q] : q + lin0;
    if (!((double)fabsf(d.dist[lin]) < lim && (band_lin || d.weight[lin] > 0))) return;
    const long long nxy = (long long)nx * ny;
    const int kl = (int)(lin / nxy), rest = (int)(lin - (long long)kl * nxy), j = rest / nx, i = rest - j * nx, k = kl + zlo;
    float g[3] = {d.g[0][lin], d.g[1][lin], d.g[2][lin]};
    const float z = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    if (z > 0) { const float s = sqrtf(z); g[0] /= s; g[1] /= s; g[2] /= s; }
    const float dd = d.dist[lin];
    const size_t o = (size_t)offs[q];
    pn[o * 6 + 0] = vs * i - dd * g[0]; pn[o * 6 + 1] = vs * j - dd * g[1]; pn[o * 6 + 2] = vs * k - dd * g[2];
    pn[o * 6 + 3] = g[0]; pn[o * 6 + 4] = g[1]; pn[o * 6 + 5] = g[2];
    for (int a = 0; a < 3; ++a) col[o * 3 + a] = (int)(255 * d.rho[a][lin]);      // (printed as int, not as a byte: ps_optimizer.hpp save_pointcloud)
}
__global__ void __launch_bounds__(kBlock) k_sdf_crop(const float* __restrict__ dist, int nx, int ny, int lo0, int lo1, int lo2, int d0, int d1, long long n, float* __restrict__ out) {
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int k = (int)(q / ((long long)d0 * d1)), rest = (int)(q - (long long)k * d0 * d1), j = rest / d0, i = rest - j * d0;
    out[q] = -dist[(long long)(k + lo2) * nx * ny + (long long)(j + lo1) * nx + (i + lo0)];
}

}  // namespace
}  // namespace psg

using namespace psge;

namespace {
int scan_counts(psgsdf_ctx* c, int* v, long long n, int* sums, int* total_host) {
    const int nb = (int)((n + psg::kTile - 1) / psg::kTile);
    hipLaunchKernelGGL(psg::k_cscan_tile, dim3(nb), dim3(kBlock), 0, c->stream, v, n, sums);
    hipLaunchKernelGGL(psg::k_cscan_sums, dim3(1), dim3(1024), 0, c->stream, sums, nb, c->d_total);
    hipLaunchKernelGGL(psg::k_cscan_add, dim3(nb), dim3(kBlock), 0, c->stream, v, n, (const int*)sums);
    HIPCHK(c, hipMemcpyAsync(total_host, c->d_total, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// engine-owned pinned host buffer that lives until the next extraction on this context
int host_out(psgsdf_ctx* c, int slot, size_t bytes, void** p) {
    if (c->xo_bytes[slot] < bytes) {
        if (c->xo_host[slot]) hipHostFree(c->xo_host[slot]);
        c->xo_host[slot] = nullptr; c->xo_bytes[slot] = 0;
        HIPCHK(c, hipHostMalloc(&c->xo_host[slot], std::max<size_t>(bytes, 4096), hipHostMallocDefault));
        c->xo_bytes[slot] = std::max<size_t>(bytes, 4096);
    }
    *p = c->xo_host[slot];
    return 0;
}
// the crop box of |d| <= sqrt(3) vs; any = false if no voxel qualifies
int crop_box_dev(psgsdf_ctx* c, int lo[3], int hi[3], bool* any) {
    // (a slab looks at the planes it OWNS: [z0, z1) of the volume = local planes [z0 - zlo, z1 - zlo))
    const long long plane = (long long)c->grid.dim[0] * c->grid.dim[1], n = plane * (c->z1 - c->z0);
    const float* dist0 = c->dense.dist + plane * (c->z0 - c->zlo);
    const int nblk = (int)std::max<long long>(1, std::min<long long>((n + kBlock - 1) / kBlock, 2048));
    int* part = nullptr;
    HIPCHK(c, hipMalloc(&part, sizeof(int) * (6 * (size_t)nblk + 6)));
    const double lim = sqrt(3.0) * (double)c->grid.vs;      // std::sqrt(3) * vs: double (ps_optimizer.hpp crop_box)
    hipLaunchKernelGGL(psg::k_box_part, dim3(nblk), dim3(kBlock), 0, c->stream, dist0, c->grid.dim[0], c->grid.dim[1], n, c->z0, lim, part);
    hipLaunchKernelGGL(psg::k_box_final, dim3(1), dim3(kBlock), 0, c->stream, part, nblk, part + 6 * (size_t)nblk);
    int box[6];
    hipError_t e = hipMemcpyAsync(box, part + 6 * (size_t)nblk, sizeof(box), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(part);
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "crop box: %s", hipGetErrorString(e));
    if (c->n_ranks > 1) {      // min / max over the slabs: every rank's six numbers in its own slots of one sum
        std::vector<double> all((size_t)6 * c->n_ranks, 0.0);
        for (int a = 0; a < 6; ++a) all[(size_t)6 * c->rank + a] = (double)box[a];
        if (int rc = host_allreduce(c, all, "crop box")) return rc;
        for (int r = 0; r < c->n_ranks; ++r)
            for (int a = 0; a < 6; ++a) { const int v = (int)all[(size_t)6 * r + a]; box[a] = r == 0 ? v : (a < 3 ? std::min(box[a], v) : std::max(box[a], v)); }
    }
    for (int a = 0; a < 3; ++a) { lo[a] = box[a]; hi[a] = box[3 + a]; }
    *any = hi[0] >= lo[0];
    return 0;
}
int extract_ready(psgsdf_ctx* c, const char* what) {
    if (!c || !c->have_volume) return fail(c, PSGSDF_ERR_STATE, "%s: no volume", what);
    if (c->n_ranks > 1 && !c->comm) return fail(c, PSGSDF_ERR_COMM, "%s: rank %d of %d has no communicator", what, c->rank, c->n_ranks);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->deferred.empty() || c->pending_fold.n) { int rc = flush(c); if (rc) return rc; }
    if (c->inited) launch_band_scatter(c->dense, c->band, c->stream);      // the band's state back into the dense arrays (as psgsdf_download_volume does)
    return 0;
}
}  // namespace

extern "C" {

int psgsdf_extract_mesh(psgsdf_ctx* c, const float** xyz, const uint8_t** rgb, int64_t* n_vertices) {
    if (!xyz || !rgb || !n_vertices) return fail(c, PSGSDF_ERR_ARG, "extract_mesh: null argument");
    { int rc = extract_ready(c, "extract_mesh"); if (rc) return rc; }
    *xyz = nullptr; *rgb = nullptr; *n_vertices = 0;
    int lo[3], hi[3]; bool any = false;
    { int rc = crop_box_dev(c, lo, hi, &any); if (rc) return rc; }
    if (!any) return PSGSDF_OK;
    psg::McGrid g{};
    g.dist = c->dense.dist; g.weight = c->dense.weight; for (int a = 0; a < 3; ++a) g.rho[a] = c->dense.rho[a];
    g.nx = c->grid.dim[0]; g.ny = c->grid.dim[1]; g.zlo = c->zlo;
    const float vs = c->grid.vs;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a]; g.d[a] = hi[a] - lo[a] + 1;
        const float size = vs * g.d[a];                    // write_mesh: size[] = {vs * d[0], ..}, org[] = {-vs * lo[0], ..}
        g.voxel[a] = size / g.d[a];                        // MarchingCubes ctor: voxel_ = size / dim
        g.origin[a] = -vs * lo[a];
    }
    g.total = (long long)g.d[0] * g.d[1] * g.d[2];
    if (g.d[0] < 3 || g.d[1] < 3 || g.d[2] < 3) return PSGSDF_OK;      // (no cell: the loops of computeIsoSurface run to dim - 2)
    // the cells of this context: lower plane lo2 + zc in [z0, z1) (their upper plane is the halo plane of a slab with a neighbour above)
    g.zc0 = std::max(0, c->z0 - lo[2]);
    const int zc1 = std::min(g.d[2] - 2, c->z1 - lo[2]);
    if (c->n_ranks > 1) {      // the albedo of plane z1 from the rank above (the cells' upper corners and their colours)
        const size_t plane = (size_t)g.nx * g.ny;
        std::vector<psgsdf_comm_xfer> sends, recvs;
        for (int a = 0; a < 3; ++a) {
            if (c->rank > 0) sends.push_back({(void*)(c->dense.rho[a] + plane * (size_t)(c->z0 - c->zlo)), sizeof(float) * plane, c->rank - 1});
            if (c->rank + 1 < c->n_ranks) recvs.push_back({(void*)(c->dense.rho[a] + plane * (size_t)(c->z1 - c->zlo)), sizeof(float) * plane, c->rank + 1});
        }
        if (int rc = comm_xfer(c, sends, recvs)) return rc;
    }
    const long long ncell = (long long)(g.d[0] - 2) * (g.d[1] - 2) * std::max(0, zc1 - g.zc0);
    if (ncell == 0) return PSGSDF_OK;
    if (ncell >= (1ll << 31)) return fail(c, PSGSDF_ERR_UNSUPPORTED, "extract_mesh: %lld cells", ncell);
    const int nb = (int)((ncell + psg::kTile - 1) / psg::kTile);
    int* cnt = nullptr; int* sums = nullptr;
    HIPCHK(c, hipMalloc(&cnt, sizeof(int) * (size_t)ncell));
    if (hipMalloc(&sums, sizeof(int) * (size_t)(nb + 1)) != hipSuccess) { hipFree(cnt); return fail(c, PSGSDF_ERR_DEVICE, "extract_mesh: out of memory"); }
    int rc = 0, total = 0;
    float* d_xyz = nullptr; unsigned char* d_rgb = nullptr;
    timed(c, "mc_count", [&] { hipLaunchKernelGGL(psg::k_mc_count, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, g, ncell, cnt); });
    rc = scan_counts(c, cnt, ncell, sums, &total);
    if (!rc && total > 0) {
        const size_t nv = (size_t)total * 3;
        if (hipMalloc(&d_xyz, sizeof(float) * 3 * nv) != hipSuccess || hipMalloc(&d_rgb, 3 * nv) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_mesh: out of memory (%d faces)", total);
        void *hx = nullptr, *hc = nullptr;
        if (!rc) rc = host_out(c, 0, sizeof(float) * 3 * nv, &hx);
        if (!rc) rc = host_out(c, 1, 3 * nv, &hc);
        if (!rc) {
            timed(c, "mc_emit", [&] { hipLaunchKernelGGL(psg::k_mc_emit, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, g, ncell, (const int*)cnt, total, d_xyz, d_rgb); });
            if (hipMemcpyAsync(hx, d_xyz, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipMemcpyAsync(hc, d_rgb, 3 * nv, hipMemcpyDeviceToHost, c->stream) != hipSuccess
                || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_mesh: download");
        }
        if (!rc) { *xyz = (const float*)hx; *rgb = (const uint8_t*)hc; *n_vertices = (int64_t)nv; }
    }
    hipFree(cnt); hipFree(sums); hipFree(d_xyz); hipFree(d_rgb);
    return rc;
}

int psgsdf_extract_pointcloud(psgsdf_ctx* c, int which, const float** xyz_nxyz, const int32_t** rgb, int64_t* n_points) {
    if (!xyz_nxyz || !rgb || !n_points || which < 0 || which > 1) return fail(c, PSGSDF_ERR_ARG, "extract_pointcloud: bad argument");
    { int rc = extract_ready(c, "extract_pointcloud"); if (rc) return rc; }
    if (which == 0 && !c->inited) return fail(c, PSGSDF_ERR_STATE, "extract_pointcloud(band): psgsdf_init first");
    *xyz_nxyz = nullptr; *rgb = nullptr; *n_points = 0;
    // a slab: its own band rows [row0, row1) / the voxels of the planes it owns
    const long long plane = (long long)c->grid.dim[0] * c->grid.dim[1], lin0 = plane * (c->z0 - c->zlo);
    const long long n = which == 0 ? (long long)(c->row1 - c->row0) : plane * (c->z1 - c->z0);
    if (n <= 0) return PSGSDF_OK;
    const int* band_lin = which == 0 ? c->band.lin + c->row0 : nullptr;
    const double lim = sqrt(3.0) * (double)c->grid.vs;
    const int nb = (int)((n + psg::kTile - 1) / psg::kTile);
    int* flag = nullptr; int* sums = nullptr;
    HIPCHK(c, hipMalloc(&flag, sizeof(int) * (size_t)n));
    if (hipMalloc(&sums, sizeof(int) * (size_t)(nb + 1)) != hipSuccess) { hipFree(flag); return fail(c, PSGSDF_ERR_DEVICE, "extract_pointcloud: out of memory"); }
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(psg::k_pc_flags, dim3(grid), dim3(kBlock), 0, c->stream, c->dense.dist, c->dense.weight, band_lin, lin0, n, lim, flag);
    int total = 0;
    int rc = scan_counts(c, flag, n, sums, &total);
    float* d_pn = nullptr; int* d_col = nullptr;
    if (!rc && total > 0) {
        if (hipMalloc(&d_pn, sizeof(float) * 6 * (size_t)total) != hipSuccess || hipMalloc(&d_col, sizeof(int) * 3 * (size_t)total) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_pointcloud: out of memory");
        void *hp = nullptr, *hc = nullptr;
        if (!rc) rc = host_out(c, 2, sizeof(float) * 6 * (size_t)total, &hp);
        if (!rc) rc = host_out(c, 3, sizeof(int) * 3 * (size_t)total, &hc);
        if (!rc) {
            hipLaunchKernelGGL(psg::k_pc_fill, dim3(grid), dim3(kBlock), 0, c->stream, c->dense, c->grid.dim[0], c->grid.dim[1], c->zlo, c->grid.vs, band_lin, lin0, n, lim, (const int*)flag, d_pn, d_col);
            if (hipMemcpyAsync(hp, d_pn, sizeof(float) * 6 * (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipMemcpyAsync(hc, d_col, sizeof(int) * 3 * (size_t)total, hipMemcpyDeviceToHost, c->stream) != hipSuccess
                || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_pointcloud: download");
        }
        if (!rc) { *xyz_nxyz = (const float*)hp; *rgb = (const int32_t*)hc; *n_points = total; }
    }
    hipFree(flag); hipFree(sums); hipFree(d_pn); hipFree(d_col);
    return rc;
}

int psgsdf_extract_sdf(psgsdf_ctx* c, int32_t lo[3], int32_t dim[3], const float** neg_dist) {
    if (!lo || !dim || !neg_dist) return fail(c, PSGSDF_ERR_ARG, "extract_sdf: null argument");
    { int rc = extract_ready(c, "extract_sdf"); if (rc) return rc; }
    *neg_dist = nullptr; for (int a = 0; a < 3; ++a) { lo[a] = 0; dim[a] = 0; }
    int l[3], h[3]; bool any = false;
    { int rc = crop_box_dev(c, l, h, &any); if (rc) return rc; }
    if (!any) return PSGSDF_OK;
    const int d0 = h[0] - l[0] + 1, d1 = h[1] - l[1] + 1, d2 = h[2] - l[2] + 1;
    for (int a = 0; a < 3; ++a) lo[a] = l[a];
    dim[0] = d0; dim[1] = d1; dim[2] = d2;
    // a slab: the planes of the box it owns, [ka, kb)
    const int ka = std::max(l[2], c->z0), kb = std::min(h[2] + 1, c->z1);
    const long long n = (long long)d0 * d1 * std::max(0, kb - ka);
    if (n == 0) return PSGSDF_OK;
    float* dv = nullptr; void* hv = nullptr;
    HIPCHK(c, hipMalloc(&dv, sizeof(float) * (size_t)n));
    int rc = host_out(c, 4, sizeof(float) * (size_t)n, &hv);
    if (!rc) {
        hipLaunchKernelGGL(psg::k_sdf_crop, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, c->dense.dist, c->grid.dim[0], c->grid.dim[1], l[0], l[1], ka - c->zlo, d0, d1, n, dv);
        if (hipMemcpyAsync(hv, dv, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_sdf: download");
    }
    hipFree(dv);
    if (rc) return rc;
    *neg_dist = (const float*)hv;
    return PSGSDF_OK;
}

}  // extern "C"

// ---- welded, indexed meshes (include/psgsdf_mesh.h; kernels: mesh.hip; DESIGN.md "Welded meshes")
namespace {
// the welded mesh of the context's state as device arrays (this rank's share), the kernels launched on the stream and not waited for: what
// psgsdf_extract_mesh_indexed downloads and psgsdf_extract_mesh_components goes on from.  nv == 0 && nf == 0: nothing was allocated.
struct WMeshDev {
    float *xyz = nullptr, *nrm = nullptr; unsigned char* rgb = nullptr; int* faces = nullptr;
    int nv = 0, nf = 0; long long first = 0;
    void* tmp[5] = {};      // the extraction's temporaries, freed with the arrays once the stream has been waited for
    void release() { for (void*& t : tmp) { hipFree(t); t = nullptr; } hipFree(xyz); hipFree(nrm); hipFree(rgb); hipFree(faces); xyz = nrm = nullptr; rgb = nullptr; faces = nullptr; }
};
int wmesh_device(psgsdf_ctx* c, WMeshDev* m) {
    int lo[3], hi[3]; bool any = false;
    { int rc = crop_box_dev(c, lo, hi, &any); if (rc) return rc; }      // (collective: every rank takes the same early returns below)
    if (!any) return PSGSDF_OK;
    psg::WMeshGrid g{};
    g.dist = c->dense.dist; g.weight = c->dense.weight;
    for (int a = 0; a < 3; ++a) { g.g[a] = c->dense.g[a]; g.rho[a] = c->dense.rho[a]; }
    g.nx = c->grid.dim[0]; g.ny = c->grid.dim[1]; g.zlo = c->zlo; g.zh = -1;
    const float vs = c->grid.vs;
    for (int a = 0; a < 3; ++a) {      // psgsdf_extract_mesh's frame, operation for operation
        g.lo[a] = lo[a]; g.d[a] = hi[a] - lo[a] + 1;
        const float size = vs * g.d[a];
        g.voxel[a] = size / g.d[a];
        g.origin[a] = -vs * lo[a];
    }
    if (g.d[0] < 3 || g.d[1] < 3 || g.d[2] < 3) return PSGSDF_OK;
    const long long P = 4ll * g.d[0] * g.d[1];      // key slots per plane
    if (P * (g.d[2] + 1) >= (1ll << 31)) return fail(c, PSGSDF_ERR_UNSUPPORTED, "extract_mesh_indexed: %lld key slots", P * (g.d[2] + 1));
    // this context: the cells whose lower plane it owns, the key planes it owns [kp0, kp1) and the one above (the upper neighbour's first plane)
    g.zc0 = std::max(0, c->z0 - lo[2]);
    const int zc1 = std::min(g.d[2] - 2, c->z1 - lo[2]), kp1 = std::min(g.d[2], c->z1 - lo[2]);
    const long long ncell = (long long)(g.d[0] - 2) * (g.d[1] - 2) * std::max(0, zc1 - g.zc0);
    g.nown = P * std::max(0, kp1 - g.zc0);
    const bool up = c->rank + 1 < c->n_ranks, down = c->rank > 0;
    const size_t plane = (size_t)g.nx * g.ny;
    // temporaries: flags / vertex numbers (4 ints per voxel of the crop planes + one plane), face counts (1 int per cell), scan sums, the exchanged planes
    const long long nflag = g.nown + P, nscan = std::max(g.nown, ncell);
    int *flag = nullptr, *cnt = nullptr, *sums = nullptr, *xin = nullptr; float* halo = nullptr;
    bool ok = hipMalloc(&flag, sizeof(int) * (size_t)nflag) == hipSuccess && hipMalloc(&cnt, sizeof(int) * (size_t)std::max(1ll, ncell)) == hipSuccess
              && hipMalloc(&sums, sizeof(int) * (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1)) == hipSuccess;
    if (ok && c->n_ranks > 1) ok = hipMalloc(&xin, sizeof(int) * (size_t)(2 * P)) == hipSuccess && (!up || hipMalloc(&halo, sizeof(float) * 6 * plane) == hipSuccess);
    auto release = [&] { hipFree(flag); hipFree(cnt); hipFree(sums); hipFree(xin); hipFree(halo); };
    if (c->n_ranks > 1) {      // every rank learns whether all of them have their temporaries before anyone enters an exchange
        std::vector<double> st(1, ok ? 0.0 : 1.0);
        if (int rc = host_allreduce(c, st, "extract_mesh_indexed")) { release(); return rc; }
        if (st[0] != 0.0) { release(); return fail(c, PSGSDF_ERR_DEVICE, "extract_mesh_indexed: out of memory on %d rank(s)", (int)st[0]); }
    } else if (!ok) { release(); return fail(c, PSGSDF_ERR_DEVICE, "extract_mesh_indexed: out of memory"); }
    int rc = 0;
    if (hipMemsetAsync(flag, 0, sizeof(int) * (size_t)nflag, c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_mesh_indexed: memset");
    if (!rc && ncell > 0) timed(c, "wmesh_mark", [&] { psg::launch_wmesh_mark(g, ncell, cnt, flag, c->stream); });
    if (c->n_ranks > 1) {      // (entered even after a local failure: the neighbours wait for it)
        // the used flags of plane z1 go up and are OR-ed into the owner's first plane; the gradient and albedo of plane z0 go down (z-edges z1 - 1 -> z1)
        std::vector<psgsdf_comm_xfer> sends, recvs;
        if (up) {
            sends.push_back({(void*)(flag + g.nown), sizeof(int) * (size_t)P, c->rank + 1});
            for (int a = 0; a < 3; ++a) {
                recvs.push_back({(void*)(halo + plane * a), sizeof(float) * plane, c->rank + 1});
                recvs.push_back({(void*)(halo + plane * (3 + a)), sizeof(float) * plane, c->rank + 1});
                g.hg[a] = halo + plane * a; g.hrho[a] = halo + plane * (3 + a);
            }
            g.zh = c->z1;
        }
        if (down) {
            recvs.push_back({(void*)xin, sizeof(int) * (size_t)P, c->rank - 1});
            for (int a = 0; a < 3; ++a) {
                sends.push_back({(void*)(c->dense.g[a] + plane * (size_t)(c->z0 - c->zlo)), sizeof(float) * plane, c->rank - 1});
                sends.push_back({(void*)(c->dense.rho[a] + plane * (size_t)(c->z0 - c->zlo)), sizeof(float) * plane, c->rank - 1});
            }
        }
        if (int r2 = comm_xfer(c, sends, recvs)) rc = rc ? rc : r2;
        if (!rc && down && g.nown > 0) psg::launch_wmesh_or(flag, xin, P, c->stream);
    }
    int nv = 0, nf = 0;
    if (!rc && g.nown > 0) rc = scan_counts(c, flag, g.nown, sums, &nv);      // flags -> vertex numbers (key order)
    if (!rc && ncell > 0) rc = scan_counts(c, cnt, ncell, sums, &nf);         // face counts -> face offsets
    // the ranks' vertex counts: this share's first global vertex number, the upper neighbour's
    long long first = 0, first_up = 0, total_v = nv;
    if (c->n_ranks > 1) {
        std::vector<double> all((size_t)c->n_ranks + 1, 0.0);
        all[(size_t)c->rank] = rc ? 0.0 : (double)nv; all[(size_t)c->n_ranks] = rc ? 1.0 : 0.0;
        if (int r2 = host_allreduce(c, all, "extract_mesh_indexed")) { release(); return r2; }
        if (all[(size_t)c->n_ranks] != 0.0 && !rc) rc = fail(c, PSGSDF_ERR_COMM, "extract_mesh_indexed: another rank failed");
        total_v = 0;
        for (int r = 0; r < c->n_ranks; ++r) { if (r < c->rank) first += (long long)all[(size_t)r]; if (r == c->rank + 1) first_up = first + nv; total_v += (long long)all[(size_t)r]; }
    }
    if (!rc && total_v > INT32_MAX) rc = fail(c, PSGSDF_ERR_UNSUPPORTED, "extract_mesh_indexed: %lld vertices", total_v);
    if (!rc && c->n_ranks > 1) {      // the vertex numbers of plane z1 come back down from its owner (as its local numbers; + first_up)
        std::vector<psgsdf_comm_xfer> sends, recvs;
        if (down) sends.push_back({(void*)flag, sizeof(int) * (size_t)P, c->rank - 1});
        if (up) recvs.push_back({(void*)(xin + P), sizeof(int) * (size_t)P, c->rank + 1});
        rc = comm_xfer(c, sends, recvs);
    }
    float *d_xyz = nullptr, *d_nrm = nullptr; unsigned char* d_rgb = nullptr; int* d_faces = nullptr;
    if (!rc && (nv > 0 || nf > 0)) {
        if ((nv > 0 && (hipMalloc(&d_xyz, sizeof(float) * 3 * (size_t)nv) != hipSuccess || hipMalloc(&d_nrm, sizeof(float) * 3 * (size_t)nv) != hipSuccess || hipMalloc(&d_rgb, 3 * (size_t)nv) != hipSuccess))
            || (nf > 0 && hipMalloc(&d_faces, sizeof(int) * 3 * (size_t)nf) != hipSuccess)) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_mesh_indexed: out of memory (%d vertices, %d faces)", nv, nf);
        if (!rc) {
            if (nf > 0) timed(c, "wmesh_faces", [&] { psg::launch_wmesh_faces(g, ncell, cnt, nf, flag, (int)first, xin ? xin + P : nullptr, (int)first_up, d_faces, c->stream); });
            if (nv > 0) timed(c, "wmesh_verts", [&] { psg::launch_wmesh_verts(g, flag, nv, d_xyz, d_nrm, d_rgb, c->stream); });
        }
    }
    if (rc) { release(); hipFree(d_xyz); hipFree(d_nrm); hipFree(d_rgb); hipFree(d_faces); return rc; }
    m->xyz = d_xyz; m->nrm = d_nrm; m->rgb = d_rgb; m->faces = d_faces; m->nv = nv; m->nf = nf; m->first = first;
    m->tmp[0] = flag; m->tmp[1] = cnt; m->tmp[2] = sums; m->tmp[3] = xin; m->tmp[4] = halo;      // (the kernels in flight read them)
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_indexed(psgsdf_ctx* c, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                           const int32_t** faces, int64_t* n_faces, int64_t* first_vertex) {
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !first_vertex) return fail(c, PSGSDF_ERR_ARG, "extract_mesh_indexed: null argument");
    { int rc = extract_ready(c, "extract_mesh_indexed"); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *n_vertices = 0; *n_faces = 0; *first_vertex = 0;
    WMeshDev m;
    int rc = wmesh_device(c, &m);
    if (rc) return rc;
    const int nv = m.nv, nf = m.nf;
    float *d_xyz = m.xyz, *d_nrm = m.nrm; unsigned char* d_rgb = m.rgb; int* d_faces = m.faces;
    if (nv > 0 || nf > 0) {
        void *hx = nullptr, *hn = nullptr, *hc = nullptr, *hf = nullptr;
        if (!rc) rc = host_out(c, 5, sizeof(float) * 3 * (size_t)nv, &hx);
        if (!rc) rc = host_out(c, 6, sizeof(float) * 3 * (size_t)nv, &hn);
        if (!rc) rc = host_out(c, 7, 3 * (size_t)nv, &hc);
        if (!rc) rc = host_out(c, 8, sizeof(int) * 3 * (size_t)nf, &hf);
        if (!rc) {
            bool cp = true;
            if (nv > 0) cp = hipMemcpyAsync(hx, d_xyz, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipMemcpyAsync(hn, d_nrm, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                            && hipMemcpyAsync(hc, d_rgb, 3 * (size_t)nv, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
            if (cp && nf > 0) cp = hipMemcpyAsync(hf, d_faces, sizeof(int) * 3 * (size_t)nf, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
            if (!cp || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "extract_mesh_indexed: download");
        }
        if (!rc) { *xyz = (const float*)hx; *normals = (const float*)hn; *rgb = (const uint8_t*)hc; *faces = (const int32_t*)hf; *n_vertices = nv; *n_faces = nf; }
    }
    if (!rc) *first_vertex = m.first;
    m.release();
    return rc;
}

// ---- connected components of the welded mesh, and the mesh without its small pieces (include/psgsdf_mesh.h; kernels: mesh_cc.hip; DESIGN.md "Mesh components")
namespace {
// the filtered mesh of the context's state as device arrays and its component list (pinned host slot 10), the last kernels launched on the stream and
// not waited for: what psgsdf_extract_mesh_components downloads and psgsdf_extract_mesh_lod goes on from.  After a failure, or with an empty mesh
// (nv == 0 && nf == 0 && nc == 0), everything has been waited for and freed.
struct MCompDev {
    WMeshDev m;
    int *parent = nullptr, *num = nullptr, *vcomp = nullptr, *uses = nullptr, *sums = nullptr, *d_kept = nullptr, *vflag = nullptr, *fflag = nullptr, *o_vcomp = nullptr, *o_faces = nullptr;
    unsigned long long* keys = nullptr; long long* stat = nullptr; unsigned* box = nullptr;
    float *o_xyz = nullptr, *o_nrm = nullptr; unsigned char* o_rgb = nullptr;
    const float *xyz = nullptr, *nrm = nullptr; const unsigned char* rgb = nullptr; const int *faces = nullptr, *vertex_component = nullptr;      // the kept components (the welded arrays themselves if all are kept)
    int nv = 0, nf = 0, nc = 0; psgsdf_mesh_component* list = nullptr;
    void release() {
        hipFree(parent); hipFree(num); hipFree(vcomp); hipFree(uses); hipFree(sums); hipFree(d_kept); hipFree(vflag); hipFree(fflag); hipFree(o_vcomp); hipFree(o_faces);
        hipFree(keys); hipFree(stat); hipFree(box); hipFree(o_xyz); hipFree(o_nrm); hipFree(o_rgb); m.release();
        parent = num = vcomp = uses = sums = d_kept = vflag = fflag = o_vcomp = o_faces = nullptr; keys = nullptr; stat = nullptr; box = nullptr; o_xyz = o_nrm = nullptr; o_rgb = nullptr;
    }
};
bool bad_filter(const psgsdf_mesh_filter& flt) { return flt.min_area != flt.min_area || flt.keep_largest < 0; }
int mcomp_device(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter& flt, MCompDev* d) {
    WMeshDev& m = d->m;
    int rc = wmesh_device(c, &m);
    if (rc) return rc;
    const int nv = m.nv, nf = m.nf;
    if (nv == 0 || nf == 0) { if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me); m.release(); return rc; }      // (every vertex belongs to a face: both or neither)
    // temporaries: 3 ints per vertex (parent, root flag / component number, component of the vertex), the edge table (6 slots of 12 B per face),
    // per component 8 x 8 B of counters and 6 x 4 B of box, the scan's sums; with a filter 1 int per vertex and face and the compacted arrays
    const unsigned long long cap = std::max<unsigned long long>(64, 6ull * (unsigned long long)nf);
    const long long nscan = std::max(nv, nf);
    int *&parent = d->parent, *&num = d->num, *&vcomp = d->vcomp, *&uses = d->uses, *&sums = d->sums, *&d_kept = d->d_kept, *&vflag = d->vflag, *&fflag = d->fflag, *&o_vcomp = d->o_vcomp, *&o_faces = d->o_faces;
    unsigned long long*& keys = d->keys; long long*& stat = d->stat; unsigned*& box = d->box;
    float *&o_xyz = d->o_xyz, *&o_nrm = d->o_nrm; unsigned char*& o_rgb = d->o_rgb;
    auto release = [&] { d->release(); };
    auto oom = [&] { hipStreamSynchronize(c->stream); release(); return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices, %d faces)", me, nv, nf); };
    if (hipMalloc(&parent, sizeof(int) * (size_t)nv) != hipSuccess || hipMalloc(&num, sizeof(int) * (size_t)nv) != hipSuccess || hipMalloc(&vcomp, sizeof(int) * (size_t)nv) != hipSuccess
        || hipMalloc(&keys, sizeof(unsigned long long) * (size_t)cap) != hipSuccess || hipMalloc(&uses, sizeof(int) * (size_t)cap) != hipSuccess
        || hipMalloc(&sums, sizeof(int) * (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1)) != hipSuccess) return oom();
    bool ok = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)cap, c->stream) == hipSuccess && hipMemsetAsync(uses, 0, sizeof(int) * (size_t)cap, c->stream) == hipSuccess;
    if (!ok) { hipStreamSynchronize(c->stream); release(); return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me); }
    timed(c, "mcomp_init", [&] { psg::launch_mcomp_init(parent, nv, c->stream); });
    timed(c, "mcomp_hook", [&] { psg::launch_mcomp_hook(m.faces, nf, parent, c->stream); });
    timed(c, "mcomp_flatten", [&] { psg::launch_mcomp_flatten(parent, nv, num, c->stream); });
    timed(c, "mcomp_edges", [&] { psg::launch_mcomp_edges(m.faces, nf, keys, uses, cap, c->stream); });
    int nc = 0;
    rc = scan_counts(c, num, nv, sums, &nc);      // root flags -> component numbers in ascending first vertex
    if (rc) { hipStreamSynchronize(c->stream); release(); return rc; }
    if (hipMalloc(&stat, sizeof(long long) * psg::kMcompStats * (size_t)nc) != hipSuccess || hipMalloc(&box, sizeof(unsigned) * 6 * (size_t)nc) != hipSuccess) return oom();
    unsigned *blo = box, *bhi = box + 3 * (size_t)nc;
    ok = hipMemsetAsync(stat, 0, sizeof(long long) * psg::kMcompStats * (size_t)nc, c->stream) == hipSuccess && hipMemsetAsync(blo, 0xff, sizeof(unsigned) * 3 * (size_t)nc, c->stream) == hipSuccess
         && hipMemsetAsync(bhi, 0, sizeof(unsigned) * 3 * (size_t)nc, c->stream) == hipSuccess;
    if (!ok) { hipStreamSynchronize(c->stream); release(); return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me); }
    const double vs = (double)c->grid.vs, unit = vs * vs / 16777216.0;      // one unit of the fixed-point area
    timed(c, "mcomp_vstats", [&] { psg::launch_mcomp_vstats(parent, num, nv, m.xyz, vcomp, stat, blo, bhi, c->stream); });
    timed(c, "mcomp_fstats", [&] { psg::launch_mcomp_fstats(m.faces, nf, vcomp, m.xyz, vs * vs, stat, c->stream); });
    timed(c, "mcomp_ecount", [&] { psg::launch_mcomp_ecount(keys, uses, cap, vcomp, stat, c->stream); });
    std::vector<long long> hstat((size_t)psg::kMcompStats * nc); std::vector<unsigned> hbox((size_t)6 * nc);
    if (hipMemcpyAsync(hstat.data(), stat, sizeof(long long) * hstat.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess
        || hipMemcpyAsync(hbox.data(), box, sizeof(unsigned) * hbox.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        release(); return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the component table", me);
    }
    void* hl = nullptr;
    rc = host_out(c, 10, sizeof(psgsdf_mesh_component) * (size_t)nc, &hl);
    if (rc) { release(); return rc; }
    psgsdf_mesh_component* list = (psgsdf_mesh_component*)hl;
    auto unordered = [](unsigned u) { u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; float f; memcpy(&f, &u, 4); return f; };
    for (int i = 0; i < nc; ++i) {
        const long long* s = hstat.data() + (size_t)psg::kMcompStats * i;
        psgsdf_mesh_component& k = list[i];
        k.first_vertex = s[psg::MC_FIRST]; k.n_vertices = s[psg::MC_VERTS]; k.n_faces = s[psg::MC_FACES]; k.n_edges = s[psg::MC_EDGES];
        k.n_boundary_edges = s[psg::MC_BOUNDARY]; k.n_nonmanifold_edges = s[psg::MC_NONMANIFOLD];
        k.area = unit * (double)s[psg::MC_AREA];
        for (int a = 0; a < 3; ++a) { k.lo[a] = unordered(hbox[(size_t)3 * i + a]); k.hi[a] = unordered(hbox[(size_t)3 * (nc + i) + a]); }
        k.kept = (k.n_faces >= flt.min_faces && k.area >= flt.min_area) ? 1 : 0; k.reserved = 0;
    }
    if (flt.keep_largest > 0) {      // of those that pass: the keep_largest with the most faces, ties to the smaller first vertex (= the smaller index)
        std::vector<int> pass;
        for (int i = 0; i < nc; ++i) if (list[i].kept) pass.push_back(i);
        std::stable_sort(pass.begin(), pass.end(), [&](int a, int b) { return list[a].n_faces > list[b].n_faces; });
        for (size_t q = (size_t)flt.keep_largest; q < pass.size(); ++q) list[pass[q]].kept = 0;
    }
    int n_kept = 0;
    for (int i = 0; i < nc; ++i) n_kept += list[i].kept;
    int ov = nv, of = nf;
    const float *r_xyz = m.xyz, *r_nrm = m.nrm; const unsigned char* r_rgb = m.rgb; const int *r_faces = m.faces, *r_vcomp = vcomp;
    if (n_kept < nc) {      // compaction (everything kept: the arrays as they are)
        std::vector<int> hk((size_t)nc);
        for (int i = 0; i < nc; ++i) hk[(size_t)i] = list[i].kept;
        if (hipMalloc(&d_kept, sizeof(int) * (size_t)nc) != hipSuccess || hipMalloc(&vflag, sizeof(int) * (size_t)nv) != hipSuccess || hipMalloc(&fflag, sizeof(int) * (size_t)nf) != hipSuccess) return oom();
        if (hipMemcpyAsync(d_kept, hk.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, c->stream) != hipSuccess) { hipStreamSynchronize(c->stream); release(); return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me); }
        timed(c, "mcomp_keep", [&] { psg::launch_mcomp_keep(d_kept, vcomp, nv, m.faces, nf, vflag, fflag, c->stream); });
        rc = scan_counts(c, vflag, nv, sums, &ov);      // (waits for the stream: hk stays alive until here)
        if (!rc) rc = scan_counts(c, fflag, nf, sums, &of);
        if (rc) { hipStreamSynchronize(c->stream); release(); return rc; }
        if (ov > 0 && of > 0) {
            if (hipMalloc(&o_xyz, sizeof(float) * 3 * (size_t)ov) != hipSuccess || hipMalloc(&o_nrm, sizeof(float) * 3 * (size_t)ov) != hipSuccess || hipMalloc(&o_rgb, 3 * (size_t)ov) != hipSuccess
                || hipMalloc(&o_vcomp, sizeof(int) * (size_t)ov) != hipSuccess || hipMalloc(&o_faces, sizeof(int) * 3 * (size_t)of) != hipSuccess) return oom();
            timed(c, "mcomp_compact", [&] { psg::launch_mcomp_compact(d_kept, vcomp, nv, m.faces, nf, vflag, fflag, m.xyz, m.nrm, m.rgb, o_xyz, o_nrm, o_rgb, o_vcomp, o_faces, c->stream); });
        }
        r_xyz = o_xyz; r_nrm = o_nrm; r_rgb = o_rgb; r_faces = o_faces; r_vcomp = o_vcomp;
    }
    d->xyz = r_xyz; d->nrm = r_nrm; d->rgb = r_rgb; d->faces = r_faces; d->vertex_component = r_vcomp; d->nv = ov; d->nf = of; d->nc = nc; d->list = list;
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_components(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                              const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component, const psgsdf_mesh_component** components, int64_t* n_components) {
    const char* me = "extract_mesh_components";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_component || !components || !n_components) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): components are not merged across z-slabs yet", me, c->rank, c->n_ranks);
    psgsdf_mesh_filter flt{0, 0.0, 0};
    if (filter) flt = *filter;
    if (bad_filter(flt)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_component = nullptr; *components = nullptr; *n_vertices = 0; *n_faces = 0; *n_components = 0;
    MCompDev d;
    int rc = mcomp_device(c, me, flt, &d);
    if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh: waited for and freed)
    const int ov = d.nv, of = d.nf;
    const float *r_xyz = d.xyz, *r_nrm = d.nrm; const unsigned char* r_rgb = d.rgb; const int *r_faces = d.faces, *r_vcomp = d.vertex_component;
    void *hx = nullptr, *hn = nullptr, *hc = nullptr, *hf = nullptr, *hv = nullptr;
    if (ov > 0 && of > 0) {
        rc = host_out(c, 5, sizeof(float) * 3 * (size_t)ov, &hx);
        if (!rc) rc = host_out(c, 6, sizeof(float) * 3 * (size_t)ov, &hn);
        if (!rc) rc = host_out(c, 7, 3 * (size_t)ov, &hc);
        if (!rc) rc = host_out(c, 8, sizeof(int) * 3 * (size_t)of, &hf);
        if (!rc) rc = host_out(c, 9, sizeof(int) * (size_t)ov, &hv);
        if (!rc) {
            const bool cp = hipMemcpyAsync(hx, r_xyz, sizeof(float) * 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipMemcpyAsync(hn, r_nrm, sizeof(float) * 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                            && hipMemcpyAsync(hc, r_rgb, 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipMemcpyAsync(hf, r_faces, sizeof(int) * 3 * (size_t)of, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                            && hipMemcpyAsync(hv, r_vcomp, sizeof(int) * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
            if (!cp || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: download", me);
        }
        if (!rc) { *xyz = (const float*)hx; *normals = (const float*)hn; *rgb = (const uint8_t*)hc; *faces = (const int32_t*)hf; *vertex_component = (const int32_t*)hv; *n_vertices = ov; *n_faces = of; }
    }
    if (!rc) { *components = d.list; *n_components = d.nc; }
    hipStreamSynchronize(c->stream);
    d.release();
    return rc;
}

// ---- a level-of-detail mesh by vertex clustering (include/psgsdf_mesh.h; kernels: mesh_lod.hip; DESIGN.md "Level of detail")
namespace {
struct LodOut {
    const float** xyz; const float** normals; const uint8_t** rgb; int64_t* n_vertices; const int32_t** faces; int64_t* n_faces; const int32_t** vertex_map;
    int64_t* n_vertices_in; int64_t* n_faces_in;
};
// from an input mesh on the device (nv > 0, nf > 0; its kernels may still be in flight on the stream) to the pinned host slots 5-8 and 11.  The
// stream has been waited for and every temporary freed when this returns, whatever it returns.
int lod_from_device(psgsdf_ctx* c, const float* xyz, const float* nrm, const unsigned char* rgb, const int* faces, int nv, int nf, double cell, const LodOut& o) {
    const char* me = "extract_mesh_lod";
    if (nv >= (1 << 30) || nf >= (1 << 30)) { hipStreamSynchronize(c->stream); return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %d vertices, %d faces", me, nv, nf); }      // (slots are ints)
    // temporaries: the cluster table of 2 nv slots (8 B key, 10 x 8 B of sums, 4 B smallest member, 4 B used flag), the face table of 2 nf slots (4 B),
    // per vertex its slot, its flag / output number and its map entry, per face its slot and its flag / output number, the scan's sums
    psg::MlodTables t{};
    t.vcap = std::max<unsigned long long>(64, 2ull * (unsigned long long)nv); t.fcap = std::max<unsigned long long>(64, 2ull * (unsigned long long)nf);
    const long long nscan = std::max(nv, nf);
    int *vflag = nullptr, *fflag = nullptr, *sums = nullptr, *vmap = nullptr, *o_faces = nullptr;
    float *o_xyz = nullptr, *o_nrm = nullptr; unsigned char* o_rgb = nullptr;
    auto release = [&] {
        hipFree(t.keys); hipFree(t.acc); hipFree(t.first); hipFree(t.used); hipFree(t.vslot); hipFree(t.ftab); hipFree(t.fslot); hipFree(t.bad);
        hipFree(vflag); hipFree(fflag); hipFree(sums); hipFree(vmap); hipFree(o_faces); hipFree(o_xyz); hipFree(o_nrm); hipFree(o_rgb);
    };
    auto give_up = [&](int code, const char* what) { hipStreamSynchronize(c->stream); release(); return fail(c, code, "%s: %s (%d vertices, %d faces)", me, what, nv, nf); };
    if (hipMalloc(&t.keys, sizeof(unsigned long long) * (size_t)t.vcap) != hipSuccess || hipMalloc(&t.acc, sizeof(long long) * psg::kMlodAcc * (size_t)t.vcap) != hipSuccess
        || hipMalloc(&t.first, sizeof(int) * (size_t)t.vcap) != hipSuccess || hipMalloc(&t.used, sizeof(int) * (size_t)t.vcap) != hipSuccess || hipMalloc(&t.vslot, sizeof(int) * (size_t)nv) != hipSuccess
        || hipMalloc(&t.ftab, sizeof(int) * (size_t)t.fcap) != hipSuccess || hipMalloc(&t.fslot, sizeof(int) * (size_t)nf) != hipSuccess || hipMalloc(&t.bad, sizeof(int)) != hipSuccess
        || hipMalloc(&vflag, sizeof(int) * (size_t)nv) != hipSuccess || hipMalloc(&fflag, sizeof(int) * (size_t)nf) != hipSuccess || hipMalloc(&vmap, sizeof(int) * (size_t)nv) != hipSuccess
        || hipMalloc(&sums, sizeof(int) * (size_t)((nscan + psg::kTile - 1) / psg::kTile + 1)) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "out of memory");
    if (hipMemsetAsync(t.keys, 0xff, sizeof(unsigned long long) * (size_t)t.vcap, c->stream) != hipSuccess || hipMemsetAsync(t.acc, 0, sizeof(long long) * psg::kMlodAcc * (size_t)t.vcap, c->stream) != hipSuccess
        || hipMemsetAsync(t.first, 0x7f, sizeof(int) * (size_t)t.vcap, c->stream) != hipSuccess || hipMemsetAsync(t.used, 0, sizeof(int) * (size_t)t.vcap, c->stream) != hipSuccess
        || hipMemsetAsync(t.ftab, 0xff, sizeof(int) * (size_t)t.fcap, c->stream) != hipSuccess || hipMemsetAsync(t.bad, 0, sizeof(int), c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "memset");
    const double vs = (double)c->grid.vs;
    timed(c, "mlod_cluster", [&] { psg::launch_mlod_cluster(xyz, nrm, rgb, nv, cell, vs, t, c->stream); });
    int bad = 0;
    if (hipMemcpyAsync(&bad, t.bad, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return give_up(PSGSDF_ERR_DEVICE, "kernels");
    if (bad) return give_up(PSGSDF_ERR_UNSUPPORTED, "a cluster coordinate is beyond 2^20: the cell is too small for this mesh");
    timed(c, "mlod_ftable", [&] { psg::launch_mlod_ftable(faces, nf, t, c->stream); });
    timed(c, "mlod_fkeep", [&] { psg::launch_mlod_fkeep(faces, nf, t, fflag, c->stream); });
    timed(c, "mlod_vflag", [&] { psg::launch_mlod_vflag(nv, t, vflag, c->stream); });
    int ov = 0, of = 0;
    int rc = scan_counts(c, vflag, nv, sums, &ov);      // smallest-member flags -> output vertex numbers
    if (!rc) rc = scan_counts(c, fflag, nf, sums, &of);     // kept-face flags -> output face numbers
    if (rc) { hipStreamSynchronize(c->stream); release(); return rc; }
    if (ov > 0 && (hipMalloc(&o_xyz, sizeof(float) * 3 * (size_t)ov) != hipSuccess || hipMalloc(&o_nrm, sizeof(float) * 3 * (size_t)ov) != hipSuccess || hipMalloc(&o_rgb, 3 * (size_t)ov) != hipSuccess
                   || hipMalloc(&o_faces, sizeof(int) * 3 * (size_t)of) != hipSuccess)) return give_up(PSGSDF_ERR_DEVICE, "out of memory");      // (a vertex exists only with a face: of > 0)
    timed(c, "mlod_emit", [&] { psg::launch_mlod_emit(xyz, nrm, rgb, nv, faces, nf, vs, t, vflag, fflag, o_xyz, o_nrm, o_rgb, o_faces, vmap, c->stream); });
    void *hx = nullptr, *hn = nullptr, *hc = nullptr, *hf = nullptr, *hm = nullptr;
    rc = host_out(c, 11, sizeof(int) * (size_t)nv, &hm);
    if (!rc && ov > 0) {
        rc = host_out(c, 5, sizeof(float) * 3 * (size_t)ov, &hx);
        if (!rc) rc = host_out(c, 6, sizeof(float) * 3 * (size_t)ov, &hn);
        if (!rc) rc = host_out(c, 7, 3 * (size_t)ov, &hc);
        if (!rc) rc = host_out(c, 8, sizeof(int) * 3 * (size_t)of, &hf);
    }
    if (!rc) {
        bool cp = hipMemcpyAsync(hm, vmap, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (cp && ov > 0) cp = hipMemcpyAsync(hx, o_xyz, sizeof(float) * 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipMemcpyAsync(hn, o_nrm, sizeof(float) * 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                                && hipMemcpyAsync(hc, o_rgb, 3 * (size_t)ov, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipMemcpyAsync(hf, o_faces, sizeof(int) * 3 * (size_t)of, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (!cp || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: download", me);
    }
    if (!rc) {
        *o.vertex_map = (const int32_t*)hm; *o.n_vertices_in = nv; *o.n_faces_in = nf;
        if (ov > 0) { *o.xyz = (const float*)hx; *o.normals = (const float*)hn; *o.rgb = (const uint8_t*)hc; *o.faces = (const int32_t*)hf; *o.n_vertices = ov; *o.n_faces = of; }
    }
    hipStreamSynchronize(c->stream);
    release();
    return rc;
}
}  // namespace

extern "C" int psgsdf_extract_mesh_lod(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                       const int32_t** faces, int64_t* n_faces, const int32_t** vertex_map, int64_t* n_vertices_in, int64_t* n_faces_in) {
    const char* me = "extract_mesh_lod";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_map || !n_vertices_in || !n_faces_in) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    // (before anything collective and before any device work: no rank waits for another)
    if (c && c->n_ranks > 1) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): clusters are not merged across z-slabs", me, c->rank, c->n_ranks);
    if (!(cell > 0.0) || std::isinf(cell)) return fail(c, PSGSDF_ERR_ARG, "%s: the cell must be a finite size > 0", me);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_map = nullptr; *n_vertices = 0; *n_faces = 0; *n_vertices_in = 0; *n_faces_in = 0;
    const LodOut out{xyz, normals, rgb, n_vertices, faces, n_faces, vertex_map, n_vertices_in, n_faces_in};
    int rc = 0;
    if (!filter) {      // the welded mesh as it is: no component pass
        WMeshDev m;
        rc = wmesh_device(c, &m);
        if (rc) return rc;
        if (m.nv > 0 && m.nf > 0) rc = lod_from_device(c, m.xyz, m.nrm, m.rgb, m.faces, m.nv, m.nf, cell, out);
        else if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me);
        m.release();
        return rc;
    }
    MCompDev d;
    rc = mcomp_device(c, me, *filter, &d);
    if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh: waited for and freed)
    if (d.nv > 0 && d.nf > 0) rc = lod_from_device(c, d.xyz, d.nrm, d.rgb, d.faces, d.nv, d.nf, cell, out);
    else if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PSGSDF_ERR_DEVICE, "%s: kernels", me);
    d.release();
    return rc;
}
