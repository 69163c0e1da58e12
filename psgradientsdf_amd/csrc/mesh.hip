// mesh.hip -- welded, indexed meshes with vertex normals (include/psgsdf_mesh.h psgsdf_extract_mesh_indexed; DESIGN.md "Welded meshes").
// The cells, the table, the face order and the vertex frame are psgsdf_extract_mesh's (extract.hip); what differs is that a vertex belongs to the
// GRID edge, not to the cell: the edge from voxel (i, j, k) to its +x / +y / +z neighbour is interpolated with its lower end point first, so every
// cell that uses it computes the same float, and a vertex that mc_interp snaps onto an end point is that corner's vertex.  Each vertex lives in a
// key slot (engine.h WMeshGrid): 4 per crop voxel, numbered in ascending key order.
//   k_wmesh_mark   one thread per cell: kept faces per cell (a face is dropped iff two of its keys are equal) and a used flag per key (plain stores of 1)
//   k_wmesh_faces  one thread per cell: the kept faces as vertex numbers (exclusive scans of the counts / flags, extract.hip scan_counts)
//   k_wmesh_verts  one thread per key slot: position, normal (the stored gradients, normalised and interpolated), albedo (interpolated, rounded to bytes)
// No atomics: the result is the same bytes on every call.
#include "engine.h"
#include "mc_common.h"

namespace psg {
namespace {

__device__ __forceinline__ long long wlin(const WMeshGrid& g, int i, int j, int k) { return (long long)(k + g.lo[2] - g.zlo) * g.nx * g.ny + (long long)(j + g.lo[1]) * g.nx + (i + g.lo[0]); }
__device__ __forceinline__ int wslot(const WMeshGrid& g, int i, int j, int k, int type) { return (((k - g.zc0) * g.d[1] + j) * g.d[0] + i) * 4 + type; }

// the key slot of cell edge e: its end points in (lower, upper) order along the edge's axis, mc_interp's snap rules in that order
__device__ __forceinline__ int edge_slot(const WMeshGrid& g, int x, int y, int z, int e) {
    const int a = kEdgeD[e][0], b = kEdgeD[e][1];
    const int ax = kCornerD[a][0] != kCornerD[b][0] ? 0 : (kCornerD[a][1] != kCornerD[b][1] ? 1 : 2);
    const int l = kCornerD[a][ax] < kCornerD[b][ax] ? a : b, h = l == a ? b : a;
    const int li = x + kCornerD[l][0], lj = y + kCornerD[l][1], lk = z + kCornerD[l][2];
    const int hi = x + kCornerD[h][0], hj = y + kCornerD[h][1], hk = z + kCornerD[h][2];
    const float tl = -g.dist[wlin(g, li, lj, lk)], th = -g.dist[wlin(g, hi, hj, hk)];
    if ((double)fabsf(0.0f - tl) < 1e-7) return wslot(g, li, lj, lk, 3);
    if ((double)fabsf(0.0f - th) < 1e-7) return wslot(g, hi, hj, hk, 3);
    if ((double)fabsf(tl - th) < 1e-7) return wslot(g, li, lj, lk, 3);
    return wslot(g, li, lj, lk, ax);
}
// the kept faces of one cell, in table order: fn(n, slot0, slot1, slot2); returns their number
template <class Fn>
__device__ __forceinline__ int cell_faces(const WMeshGrid& g, int x, int y, int z, Fn&& fn) {
    int cs = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const long long dl = wlin(g, x + kCornerD[c][0], y + kCornerD[c][1], z + kCornerD[c][2]);
        if (g.weight[dl] == 0.0f) return 0;
        if (-g.dist[dl] > 0.0f) cs |= 1 << c;
    }
    if (cs == 0 || cs == 255) return 0;
    int n = 0;
    for (int q = 0; q + 2 < 16 && kTri[cs][q] >= 0; q += 3) {
        const int s0 = edge_slot(g, x, y, z, kTri[cs][q]), s1 = edge_slot(g, x, y, z, kTri[cs][q + 1]), s2 = edge_slot(g, x, y, z, kTri[cs][q + 2]);
        if (s0 == s1 || s0 == s2 || s1 == s2) continue;
        fn(n, s0, s1, s2);
        ++n;
    }
    return n;
}
__device__ __forceinline__ void cell_of(const WMeshGrid& g, long long c, int& x, int& y, int& z) {
    const int cx = g.d[0] - 2, cy = g.d[1] - 2;
    const int zl = (int)(c / ((long long)cx * cy)), rest = (int)(c - (long long)zl * cx * cy);
    y = rest / cx; x = rest - y * cx; z = zl + g.zc0;
}

__global__ void __launch_bounds__(kBlock) k_wmesh_mark(WMeshGrid g, long long ncell, int* __restrict__ cnt, int* __restrict__ flag) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    int x, y, z; cell_of(g, c, x, y, z);
    cnt[c] = cell_faces(g, x, y, z, [&](int, int s0, int s1, int s2) { flag[s0] = 1; flag[s1] = 1; flag[s2] = 1; });
}
__global__ void __launch_bounds__(kBlock) k_wmesh_or(int* __restrict__ dst, const int* __restrict__ src, long long n) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) dst[i] |= src[i];
}
__global__ void __launch_bounds__(kBlock) k_wmesh_faces(WMeshGrid g, long long ncell, const int* __restrict__ offs, int n_faces, const int* __restrict__ num, int first,
                                                         const int* __restrict__ num_up, int first_up, int* __restrict__ faces) {
    const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const int f0 = offs[c];
    if ((c + 1 < ncell ? offs[c + 1] : n_faces) == f0) return;
    int x, y, z; cell_of(g, c, x, y, z);
    auto number = [&](int s) { return s < g.nown ? num[s] + first : num_up[s - g.nown] + first_up; };
    cell_faces(g, x, y, z, [&](int n, int s0, int s1, int s2) {
        int* f = faces + 3 * (size_t)(f0 + n);
        f[0] = number(s0); f[1] = number(s1); f[2] = number(s2);
    });
}

// the stored gradient of a voxel, normalised (a zero gradient stays zero); albedo
__device__ __forceinline__ void unit_grad(const float* const gp[3], long long q, float out[3]) {
    out[0] = gp[0][q]; out[1] = gp[1][q]; out[2] = gp[2][q];
    const float z = out[0] * out[0] + out[1] * out[1] + out[2] * out[2];
    if (z > 0) { const float s = sqrtf(z); out[0] /= s; out[1] /= s; out[2] /= s; }
}
__device__ __forceinline__ unsigned char colour_byte(float c) { return (unsigned char)(int)floorf(255.0f * fminf(fmaxf(c, 0.0f), 1.0f) + 0.5f); }

__global__ void __launch_bounds__(kBlock) k_wmesh_verts(WMeshGrid g, const int* __restrict__ num, int n_verts, float* __restrict__ xyz, float* __restrict__ nrm, unsigned char* __restrict__ rgb) {
    const long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (s >= g.nown) return;
    const int v = num[s];
    if ((s + 1 < g.nown ? num[s + 1] : n_verts) == v) return;      // an unused key
    const int type = (int)(s & 3), q = (int)(s >> 2);
    const int i = q % g.d[0], j = (q / g.d[0]) % g.d[1], k = q / (g.d[0] * g.d[1]) + g.zc0;
    const int p[3] = {i, j, k};
    float pl[3], gl[3], cl[3];
    const long long dl = wlin(g, i, j, k);
#pragma unroll
    for (int a = 0; a < 3; ++a) pl[a] = (p[a] + g.poff[a]) * g.voxel[a] - g.origin[a];      // voxelToWorld, as extract.hip mc_cell
    unit_grad(g.g, dl, gl);
    for (int a = 0; a < 3; ++a) cl[a] = g.rho[a][dl];
    float pos[3], n[3], col[3];
    if (type == 3) {      // a corner: its own position, gradient and albedo
        for (int a = 0; a < 3; ++a) { pos[a] = pl[a]; n[a] = gl[a]; col[a] = cl[a]; }
    } else {
        const int ph[3] = {i + (type == 0), j + (type == 1), k + (type == 2)};
        float phf[3], gh[3], ch[3];
        for (int a = 0; a < 3; ++a) phf[a] = (ph[a] + g.poff[a]) * g.voxel[a] - g.origin[a];
        const long long dh = wlin(g, ph[0], ph[1], ph[2]);
        if (ph[2] + g.lo[2] == g.zh) {      // the upper end in the plane above this slab: gradient and albedo from the exchanged plane
            const long long hq = (long long)(ph[1] + g.lo[1]) * g.nx + (ph[0] + g.lo[0]);
            unit_grad(g.hg, hq, gh);
            for (int a = 0; a < 3; ++a) ch[a] = g.hrho[a][hq];
        } else {
            unit_grad(g.g, dh, gh);
            for (int a = 0; a < 3; ++a) ch[a] = g.rho[a][dh];
        }
        const float tl = -g.dist[dl], th = -g.dist[dh];
        mc_interp(tl, th, pl, phf, pos);
        double mu = (double)((0.0f - tl) / (th - tl));      // mc_interp's interpolation parameter (the key was not snapped)
        if (mu > 1.0) mu = 1.0; else if (mu < 0) mu = 0.0;
        const float m = (float)mu;
        for (int a = 0; a < 3; ++a) { n[a] = gl[a] + m * (gh[a] - gl[a]); col[a] = cl[a] + m * (ch[a] - cl[a]); }
        const float z = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        if (z > 0) { const float r = sqrtf(z); n[0] /= r; n[1] /= r; n[2] /= r; }
    }
    for (int a = 0; a < 3; ++a) { xyz[3 * (size_t)v + a] = pos[a]; nrm[3 * (size_t)v + a] = n[a]; rgb[3 * (size_t)v + a] = colour_byte(col[a]); }
}

unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + kBlock - 1) / kBlock); }

}  // namespace

void launch_wmesh_mark(const WMeshGrid& g, long long ncell, int* cnt, int* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_mark, dim3(blocks(ncell)), dim3(kBlock), 0, s, g, ncell, cnt, flag);
}
void launch_wmesh_or(int* dst, const int* src, long long n, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_or, dim3(blocks(n)), dim3(kBlock), 0, s, dst, src, n);
}
void launch_wmesh_faces(const WMeshGrid& g, long long ncell, const int* offs, int n_faces, const int* num, int first, const int* num_up, int first_up, int* faces, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_faces, dim3(blocks(ncell)), dim3(kBlock), 0, s, g, ncell, offs, n_faces, num, first, num_up, first_up, faces);
}
void launch_wmesh_verts(const WMeshGrid& g, const int* num, int n_verts, float* xyz, float* nrm, unsigned char* rgb, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_verts, dim3(blocks(g.nown)), dim3(kBlock), 0, s, g, num, n_verts, xyz, nrm, rgb);
}

}  // namespace psg
