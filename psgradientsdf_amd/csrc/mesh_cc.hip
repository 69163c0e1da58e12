// mesh_cc.hip -- connected components of the welded mesh (include/psgsdf_mesh.h psgsdf_extract_mesh_components; DESIGN.md "Mesh components").
// Input: the device arrays of psgsdf_extract_mesh_indexed (positions, faces as vertex numbers).  Two vertices are connected iff a face uses both.
//   k_mcomp_init      parent[v] = v
//   k_mcomp_hook      one thread per face: union (a, b) and (b, c).  A root is only ever hooked (atomicCAS) below a SMALLER vertex number, so the root
//                     of a component ends up as its smallest vertex whatever the schedule; finds halve the paths they walk
//   k_mcomp_flatten   one thread per vertex: parent[v] = root(v), flag[v] = (root == v); the exclusive scan of the flags numbers the components in
//                     ascending first vertex (extract.hip scan_counts)
//   k_mcomp_vstats    one thread per vertex: its component number, vertices per component, bounding box (float min / max as ordered integers)
//   k_mcomp_fstats    one thread per face: faces per component, area in fixed point (64-bit integer adds of llrint(2^24 A_f / vs^2))
//   k_mcomp_edges     one thread per face: its three undirected edges (min << 32 | max) into an open-addressing table, use count per slot
//   k_mcomp_ecount    one thread per slot: edges / boundary edges (used once) / non-manifold edges (used more than twice) of the lower vertex's component
//   k_mcomp_keep      kept flags per vertex and face from the components' kept flags;  k_mcomp_compact  the kept vertices / faces, renumbered
// Integer atomics only, every sum an integer sum: the same bytes on every call.  One component usually holds nearly every face, so the lanes of a
// wavefront that agree on the component combine their contribution first and one of them issues the atomic (wave_groups).
#include "engine.h"

namespace psg {
namespace {

#pragma clang fp contract(off)

__device__ __forceinline__ int ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void st(int* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// root of v; every vertex on the way is re-pointed at its grandparent (a non-root's parent only ever moves towards the root)
__device__ __forceinline__ int find_root(int* parent, int v) {
    int p = ld(parent + v);
    while (p != v) {
        const int gp = ld(parent + p);
        if (gp != p) st(parent + v, gp);
        v = p; p = gp;
    }
    return v;
}
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a); b = find_root(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        if (atomicCAS(parent + hi, hi, lo) == hi) return;      // (lost: hi was hooked elsewhere in the meantime; find again)
    }
}

__global__ void __launch_bounds__(kBlock) k_mcomp_init(int* __restrict__ parent, int nv) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) parent[v] = v;
}
__global__ void __launch_bounds__(kBlock) k_mcomp_hook(const int* __restrict__ faces, int nf, int* parent) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    unite(parent, a, b);
    unite(parent, b, c);
}
__global__ void __launch_bounds__(kBlock) k_mcomp_flatten(int* parent, int nv, int* __restrict__ flag) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    int r = v;
    for (int p = ld(parent + r); p != r; p = ld(parent + r)) r = p;
    st(parent + v, r);
    flag[v] = r == v ? 1 : 0;
}

// the lanes of the wavefront grouped by component: fn(mine, leader) once per distinct component among the valid lanes, with every lane of the
// wavefront active (mine: this lane belongs to the group; leader: this lane issues the group's atomics).  Every thread of the wavefront must call.
template <class Fn>
__device__ __forceinline__ void wave_groups(bool valid, int comp, Fn&& fn) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(comp, leader, 64);
        const bool mine = valid && comp == lc;
        fn(mine, lane == leader);
        todo &= ~__ballot(mine);
    }
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
// float -> unsigned with the same order (and back on the host: extract.hip)
__device__ __forceinline__ unsigned ordered(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__global__ void __launch_bounds__(kBlock) k_mcomp_vstats(const int* __restrict__ parent, const int* __restrict__ num, int nv, const float* __restrict__ xyz, int* __restrict__ vcomp,
                                                          long long* __restrict__ stat, unsigned* __restrict__ blo, unsigned* __restrict__ bhi) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = v < nv;
    int comp = -1; float p[3] = {0, 0, 0};
    if (valid) {
        const int r = parent[v];
        comp = num[r];
        vcomp[v] = comp;
        if (r == v) stat[(size_t)comp * kMcompStats + MC_FIRST] = v;
        for (int a = 0; a < 3; ++a) p[a] = xyz[3 * (size_t)v + a];
    }
    wave_groups(valid, comp, [&](bool mine, bool leader) {
        const long long n = wave_sum(mine ? 1 : 0);
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = wave_min(mine ? p[a] : INFINITY); hi[a] = wave_max(mine ? p[a] : -INFINITY); }
        if (leader) {
            add64(stat + (size_t)comp * kMcompStats + MC_VERTS, n);
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(blo + 3 * (size_t)comp + a, ordered(lo[a])); atomicMax(bhi + 3 * (size_t)comp + a, ordered(hi[a])); }
        }
    });
}
__global__ void __launch_bounds__(kBlock) k_mcomp_fstats(const int* __restrict__ faces, int nf, const int* __restrict__ vcomp, const float* __restrict__ xyz, double vs2,
                                                          long long* __restrict__ stat) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = f < nf;
    int comp = -1; long long q = 0;
    if (valid) {
        const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
        comp = vcomp[i0];
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { const double p0 = (double)xyz[3 * (size_t)i0 + k]; a[k] = (double)xyz[3 * (size_t)i1 + k] - p0; b[k] = (double)xyz[3 * (size_t)i2 + k] - p0; }
        const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
        const double area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
        q = llrint(16777216.0 * area / vs2);      // 2^24 A_f / vs^2, the definition's order of operations
    }
    wave_groups(valid, comp, [&](bool mine, bool leader) {
        const long long n = wave_sum(mine ? 1 : 0), s = wave_sum(mine ? q : 0);
        if (leader) { add64(stat + (size_t)comp * kMcompStats + MC_FACES, n); add64(stat + (size_t)comp * kMcompStats + MC_AREA, s); }
    });
}

constexpr unsigned long long kEmpty = ~0ull;
__device__ __forceinline__ void edge_insert(unsigned long long* keys, int* uses, unsigned long long cap, int a, int b) {
    const unsigned long long key = ((unsigned long long)(unsigned)min(a, b) << 32) | (unsigned)max(a, b);
    unsigned long long h = __umul64hi(key * 0x9E3779B97F4A7C15ull, cap);      // [0, cap)
    for (;;) {      // (at most half of the slots are ever taken: a free or matching slot is found)
        const unsigned long long old = atomicCAS(keys + h, kEmpty, key);
        if (old == kEmpty || old == key) { atomicAdd(uses + h, 1); return; }
        if (++h == cap) h = 0;
    }
}
__global__ void __launch_bounds__(kBlock) k_mcomp_edges(const int* __restrict__ faces, int nf, unsigned long long* keys, int* uses, unsigned long long cap) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    edge_insert(keys, uses, cap, a, b);
    edge_insert(keys, uses, cap, b, c);
    edge_insert(keys, uses, cap, c, a);
}
__global__ void __launch_bounds__(kBlock) k_mcomp_ecount(const unsigned long long* __restrict__ keys, const int* __restrict__ uses, unsigned long long cap, const int* __restrict__ vcomp,
                                                          long long* __restrict__ stat) {
    const unsigned long long s = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
    const unsigned long long key = s < cap ? keys[s] : kEmpty;
    const bool valid = key != kEmpty;
    int comp = -1, u = 0;
    if (valid) { comp = vcomp[(int)(key >> 32)]; u = uses[s]; }
    wave_groups(valid, comp, [&](bool mine, bool leader) {
        const long long e = wave_sum(mine ? 1 : 0), b = wave_sum(mine && u == 1 ? 1 : 0), m = wave_sum(mine && u > 2 ? 1 : 0);
        if (leader) {
            long long* st_ = stat + (size_t)comp * kMcompStats;
            add64(st_ + MC_EDGES, e);
            if (b) add64(st_ + MC_BOUNDARY, b);
            if (m) add64(st_ + MC_NONMANIFOLD, m);
        }
    });
}

__global__ void __launch_bounds__(kBlock) k_mcomp_keep(const int* __restrict__ kept, const int* __restrict__ vcomp, int nv, const int* __restrict__ faces, int nf,
                                                        int* __restrict__ vflag, int* __restrict__ fflag) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nv) vflag[i] = kept[vcomp[i]];
    if (i < nf) fflag[i] = kept[vcomp[faces[3 * (size_t)i]]];
}
// vnum / fnum: the exclusive scans of the kept flags
__global__ void __launch_bounds__(kBlock) k_mcomp_compact(const int* __restrict__ kept, const int* __restrict__ vcomp, int nv, const int* __restrict__ faces, int nf,
                                                           const int* __restrict__ vnum, const int* __restrict__ fnum,
                                                           const float* __restrict__ xyz, const float* __restrict__ nrm, const unsigned char* __restrict__ rgb,
                                                           float* __restrict__ oxyz, float* __restrict__ onrm, unsigned char* __restrict__ orgb, int* __restrict__ ovcomp, int* __restrict__ ofaces) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nv && kept[vcomp[i]]) {
        const size_t o = 3 * (size_t)vnum[i], s = 3 * (size_t)i;
        for (int a = 0; a < 3; ++a) { oxyz[o + a] = xyz[s + a]; onrm[o + a] = nrm[s + a]; orgb[o + a] = rgb[s + a]; }
        ovcomp[vnum[i]] = vcomp[i];
    }
    if (i < nf) {
        const size_t s = 3 * (size_t)i;
        const int a = faces[s];
        if (kept[vcomp[a]]) {
            const size_t o = 3 * (size_t)fnum[i];
            ofaces[o] = vnum[a]; ofaces[o + 1] = vnum[faces[s + 1]]; ofaces[o + 2] = vnum[faces[s + 2]];
        }
    }
}

unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + kBlock - 1) / kBlock); }

}  // namespace

void launch_mcomp_init(int* parent, int nv, hipStream_t s) { hipLaunchKernelGGL(k_mcomp_init, dim3(blocks(nv)), dim3(kBlock), 0, s, parent, nv); }
void launch_mcomp_hook(const int* faces, int nf, int* parent, hipStream_t s) { hipLaunchKernelGGL(k_mcomp_hook, dim3(blocks(nf)), dim3(kBlock), 0, s, faces, nf, parent); }
void launch_mcomp_flatten(int* parent, int nv, int* flag, hipStream_t s) { hipLaunchKernelGGL(k_mcomp_flatten, dim3(blocks(nv)), dim3(kBlock), 0, s, parent, nv, flag); }
void launch_mcomp_vstats(const int* parent, const int* num, int nv, const float* xyz, int* vcomp, long long* stat, unsigned* blo, unsigned* bhi, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_vstats, dim3(blocks(nv)), dim3(kBlock), 0, s, parent, num, nv, xyz, vcomp, stat, blo, bhi);
}
void launch_mcomp_fstats(const int* faces, int nf, const int* vcomp, const float* xyz, double vs2, long long* stat, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_fstats, dim3(blocks(nf)), dim3(kBlock), 0, s, faces, nf, vcomp, xyz, vs2, stat);
}
void launch_mcomp_edges(const int* faces, int nf, unsigned long long* keys, int* uses, unsigned long long cap, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_edges, dim3(blocks(nf)), dim3(kBlock), 0, s, faces, nf, keys, uses, cap);
}
void launch_mcomp_ecount(const unsigned long long* keys, const int* uses, unsigned long long cap, const int* vcomp, long long* stat, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_ecount, dim3(blocks((long long)cap)), dim3(kBlock), 0, s, keys, uses, cap, vcomp, stat);
}
void launch_mcomp_keep(const int* kept, const int* vcomp, int nv, const int* faces, int nf, int* vflag, int* fflag, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_keep, dim3(blocks(std::max(nv, nf))), dim3(kBlock), 0, s, kept, vcomp, nv, faces, nf, vflag, fflag);
}
void launch_mcomp_compact(const int* kept, const int* vcomp, int nv, const int* faces, int nf, const int* vnum, const int* fnum, const float* xyz, const float* nrm,
                          const unsigned char* rgb, float* oxyz, float* onrm, unsigned char* orgb, int* ovcomp, int* ofaces, hipStream_t s) {
    hipLaunchKernelGGL(k_mcomp_compact, dim3(blocks(std::max(nv, nf))), dim3(kBlock), 0, s, kept, vcomp, nv, faces, nf, vnum, fnum, xyz, nrm, rgb, oxyz, onrm, orgb, ovcomp, ofaces);
}

}  // namespace psg
