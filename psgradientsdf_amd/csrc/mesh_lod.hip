// mesh_lod.hip -- a level-of-detail mesh by vertex clustering (include/psgsdf_mesh.h psgsdf_extract_mesh_lod; DESIGN.md "Level of detail").
// Input: the device arrays of psgsdf_extract_mesh_indexed, or of psgsdf_extract_mesh_components after its compaction.
//   k_mlod_cluster   one thread per vertex: the cluster key (floor of the double quotient per axis, 3 x 21 bits) into an open-addressing table
//                    (64-bit atomicCAS, linear probing); into the slot: members, the fixed-point sums of positions and normals, the sums of the
//                    colour bytes (64-bit integer atomicAdd), the smallest member (atomicMin)
//   k_mlod_ftable    one thread per face: collapsed (two clusters equal)?  Otherwise into a second table whose slots hold a FACE INDEX: an empty slot
//                    is claimed (atomicCAS); an occupied one holds a face of some triple -- the same unordered triple: atomicMin of the own index,
//                    another: probe on.  A slot only ever changes to a face of the same triple, faces of one triple follow one probe sequence, so
//                    they meet in one slot and it ends up with the smallest index whatever the order
//   k_mlod_fkeep     one thread per face: kept iff its slot holds its own index; the three clusters of a kept face flagged used
//   k_mlod_vflag     one thread per vertex: 1 on the smallest member of every used cluster; the exclusive scan of these flags numbers the output
//                    vertices in ascending smallest member, that of the face flags the kept faces in input order (extract.hip scan_counts)
//   k_mlod_emit      one thread per vertex / face: the map of every input vertex, the output vertex of every smallest member, the kept faces
// Integer atomics only and every sum an integer sum: the same bytes on every call.  Vertices arrive in key order (z-major, x fastest), so the lanes
// of a wavefront that share a cluster are mostly neighbours: k_mlod_cluster sums each run of adjacent lanes with equal slots through shuffles and
// the run's first lane issues the atomics -- with a coarse cell that is 11 atomics per wavefront rather than 64 x 11 on one address.
#include "engine.h"
#include "mesh_lod.h"

namespace psg {
namespace {

#pragma clang fp contract(off)

constexpr unsigned long long kEmpty = ~0ull;      // (a key has 63 bits)

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
__device__ __forceinline__ unsigned long long mix(unsigned long long x, unsigned long long cap) { return __umul64hi(x * 0x9E3779B97F4A7C15ull, cap); }      // [0, cap)

// sum over the lanes [lane, lane + len) -- the rest of this lane's run; every lane of the wavefront must call
template <class T>
__device__ __forceinline__ T run_sum(T v, int len) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_down(v, o, 64); if (o < len) v += t; }
    return v;
}

__global__ void __launch_bounds__(kBlock) k_mlod_cluster(const float* __restrict__ xyz, const float* __restrict__ nrm, const unsigned char* __restrict__ rgb, int nv, double cell, double vs, MlodTables t) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    int slot = -1, one = 0, col[3] = {0, 0, 0};
    long long p[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    if (v < nv) {
        double c[3]; bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) { c[a] = floor((double)xyz[3 * (size_t)v + a] / cell); ok = ok && fabs(c[a]) < (double)kMlodLimit; }      // an IEEE division: its bits decide on which side of a wall a vertex is
        if (ok) {
            const unsigned long long key = ((unsigned long long)((long long)c[0] + kMlodLimit) << 42) | ((unsigned long long)((long long)c[1] + kMlodLimit) << 21) | (unsigned long long)((long long)c[2] + kMlodLimit);
            unsigned long long h = mix(key, t.vcap);
            for (;;) {      // (at most half of the slots are ever taken)
                const unsigned long long old = atomicCAS(t.keys + h, kEmpty, key);
                if (old == kEmpty || old == key) break;
                if (++h == t.vcap) h = 0;
            }
            slot = (int)h; one = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[a] = llrint((double)xyz[3 * (size_t)v + a] * kMlodFix / vs);
                q[a] = llrint((double)nrm[3 * (size_t)v + a] * kMlodFix);
                col[a] = rgb[3 * (size_t)v + a];
            }
        } else atomicOr(t.bad, 1);
        t.vslot[v] = slot;
    }
    // runs of adjacent lanes with the same slot
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(slot, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != slot);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);      // bit k: lane + 1 + k starts a run
    const int len = above ? __ffsll((long long)above) : 64 - lane;
    const int n = run_sum(one, len);
#pragma unroll
    for (int a = 0; a < 3; ++a) { p[a] = run_sum(p[a], len); q[a] = run_sum(q[a], len); col[a] = run_sum(col[a], len); }
    if (((heads >> lane) & 1) && slot >= 0) {
        long long* acc = t.acc + (size_t)slot * kMlodAcc;
        add64(acc + ML_COUNT, n);
#pragma unroll
        for (int a = 0; a < 3; ++a) { add64(acc + ML_POS + a, p[a]); add64(acc + ML_NRM + a, q[a]); add64(acc + ML_RGB + a, col[a]); }
        atomicMin(t.first + slot, v);      // (the run's first lane has its smallest vertex)
    }
}

struct Tri { int a, b, c; };
// the face's clusters in ascending order
__device__ __forceinline__ Tri sorted_triple(const int* __restrict__ faces, const int* __restrict__ vslot, int f) {
    int a = vslot[faces[3 * (size_t)f]], b = vslot[faces[3 * (size_t)f + 1]], c = vslot[faces[3 * (size_t)f + 2]];
    if (a > b) { const int x = a; a = b; b = x; }
    if (b > c) { const int x = b; b = c; c = x; }
    if (a > b) { const int x = a; a = b; b = x; }
    return {a, b, c};
}
__global__ void __launch_bounds__(kBlock) k_mlod_ftable(const int* __restrict__ faces, int nf, MlodTables t) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const Tri m = sorted_triple(faces, t.vslot, f);
    if (m.a == m.b || m.b == m.c) { t.fslot[f] = -1; return; }
    unsigned long long h = mix((((unsigned long long)(unsigned)m.a << 32) | (unsigned)m.b) * 0xD6E8FEB86659FD93ull + (unsigned)m.c, t.fcap);
    for (;;) {      // (at most half of the slots are ever taken)
        const int old = atomicCAS(t.ftab + h, -1, f);
        if (old == -1) break;
        const Tri o = sorted_triple(faces, t.vslot, old);
        if (o.a == m.a && o.b == m.b && o.c == m.c) {
            if (f < old) atomicMin(t.ftab + h, f);      // (the slot only ever decreases)
            break;
        }
        if (++h == t.fcap) h = 0;
    }
    t.fslot[f] = (int)h;
}
__global__ void __launch_bounds__(kBlock) k_mlod_fkeep(const int* __restrict__ faces, int nf, MlodTables t, int* __restrict__ fflag) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const int h = t.fslot[f];
    const bool keep = h >= 0 && t.ftab[h] == f;
    fflag[f] = keep ? 1 : 0;
    if (keep)
        for (int k = 0; k < 3; ++k) t.used[t.vslot[faces[3 * (size_t)f + k]]] = 1;
}
__global__ void __launch_bounds__(kBlock) k_mlod_vflag(int nv, MlodTables t, int* __restrict__ vflag) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int s = t.vslot[v];
    vflag[v] = (t.used[s] && t.first[s] == v) ? 1 : 0;
}
__global__ void __launch_bounds__(kBlock) k_mlod_emit(const float* __restrict__ xyz, const float* __restrict__ nrm, const unsigned char* __restrict__ rgb, int nv, const int* __restrict__ faces, int nf, double vs,
                                                       MlodTables t, const int* __restrict__ vnum, const int* __restrict__ fnum,
                                                       float* __restrict__ oxyz, float* __restrict__ onrm, unsigned char* __restrict__ orgb, int* __restrict__ ofaces, int* __restrict__ vmap) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nv) {
        const int s = t.vslot[i];
        if (!t.used[s]) vmap[i] = -1;
        else {
            const int fv = t.first[s], o = vnum[fv];
            vmap[i] = o;
            if (fv == i) {
                const long long* acc = t.acc + (size_t)s * kMlodAcc;
                const long long n = acc[ML_COUNT];
                if (n == 1) {      // a single member: its own bits
                    for (int a = 0; a < 3; ++a) { oxyz[3 * (size_t)o + a] = xyz[3 * (size_t)i + a]; onrm[3 * (size_t)o + a] = nrm[3 * (size_t)i + a]; orgb[3 * (size_t)o + a] = rgb[3 * (size_t)i + a]; }
                } else {
                    const double tx = (double)acc[ML_NRM], ty = (double)acc[ML_NRM + 1], tz = (double)acc[ML_NRM + 2];
                    const double len = sqrt((tx * tx + ty * ty) + tz * tz);
                    const double tn[3] = {tx, ty, tz};
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        oxyz[3 * (size_t)o + a] = (float)((double)acc[ML_POS + a] / (double)n * (vs / kMlodFix));      // division, product, one rounding to float
                        onrm[3 * (size_t)o + a] = len > 0.0 ? (float)(tn[a] / len) : 0.0f;
                        orgb[3 * (size_t)o + a] = (unsigned char)((2 * acc[ML_RGB + a] + n) / (2 * n));
                    }
                }
            }
        }
    }
    if (i < nf) {
        const int h = t.fslot[i];
        if (h >= 0 && t.ftab[h] == i) {
            const size_t o = 3 * (size_t)fnum[i];
            for (int k = 0; k < 3; ++k) ofaces[o + k] = vnum[t.first[t.vslot[faces[3 * (size_t)i + k]]]];
        }
    }
}

unsigned blocks(long long n) { return (unsigned)std::max<long long>(1, (n + kBlock - 1) / kBlock); }

}  // namespace

void launch_mlod_cluster(const float* xyz, const float* nrm, const unsigned char* rgb, int nv, double cell, double vs, const MlodTables& t, hipStream_t s) {
    hipLaunchKernelGGL(k_mlod_cluster, dim3(blocks(nv)), dim3(kBlock), 0, s, xyz, nrm, rgb, nv, cell, vs, t);
}
void launch_mlod_ftable(const int* faces, int nf, const MlodTables& t, hipStream_t s) { hipLaunchKernelGGL(k_mlod_ftable, dim3(blocks(nf)), dim3(kBlock), 0, s, faces, nf, t); }
void launch_mlod_fkeep(const int* faces, int nf, const MlodTables& t, int* fflag, hipStream_t s) { hipLaunchKernelGGL(k_mlod_fkeep, dim3(blocks(nf)), dim3(kBlock), 0, s, faces, nf, t, fflag); }
void launch_mlod_vflag(int nv, const MlodTables& t, int* vflag, hipStream_t s) { hipLaunchKernelGGL(k_mlod_vflag, dim3(blocks(nv)), dim3(kBlock), 0, s, nv, t, vflag); }
void launch_mlod_emit(const float* xyz, const float* nrm, const unsigned char* rgb, int nv, const int* faces, int nf, double vs, const MlodTables& t, const int* vnum, const int* fnum,
                      float* oxyz, float* onrm, unsigned char* orgb, int* ofaces, int* vmap, hipStream_t s) {
    hipLaunchKernelGGL(k_mlod_emit, dim3(blocks(std::max(nv, nf))), dim3(kBlock), 0, s, xyz, nrm, rgb, nv, faces, nf, vs, t, vnum, fnum, oxyz, onrm, orgb, ofaces, vmap);
}

}  // namespace psg
