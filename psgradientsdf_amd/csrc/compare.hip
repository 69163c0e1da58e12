// compare.hip -- nearest-primitive search between the welded mesh and a reference mesh or cloud (include/psgsdf_compare.h):
//   k_cmp_total / k_cmp_count / k_cmp_fill   a uniform grid over one direction's targets by a counting sort: one lane per target; the cells its
//            bounding box overlaps are counted (a 64-bit total first, which the host checks against 2^31 - 1 before anything is sized by it), then
//            per cell with integer atomics, scanned (extract.hip scan_counts), filled through a per-cell cursor.  The order inside a cell is
//            whatever the atomics give; the query's min-with-index rule makes the result independent of it, duplicates are harmless.
//   k_cmp_query   one wavefront per query, four per workgroup, consecutive queries in consecutive wavefronts (mesh vertices come in key order
//            (z, y, x): neighbouring wavefronts read neighbouring cells).  The cells are visited in shells of growing Chebyshev radius around the
//            query's cell; a shell is a set of x-rows, and the entries of a row's cells are contiguous, so the lanes stride over each row's segment
//            and keep their own best (D2, index).  After every shell one butterfly reduces the pair lexicographically -- every lane then holds
//            the wavefront's best -- and the search stops once the distance to the nearest unvisited cell, taken 1e-6 on the conservative side,
//            exceeds the best found or max_dist.  All loop bounds are wave-uniform.  Lane 0 stores.  No LDS, no scratch.
//   k_cmp_stats   a grid-stride loop, one lane per query and turn: a lane's sums, then wave sums and one integer atomicAdd per wavefront and field, the
//            maximum by an integer atomicMax on the double's bits (d >= 0).  No floating-point atomics: the same bits in whatever order.
// The pair function is the definition's, operation for operation, with contraction off; / and sqrt are the IEEE ones (no fast-math flag in the
// file's build line; the assembly has the v_div_scale / v_div_fmas / v_div_fixup and the refined v_rsq_f64 sequences).
#pragma clang fp contract(off)
#include "compare_device.h"      // cmp_dot, cmp_target, cmp_pair: shared with align.hip

namespace psg {
namespace {

// the cell of coordinate x along axis k, as a double clamped to [-1, n]: monotone in x
__device__ __forceinline__ int cmp_cell(const CompareGrid& g, double x, int k) {
    const double t = floor((x - g.lo[k]) / g.h);
    return (int)fmin(fmax(t, -1.0), (double)g.n[k]);
}

// the cells target t's bounding box overlaps, clamped to the grid: false if it has a non-finite corner or lies outside
__device__ __forceinline__ bool cmp_target_cells(const CompareArgs& a, int t, int* c0, int* c1) {
    double A[3], B[3], C[3];
    cmp_target(a, t, A, B, C);
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = fmin(A[k], fmin(B[k], C[k])), hi = fmax(A[k], fmax(B[k], C[k]));
        in = in && isfinite(A[k]) && isfinite(B[k]) && isfinite(C[k]);
        c0[k] = cmp_cell(a.g, lo, k); c1[k] = cmp_cell(a.g, hi, k);
        in = in && c1[k] >= 0 && c0[k] < a.g.n[k];
        c0[k] = max(c0[k], 0); c1[k] = min(c1[k], a.g.n[k] - 1);
    }
    return in;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(kBlock) k_cmp_total(CompareArgs a) {
    const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
    int c0[3], c1[3];
    long long cnt = 0;
    if (t < a.nt && cmp_target_cells(a, (int)t, c0, c1)) cnt = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    cnt = wave_sum_ll(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(a.total, (unsigned long long)cnt);
}

template <bool FILL>
__global__ void __launch_bounds__(kBlock) k_cmp_cells(CompareArgs a) {
    const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
    int c0[3], c1[3];
    if (t >= a.nt || !cmp_target_cells(a, (int)t, c0, c1)) return;
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y) {
            const long long row = ((long long)z * a.g.n[1] + y) * a.g.n[0];
            for (int x = c0[0]; x <= c1[0]; ++x) {
                if (FILL) a.g.entries[a.g.start[row + x] + atomicAdd(a.g.cursor + row + x, 1)] = (int)t;
                else atomicAdd(a.g.start + row + x, 1);
            }
        }
}

// the lanes stride over entries [s0, s1): each keeps its own best (D2, index)
__device__ __forceinline__ void cmp_scan(const CompareArgs& a, const double* p, int s0, int s1, int lane, double& best, int& bi) {
    for (int e = s0 + lane; e < s1; e += 64) {
        const int t = a.g.entries[e];
        double A[3], B[3], C[3], q[3];
        cmp_target(a, t, A, B, C);
        const double D2 = cmp_pair(p, A, B, C, q);
        if (D2 < best || (D2 == best && t < bi)) { best = D2; bi = t; }
    }
}

__global__ void __launch_bounds__(kBlock) k_cmp_query(CompareArgs a) {
    const int lane = threadIdx.x & 63;
    const long long qi = a.q0 + (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (qi >= a.q1) return;
    const CompareGrid& g = a.g;
    double p[3];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = (double)a.q_xyz[3 * qi + k]; valid = valid && isfinite(p[k]); }
    const double margin = 1e-6 * g.h;
    double best = INFINITY; int bi = INT_MAX; long long pairs = 0;
    // a query farther from the grid's box than max_dist (conservatively) has no match: no search
    bool search = valid && g.start != nullptr;
    int cq[3] = {0, 0, 0};
    if (search) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double out = fmax(fmax(g.lo[k] - p[k], p[k] - (g.lo[k] + (double)g.n[k] * g.h)), 0.0);
            search = search && !(out * (1.0 - 1e-6) - margin > a.max_dist);
            cq[k] = min(max(cmp_cell(g, p[k], k), 0), g.n[k] - 1);
        }
    }
    if (search) {
        for (int r = 0;; ++r) {
            const int z0 = max(cq[2] - r, 0), z1 = min(cq[2] + r, g.n[2] - 1), y0 = max(cq[1] - r, 0), y1 = min(cq[1] + r, g.n[1] - 1);
            const int xa = cq[0] - r, xb = cq[0] + r, xa_c = max(xa, 0), xb_c = min(xb, g.n[0] - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const long long row = ((long long)z * g.n[1] + y) * g.n[0];
                    if (z - cq[2] == r || cq[2] - z == r || y - cq[1] == r || cq[1] - y == r) {      // a row of the shell's z or y face: all of its cells
                        const int s0 = __builtin_amdgcn_readfirstlane(g.start[row + xa_c]), s1 = __builtin_amdgcn_readfirstlane(g.start[row + xb_c + 1]);
                        pairs += s1 - s0;
                        cmp_scan(a, p, s0, s1, lane, best, bi);
                    } else {                                                                          // an inner row: its two end cells (r > 0 here)
                        if (xa >= 0) {
                            const int s0 = __builtin_amdgcn_readfirstlane(g.start[row + xa]), s1 = __builtin_amdgcn_readfirstlane(g.start[row + xa + 1]);
                            pairs += s1 - s0;
                            cmp_scan(a, p, s0, s1, lane, best, bi);
                        }
                        if (xb < g.n[0]) {
                            const int s0 = __builtin_amdgcn_readfirstlane(g.start[row + xb]), s1 = __builtin_amdgcn_readfirstlane(g.start[row + xb + 1]);
                            pairs += s1 - s0;
                            cmp_scan(a, p, s0, s1, lane, best, bi);
                        }
                    }
                }
            // the wavefront's best so far, in every lane
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const double oD = __shfl_xor(best, m, 64); const int oi = __shfl_xor(bi, m, 64);
                if (oD < best || (oD == best && oi < bi)) { best = oD; bi = oi; }
            }
            // a lower bound of the distance to anything in a cell not yet visited: the nearest wall of the block of visited cells that has cells
            // behind it, 1e-6 on the conservative side (a cell's index is monotone in the coordinate; rounding moves a wall by far less)
            double lb = INFINITY;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int lo_i = cq[k] - r, hi_i = cq[k] + r;
                if (lo_i > 0) lb = fmin(lb, p[k] - (g.lo[k] + (double)lo_i * g.h));
                if (hi_i < g.n[k] - 1) lb = fmin(lb, (g.lo[k] + (double)(hi_i + 1) * g.h) - p[k]);
            }
            if (!(lb < INFINITY)) break;      // every cell has been visited
            lb = lb * (1.0 - 1e-6) - margin;
            if (lb > a.max_dist || (lb > 0.0 && lb * lb * (1.0 - 1e-6) > best)) break;
        }
    }
    const double d = sqrt(best);
    const bool matched = valid && bi != INT_MAX && d <= a.max_dist;
    int side = 0;
    if (matched && a.t_faces) {      // (wave-uniform) the winner once more, for the side of its plane p lies on
        double A[3], B[3], C[3], q[3];
        cmp_target(a, bi, A, B, C);
        cmp_pair(p, A, B, C, q);
        const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, pq[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double s = cmp_dot(pq, n);
        side = s > 0.0 ? 1 : s < 0.0 ? -1 : 0;
    }
    if (lane == 0) {
        const double dd = !valid ? (double)NAN : matched ? d : (double)INFINITY;
        a.d[qi] = dd; a.dist[qi] = (float)dd; a.nearest[qi] = matched ? bi : -1; a.side[qi] = (signed char)side;
        a.pairs[qi] = (int)min(pairs, (long long)INT_MAX);
    }
}

__global__ void __launch_bounds__(kBlock) k_cmp_stats(CompareArgs a) {
    const int lane = threadIdx.x & 63;
    long long v[6] = {0, 0, 0, 0, 0, 0}, pairs = 0;
    unsigned long long mx = 0;
    int hist[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) hist[b] = 0;
    // a lane adds up its queries (a grid-stride loop over at most kCompareStatBlocks workgroups), then the wavefront, then one atomic per field
    for (long long qi = blockIdx.x * (long long)kBlock + threadIdx.x; qi < a.nq; qi += (long long)gridDim.x * kBlock) {
        const double d = a.d[qi];
        const bool valid = !(d != d), matched = valid && d < INFINITY;
        v[CS_VALID] += valid; v[CS_MATCHED] += matched;
        pairs += a.pairs[qi];
        if (matched) {
            const double u = d / a.vs;
            const long long f = llrint(u * 1048576.0);
            v[CS_TAU] += d <= a.tau; v[CS_SUM_D] += f; v[CS_SUM_D2] += llrint(u * u * 1048576.0); v[CS_SIGNED] += (long long)a.side[qi] * f;
            const int bin = min(15, (int)(16.0 * d / a.max_dist));
#pragma unroll
            for (int b = 0; b < 16; ++b) hist[b] += bin == b;      // (no runtime-indexed register array)
            const unsigned long long bitsd = (unsigned long long)__double_as_longlong(d);
            mx = bitsd > mx ? bitsd : mx;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum_ll(v[k]);
    pairs = wave_sum_ll(pairs);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx; }
#pragma unroll
    for (int b = 0; b < 16; ++b) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hist[b] += __shfl_xor(hist[b], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) if (v[k]) atomicAdd(a.stats + k, (unsigned long long)v[k]);
        if (mx) atomicMax(a.stats + CS_MAX, mx);
        if (pairs) atomicAdd(a.stats + CS_PAIRS, (unsigned long long)pairs);
#pragma unroll
        for (int b = 0; b < 16; ++b) if (hist[b]) atomicAdd(a.stats + CS_HIST + b, (unsigned long long)hist[b]);
    }
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_compare_total(const CompareArgs& a, hipStream_t s) {
    if (a.nt > 0) hipLaunchKernelGGL(k_cmp_total, dim3(blocks_of(a.nt)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compare_count(const CompareArgs& a, hipStream_t s) {
    if (a.nt > 0) hipLaunchKernelGGL(k_cmp_cells<false>, dim3(blocks_of(a.nt)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_compare_fill(const CompareArgs& a, hipStream_t s) {
    if (a.nt > 0) hipLaunchKernelGGL(k_cmp_cells<true>, dim3(blocks_of(a.nt)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// A dispatch counts its work-items in 32 bits and 64 lanes per query pass that at 2^26 queries: the queries go out in launches of at most
// `chunk` (PSGSDF_COMPARE_CHUNK; no wavefront straddles two launches, a wavefront is one query).
hipError_t launch_compare_query(CompareArgs a, long long chunk, hipStream_t s) {
    chunk = std::min(std::max(chunk, 1ll), kCompareChunk);
    for (a.q0 = 0; a.q0 < a.nq; a.q0 += chunk) {
        a.q1 = std::min(a.nq, a.q0 + chunk);
        const unsigned blocks = (unsigned)((a.q1 - a.q0 + kBlock / 64 - 1) / (kBlock / 64));
        hipLaunchKernelGGL(k_cmp_query, dim3(blocks), dim3(kBlock), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}
hipError_t launch_compare_stats(const CompareArgs& a, hipStream_t s) {
    if (a.nq > 0) hipLaunchKernelGGL(k_cmp_stats, dim3(std::min(blocks_of(a.nq), (unsigned)kCompareStatBlocks)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace psg
