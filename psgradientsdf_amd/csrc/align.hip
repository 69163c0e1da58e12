// align.hip -- the device side of the registration of a reference to the welded mesh (include/psgsdf_align.h).  One evaluation at a
// transform T is: the points moved (k_aln_move), compare.hip's search on the moved points (k_cmp_query, unchanged), the point-to-plane rows of the
// winners reduced to one 6x6 system (k_aln_rows, k_aln_fold).
//   k_aln_move   one lane per point: (float)(((r0 x + r1 y) + r2 z) + t) per row of the 3x4 transform, in double; NaN stays NaN.
//   k_aln_rows<DIR>   one lane per query in a grid-stride loop over align_row_blocks(nq) <= 128 workgroups.  A lane evaluates its winner's pair once
//            more for the closest point q (the search keeps only the index), forms the row J, rho and adds J J^T (21), J rho (6), rho^2 and 1 to 29
//            double accumulators of its own, all indexed at compile time (registers).  Then a fixed __shfl_xor butterfly (offsets 32 .. 1: every lane
//            ends with the wavefront's sum), lane 0 of each wavefront to LDS, and lanes 0 .. 29 add the four wavefronts in their order and write the
//            workgroup's partial row with plain stores.  Which queries a lane sees, and so the order of every sum, depends on nq only.
//   k_aln_fold   one wavefront: lane k adds column k of the partial rows in workgroup order, direction 1 then direction 2.
// No atomics.  Contraction off, IEEE / and sqrt, as in compare.hip: every term is the bits tests/_align_ref.py computes.
#pragma clang fp contract(off)
#include "compare_device.h"
#include "align.h"

namespace psg {
namespace {

__global__ void __launch_bounds__(kBlock) k_aln_move(AlignMoveArgs a) {
    const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
    if (i >= a.n) return;
    const double x = (double)a.src[3 * i], y = (double)a.src[3 * i + 1], z = (double)a.src[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.dst[3 * i + k] = (float)(((a.M[4 * k] * x + a.M[4 * k + 1] * y) + a.M[4 * k + 2] * z) + a.M[4 * k + 3]);
}

template <int DIR>
__global__ void __launch_bounds__(kBlock) k_aln_rows(AlignRowArgs a) {
    __shared__ double red[kBlock / 64][kAlignRow];
    double acc[kAlignRow - 1];
#pragma unroll
    for (int k = 0; k < kAlignRow - 1; ++k) acc[k] = 0.0;
    long long pairs = 0;
    for (long long qi = blockIdx.x * (long long)kBlock + threadIdx.x; qi < a.s.nq; qi += (long long)gridDim.x * kBlock) {
        pairs += a.s.pairs[qi];
        const int t = a.s.nearest[qi];
        if (t < 0) continue;
        double p[3], A[3], B[3], C[3], q[3], x[3], n[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (double)a.s.q_xyz[3 * qi + k];
        cmp_target(a.s, t, A, B, C);
        cmp_pair(p, A, B, C, q);
        if (DIR == 1) {      // the moved reference point against the plane of the winning face
            const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
            n[0] = ab[1] * ac[2] - ab[2] * ac[1]; n[1] = ab[2] * ac[0] - ab[0] * ac[2]; n[2] = ab[0] * ac[1] - ab[1] * ac[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) { x[k] = p[k]; d[k] = p[k] - q[k]; }
        } else {             // the closest reference point, moved in double, against the plane of the vertex it was found from
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[k] = ((a.T[4 * k] * q[0] + a.T[4 * k + 1] * q[1]) + a.T[4 * k + 2] * q[2]) + a.T[4 * k + 3];
                n[k] = (double)a.v_nrm[3 * qi + k];
                d[k] = x[k] - (double)a.v_xyz[3 * qi + k];
            }
        }
        const double len = sqrt(cmp_dot(n, n));
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
        if (!(isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]))) continue;
        const double r = cmp_dot(n, d), rho = r / a.vs;
        const double y[3] = {(x[0] - a.c[0]) / a.vs, (x[1] - a.c[1]) / a.vs, (x[2] - a.c[2]) / a.vs};
        const double J[6] = {y[1] * n[2] - y[2] * n[1], y[2] * n[0] - y[0] * n[2], y[0] * n[1] - y[1] * n[0], n[0], n[1], n[2]};
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[AL_G + i] += J[i] * rho;
        acc[AL_E] += rho * rho;
        acc[AL_N] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < kAlignRow - 1; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pairs += __shfl_xor(pairs, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kAlignRow - 1; ++k) red[w][k] = acc[k];
        red[w][AL_PAIRS] = (double)pairs;      // (below 2^53: exact)
    }
    __syncthreads();
    if (threadIdx.x < kAlignRow) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < kBlock / 64; ++v) s += red[v][threadIdx.x];
        a.partial[(long long)blockIdx.x * kAlignRow + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(64) k_aln_fold(const double* p1, int nb1, const double* p2, int nb2, double* sys) {
    const int k = threadIdx.x;
    if (k >= kAlignSys) return;
    // columns 0 .. 27 over both directions; then the rows and the candidate pairs of each direction
    const int col = k < AS_N ? k : k < AS_PAIRS ? AL_N : AL_PAIRS;
    const bool d1 = k < AS_N || k == AS_N || k == AS_PAIRS, d2 = k < AS_N || k == AS_N + 1 || k == AS_PAIRS + 1;
    double s = 0.0;
    if (d1) for (int b = 0; b < nb1; ++b) s += p1[(long long)b * kAlignRow + col];
    if (d2) for (int b = 0; b < nb2; ++b) s += p2[(long long)b * kAlignRow + col];
    sys[k] = s;
}

}  // namespace

hipError_t launch_align_move(const AlignMoveArgs& a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(k_aln_move, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_align_rows(const AlignRowArgs& a, int dir, hipStream_t s) {
    if (a.s.nq > 0) {
        if (dir == 1) hipLaunchKernelGGL(k_aln_rows<1>, dim3(align_row_blocks(a.s.nq)), dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL(k_aln_rows<2>, dim3(align_row_blocks(a.s.nq)), dim3(kBlock), 0, s, a);
    }
    return hipGetLastError();
}
hipError_t launch_align_fold(const double* p1, int nb1, const double* p2, int nb2, double* sys, hipStream_t s) {
    hipLaunchKernelGGL(k_aln_fold, dim3(1), dim3(64), 0, s, p1, nb1, p2, nb2, sys);
    return hipGetLastError();
}

}  // namespace psg
