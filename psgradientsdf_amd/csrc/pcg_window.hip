// pcg_window.hip -- the windowed instances of the persistent distance solve (pcg_solve.h k_cgp_solve<R, false, WIN = true>): their static window
// table, whether a band's windows fit next to the coefficients, and their launch.  A translation unit of its own: pcg.hip holds the gathering instances.
#include "pcg_solve.h"

namespace psg {

// ---- the windowed instance (k_cgp_solve<R, false, true>): its static table and whether a band's windows fit
// Per workgroup of the partition (G x rows_per_wg contiguous rows) and per segment s = z - 1, in-plane, z + 1: tab[6 lb + 2 s] = the first band row,
// tab[6 lb + 2 s + 1] = the length of the range that covers every row the workgroup's rows reference through their packed column deltas, clipped to the
// band; the in-plane range always contains the own rows, an absent column (delta 0) widens nothing.  *max_total = the largest sum of the three lengths.
// Integer min / max only: wave reductions, LDS, one atomicMax per workgroup.
__global__ void __launch_bounds__(kSolveThreads) k_solve_windows(Band b, int row0, int row1, int rows_per_wg, int* __restrict__ tab, int* __restrict__ max_total) {
    __shared__ int red[6][kSolveThreads / 64];
    const int lb = blockIdx.x, tid = threadIdx.x;
    const int first = row0 + lb * rows_per_wg, last = min(row1, first + rows_per_wg) - 1;
    int lo[3] = {INT_MAX, first <= last ? first : INT_MAX, INT_MAX}, hi[3] = {INT_MIN, first <= last ? last : INT_MIN, INT_MIN};
    for (int i = first + tid; i <= last; i += kSolveThreads) {
#pragma unroll
        for (int jj = 0; jj < kNQ - 1; ++jj) {
            const int pk = (int)b.colp[(size_t)(jj >> 1) * b.Spad + i];
            const int d = (jj & 1) ? (pk >> 16) : ((pk << 16) >> 16);
            if (d != 0) { lo[solve_col_seg(jj)] = min(lo[solve_col_seg(jj)], i + d); hi[solve_col_seg(jj)] = max(hi[solve_col_seg(jj)], i + d); }
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[s] = min(lo[s], __shfl_xor(lo[s], o, 64)); hi[s] = max(hi[s], __shfl_xor(hi[s], o, 64)); }
        if ((tid & 63) == 0) { red[2 * s][tid >> 6] = lo[s]; red[2 * s + 1][tid >> 6] = hi[s]; }
    }
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int s = 0; s < 3; ++s) {
            int l = INT_MAX, h = INT_MIN;
            for (int i = 0; i < kSolveThreads / 64; ++i) { l = min(l, red[2 * s][i]); h = max(h, red[2 * s + 1][i]); }
            l = max(l, 0); h = min(h, b.S - 1);
            const int len = h >= l ? h - l + 1 : 0;
            tab[6 * lb + 2 * s] = len ? l : 0; tab[6 * lb + 2 * s + 1] = len;
            total += len;
        }
        atomicMax(max_total, total);
    }
}
void launch_solve_windows(const Band& b, int row0, int row1, int G, int rows_per_wg, int* tab, int* max_total, hipStream_t s) {
    hipMemsetAsync(max_total, 0, sizeof(int), s);
    hipLaunchKernelGGL(k_solve_windows, dim3(G), dim3(kSolveThreads), 0, s, b, row0, row1, rows_per_wg, tab, max_total);
}
// Dynamic LDS of the windowed instance for windows of `doubles` values (0: they do not fit next to the coefficients and the kernel's static buffers,
// they exceed the kWinLoads x 512 values one pass fetches, or the instance cannot be resident at that size).  Asked for and checked with the real size.
constexpr size_t kSolveLdsBytes = 160 * 1024;      // LDS of one CU (gfx950)
static int solve_window_capacity(int rows) {      // doubles a window may hold at this row count
    return solve_with_rows(rows, [](auto rc) {
        constexpr int R = decltype(rc)::value;
        if constexpr (R >= kCgpMaxRows) return 0;      // (four rows of coefficients leave 8 KB: less than the workgroup's own rows -- no windowed instance)
        else {
        static const int cap = [] {
            hipFuncAttributes fa{};
            if (hipFuncGetAttributes(&fa, (const void*)k_cgp_solve<R, false, true>) != hipSuccess || fa.sharedSizeBytes + solve_lds(R) >= kSolveLdsBytes) return 0;
            return (int)std::min<size_t>((kSolveLdsBytes - fa.sharedSizeBytes - solve_lds(R)) / sizeof(double), (size_t)kWinLoads * kSolveThreads);
        }();
        return cap;
        }
    });
}
static size_t solve_window_lds(int rows, int doubles) {
    if (doubles <= 0 || doubles > solve_window_capacity(rows)) return 0;
    return solve_with_rows(rows, [&](auto rc) -> size_t {
        constexpr int R = decltype(rc)::value;
        if constexpr (R >= kCgpMaxRows) return 0;
        else {
        static size_t prepared = 0; static int resident = 0;      // the last size this instance was prepared for
        const size_t lds = solve_lds(R) + sizeof(double) * (size_t)doubles;
        if (lds != prepared) { resident = solve_prepare(k_cgp_solve<R, false, true>, lds); prepared = lds; }
        return resident >= 1 ? lds : 0;
        }
    });
}
int cgf_solve_window_budget(int rows_per_wg) { return solve_window_capacity((rows_per_wg + kSolveThreads - 1) / kSolveThreads); }
bool launch_cgp_solve_window(const SweepArgs& a, double* fs, double* gran, int G, int rows_per_wg, int kmax, double* mb, unsigned long long mb_key, int force_passes, hipStream_t s) {
    const int rows = (rows_per_wg + kSolveThreads - 1) / kSolveThreads;
    const size_t lds = solve_window_lds(rows, a.pcg_win_max);      // (asks for, and checks residency with, the real size)
    if (!lds) return false;
    solve_with_rows(rows, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if constexpr (R < kCgpMaxRows) hipLaunchKernelGGL((k_cgp_solve<R, false, true>), dim3(G), dim3(kSolveThreads), lds, s, a, fs, gran, rows_per_wg, kmax, mb, mb_key, force_passes, XrArgs{});
    });
    return true;
}

}  // namespace psg
