// pcg_solve.h -- the persistent distance solve as templates: the workgroup's place in the band, the bounded waits of the hand-off protocol, the
// assembly of a thread's rows, the epilogue, the pipelined kernel k_cgp_solve itself, and the host-side row-count dispatch.
// Instantiated by pcg.hip (the gathering instances) and by pcg_window.hip (the windowed instances).
#pragma once
#include "device_common.h"

namespace psg {

__device__ __forceinline__ float pcg_threshold(float rhsNorm2) { return fmaxf(FLT_EPSILON * FLT_EPSILON * rhsNorm2, FLT_MIN); }

// ------------------------------------------------------------------------------------------
// The whole solve as ONE persistent kernel (contexts whose band fits the register file and the LDS).
//
// A per-pass launch re-streams the 19 ELL coefficients and 9 index words of every row (152 B/row, 51 MB at the 256^3 band:
// 9.7 of the pass's 14.3 us at the ~5.3 TB/s the L2-miss path sustains; profiles/r01_notes.md) although the matrix never
// changes during a solve.  Here every thread assembles the coefficients of its R rows ONCE into LDS (five 16-byte words per row: SolveCoefs), keeps the column deltas
// (9 packed words per row) and the row's own vectors in registers, and loops over the passes; per pass it obtains the 18
// neighbour values of each row (L2-resident), updates its rows and meets the other workgroups at a device-wide all-gather of
// the per-workgroup sums (k_cgp_solve below says which values and which sums):
//   publish : a row's value is ONE double that carries its own tag (m_tag below), stored at agent scope; the sums are 8-byte granules
//             {sum with a 2-bit pass tag in its two lowest mantissa bits}, one store each: data and tag arrive together, no flag, no
//             ordering between them, no drain of the stores in front of them.  (Measured on the way here: plain stores + an agent-scope
//             release fence cost 4.8 us for drain + write-back per pass, profiles/r02_notes.md; write-through stores, a drain, and a wait
//             for the band neighbours' tags with an acquire behind it cost 1 us per pass more than this, profiles/r05_notes.md.  Both are
//             gone: a value that is not the pass's yet is simply asked for again.)
//   wait    : thread t polls the granules of workgroup t until their tags name the pass, and the fixed-order sum over workgroups that
//             every workgroup computes identically gives alpha, beta, |r|^2 and the stop decision -- the same everywhere, so all
//             workgroups leave in the same pass.  The values double-buffer exactly as k_cgf_pass's records do: a workgroup writes its
//             pass-k values only after it has seen EVERY workgroup's pass k-1 sums, i.e. after every reader of the old ones is done.
// One workgroup of 512 threads per CU at most (grid <= the CU count, so all workgroups are co-resident); logical workgroup ids
// are remapped so that every XCD owns a contiguous range of rows (gathers stay in that XCD's L2).  Every wait is bounded:
// a workgroup that sees nothing for ~1 s raises the abort flag and every workgroup leaves (the host reports PSGSDF_ERR_DEVICE).
// Two mantissa bits of the double sums carry the tag: 4e-16 relative, far below the float the sums are rounded to.
// ------------------------------------------------------------------------------------------
constexpr int kSolveThreads = 512;            // one workgroup of 8 waves per CU: 2 waves per SIMD at <= 256 VGPRs (16 waves at 128 VGPRs spilled: 21 us per pass)
constexpr int kSolveMaxBlocks = 256;          // one per CU
constexpr int kSolveMaxRows = 4;              // rows per thread: R x 40 KB of coefficients in the CU's 160 KB of LDS (four rows: 152 KB, SolveCoefs below)
typedef float v4f_t __attribute__((ext_vector_type(4)));
// THE COEFFICIENTS OF A ROW SLOT IN LDS (round 10): the 19 floats of a thread's row are FIVE 16-byte words (q = 4 g + c is component c of word g; the
// twentieth float is an exact 0 that no sum reads), word g of row slot u in a plane of its own: hs4[(u * 5 + g) * kSolveThreads + tid].  A row is
// fetched with five ds_read_b128 -- lanes read consecutive 16-byte words: no bank conflict -- instead of nineteen ds_read_b32: 60 instead of 114
// LDS-array cycles per wave and pass at R = 3, and ds_read_b128 reaches its rate at the solve's two waves per SIMD where ds_read_b32 needs about four.
// The layout belongs to the thread (it writes its words once per solve and nobody else reads them); the readers multiply in the column order they
// always had.  Four row slots of five words would be the CU's whole 160 KB: at R = 4 (no windowed instance, not tuned) only the four full words of a
// slot are planes of words, hs4[(u * 4 + g) * kSolveThreads + tid], and the three floats of the fifth stay planes of floats behind them.
constexpr int kCoefWords = (kNQ + 3) / 4;
static_assert(kNQ == 19 && kCoefWords == 5, "a row's coefficients are five 16-byte words, the last one padded with one zero");
template <int R> struct SolveCoefs {
    static constexpr int kPlanes = R < kSolveMaxRows ? kCoefWords : kCoefWords - 1;      // planes of 16-byte words per row slot
    static constexpr int kTail = kNQ - 4 * (kCoefWords - 1);                              // R = 4: floats of the fifth word, in planes of floats
    static constexpr size_t kBytes = sizeof(v4f_t) * R * kPlanes * kSolveThreads + (kPlanes < kCoefWords ? sizeof(float) * R * kTail * kSolveThreads : 0);
    static __device__ __forceinline__ v4f_t* words(int u, int tid) { return reinterpret_cast<v4f_t*>(psg_dyn_smem) + (size_t)u * kPlanes * kSolveThreads + tid; }
    static __device__ __forceinline__ float* tail(int u, int tid) { return reinterpret_cast<float*>(reinterpret_cast<v4f_t*>(psg_dyn_smem) + (size_t)R * kPlanes * kSolveThreads) + (size_t)u * kTail * kSolveThreads + tid; }
    static __device__ __forceinline__ void store(int u, int tid, const float (&hv)[4 * kCoefWords]) {
        v4f_t* w = words(u, tid);
#pragma unroll
        for (int g = 0; g < kPlanes; ++g) { v4f_t t; t[0] = hv[4 * g]; t[1] = hv[4 * g + 1]; t[2] = hv[4 * g + 2]; t[3] = hv[4 * g + 3]; w[g * kSolveThreads] = t; }
        if constexpr (kPlanes < kCoefWords) {
#pragma unroll
            for (int c = 0; c < kTail; ++c) tail(u, tid)[c * kSolveThreads] = hv[4 * kPlanes + c];
        }
    }
    // words [G0, G1) of row slot u into hc
    template <int G0, int G1> static __device__ __forceinline__ void load(int u, int tid, v4f_t (&hc)[kCoefWords]) {
        const v4f_t* w = words(u, tid);
#pragma unroll
        for (int g = G0; g < G1; ++g) {
            if (g < kPlanes) hc[g] = w[g * kSolveThreads];
            else {
                v4f_t t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < kTail; ++c) t[c] = tail(u, tid)[c * kSolveThreads];
                hc[g] = t;
            }
        }
    }
};
__device__ __forceinline__ float solve_coef(const v4f_t (&hc)[kCoefWords], int q) { return hc[q >> 2][q & 3]; }
__device__ __forceinline__ double gran_tag(double v, unsigned tag) { return __longlong_as_double((long long)(((unsigned long long)__double_as_longlong(v) & ~3ull) | tag)); }
__device__ __forceinline__ unsigned gran_tag_of(double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) & 3ull); }
// cross-rank words (multi-rank solve): the tag is 16 bits wide, (epoch of the solve << 2 | pass tag) -- 2^-36 of the value, still far below the float the
// sums are rounded to.  No word of an earlier solve can match, so the regions are never cleared between solves (engine.h XrArgs).
__device__ __forceinline__ double xr_tag(double v, unsigned tag) { return __longlong_as_double((long long)(((unsigned long long)__double_as_longlong(v) & ~0xffffull) | tag)); }
__device__ __forceinline__ unsigned xr_tag_of(double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) & 0xffffull); }

// One ELL row of the distance system accumulated in REGISTERS: the contributions of assemble_row (dist.hip), in its order.  There the column
// of a contribution is a run-time index into an LDS table; here every (contributor, block column) pair has at most two possible
// columns, known at compile time, and the one the contributor's stencil direction does not select receives an exact + 0.0 -- the
// nineteen sums are bit-identical to the LDS version's.
__device__ __forceinline__ bool ell_valid(const int* o) {
    const int nz = (o[0] != 0) + (o[1] != 0) + (o[2] != 0);
    return nz <= 2 && o[0] >= -1 && o[0] <= 1 && o[1] >= -1 && o[1] <= 1 && o[2] >= -1 && o[2] <= 1;
}
__device__ __forceinline__ void assemble_row_regs(const SweepArgs& a, int i, double (&acc)[kNQ], double& rhs) {
    const Band& b = a.b;
    int jr[7]; jr[0] = i;
#pragma unroll
    for (int c = 1; c < 7; ++c) { const int ax = (c - 1) >> 1; const bool upper = (c - 1) & 1; jr[c] = b.nb[(size_t)(2 * ax + (upper ? 0 : 1)) * b.Spad + i]; }
    int db[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) db[c] = b.dirb[jr[c] >= 0 ? jr[c] : i];
    bool use[7]; use[0] = true;
#pragma unroll
    for (int c = 1; c < 7; ++c) { const int ax = (c - 1) >> 1; const bool upper = (c - 1) & 1; use[c] = jr[c] >= 0 && !(upper && ((db[c] >> ax) & 1)); }
    float val[7][4], gr[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const int sl = c == 0 ? 0 : ((c - 1) >> 1) + 1;
        const int jrow = use[c] ? jr[c] : i;
        gr[c] = b.blk[(size_t)(10 + sl) * b.Spad + jrow];
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) val[c][bq] = b.blk[(size_t)sym4(sl, bq) * b.Spad + jrow];
    }
#pragma unroll
    for (int q = 0; q < kNQ; ++q) acc[q] = 0.0;
    rhs = 0.0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const int ax = c == 0 ? 0 : (c - 1) >> 1; const bool upper = c > 0 && ((c - 1) & 1);
        int coff[3] = {0, 0, 0};
        if (c > 0) coff[ax] = upper ? 1 : -1;
        rhs += use[c] ? (double)gr[c] : 0.0;
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) {
            const double v = use[c] ? (double)val[c][bq] : 0.0;
            if (bq == 0) { acc[q_of(coff)] += v; continue; }
            const bool fwd = (db[c] >> (bq - 1)) & 1;
            int oP[3] = {coff[0], coff[1], coff[2]}, oM[3] = {coff[0], coff[1], coff[2]};
            oP[bq - 1] += 1; oM[bq - 1] -= 1;
            if (ell_valid(oP)) acc[q_of(oP)] += fwd ? v : 0.0;
            if (ell_valid(oM)) acc[q_of(oM)] += fwd ? 0.0 : v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The parts of k_cgp_solve that do not depend on its recurrences: the workgroup's place in the band and in the slab, the exchange of the ranks' sums
//  with its bounded waits and the abort path, the assembly of a thread's rows, the distance update of the epilogue and the
// outcome the host reads.
// ------------------------------------------------------------------------------------------
constexpr int kXrSpins = 1 << 24;            // bound of every wait for another RANK (~1 s)
// stage timestamps of pass 8 (timing hook only: force_passes > 0), wall clock at 100 MHz, written by thread 0 of two workgroups
#define SOLVE_STAMP(j) do { if (force_passes > 0 && k == 8 && tid == 0 && (lb == 0 || lb == (G * 9) / 16)) mb[8 + (lb ? 8 : 0) + (j)] = (double)wall_clock64(); } while (0)

template <bool MR> struct SolveWg {
    static constexpr int kLocalSpins = MR ? kXrSpins : (1 << 22);      // MR: a local neighbour may itself be waiting for a late RANK -- the local waits must not expire first
    const SweepArgs& a; const XrArgs& xr; double* const fs; double* const gran; const int rows_per_wg;
    const int G = gridDim.x, tid = threadIdx.x;
    // The XCD this workgroup REALLY runs on (HW_REG_XCC_ID): what the prologue's flag and the timing hook report
    const int my_xcc = (int)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));
    // XCD-aware placement: workgroups are dealt round-robin to the 8 XCDs; logical block lb gives XCD x the contiguous blocks [x G/8, (x+1) G/8)
    const int lb = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    const int own_n = a.row1 - a.row0;
    double* const xr_me = MR ? xr.region[xr.rank] : nullptr;
    const unsigned etag0 = MR ? (xr.epoch & kXrEpochMask) << 2 : 0u;      // cross-rank tags: (epoch << 2 | pass tag)

    __device__ __forceinline__ SolveWg(const SweepArgs& a_, const XrArgs& xr_, double* fs_, double* gran_, int rows_per_wg_) : a(a_), xr(xr_), fs(fs_), gran(gran_), rows_per_wg(rows_per_wg_) {}

    // row slot u of this thread.  The band is dealt evenly to ALL workgroups (rows_per_wg each, a multiple of 64): the last row slot of a thread is only
    // partly used; a slot without a row works on the last own row and stores nothing
    __device__ __forceinline__ int own_row(int u, bool& live) const {
        const int i = a.row0 + lb * rows_per_wg + u * kSolveThreads + tid;
        live = u * kSolveThreads + tid < rows_per_wg && i < a.row1;
        return live ? i : a.row1 - 1;
    }
    __device__ __forceinline__ double* gran_plane(int buf, int q) const { return gran + ((size_t)buf * kSolveGranPlanes + q) * kSolveMaxBlocks; }
    // 'a wait gave up': here and in every rank's region, so that every workgroup of every rank leaves
    __device__ __forceinline__ void raise_abort() const {
        __hip_atomic_store(fs + 3, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (MR) for (int r = 0; r < xr.n_ranks; ++r) __hip_atomic_store(xr.region[r] + kXrAbort, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __device__ __forceinline__ bool aborted() const { return __hip_atomic_load(fs + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0.0; }
    __device__ __forceinline__ bool aborted_by_rank() const { return aborted() || __hip_atomic_load(xr_me + kXrAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0.0; }
    // Prologue (thread 0, behind the barrier that follows the drain of the workgroup's first stores): 1 + the XCD id into plane 7 of buffer 1.
    // Nothing waits for this flag or reads it.  It stays because the gathering instances measured 0.3-0.4 us per pass slower without it (7.2 against 6.8 us
    // at the 256^3 band; the windowed instances do not care): the store lies outside the pass loop, what changes is the code the compiler makes of the
    // loop (profiles/r09_notes.md section 5)
    __device__ __forceinline__ void publish_prologue() const {
        __hip_atomic_store(gran_plane(1, 7) + lb, (double)(1 + my_xcc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Stage C2 (MR): t[0..n) are this RANK's sums (every local workgroup holds the same bits).  Workgroup 0 hands them to every rank as tagged granules of
    // buffer pb; every workgroup then adds the granules of its own region in rank order (one fixed tree: the same bits on every rank) -- all <= 32 of them
    // sit in wavefront 0.  false = a wait gave up.  The caller's next barrier protects `red`.
    template <int N> __device__ __forceinline__ bool exchange_rank_sums(double (&t)[N], int n, int pb, unsigned want, double* red /*[8 * kSolveThreads / 64]*/, int* abort_word) const {
        static_assert(N <= 8, "eight granule planes per buffer");
        if (lb == 0 && tid < n) {
            const double mine = xr_tag(t[tid], etag0 | want);
            for (int r = 0; r < xr.n_ranks; ++r) __hip_atomic_store(xr.region[r] + kXrRankGran + (pb * 8 + tid) * kXrMaxRanks + xr.rank, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        double rv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) rv[q] = 0.0;
        if (tid < xr.n_ranks) {
            int spins = 0; bool ok = false;
            while (!ok) {
                ok = true;
#pragma unroll
                for (int q = 0; q < N; ++q) if (q < n) { rv[q] = __hip_atomic_load(xr_me + kXrRankGran + (pb * 8 + q) * kXrMaxRanks + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); ok = ok && xr_tag_of(rv[q]) == (etag0 | want); }
                if (!ok) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kXrSpins || aborted_by_rank()) { *abort_word = 1; break; }
                }
            }
        }
        double r0, r1; wave_sum8(rv, r0, r1);
        wave_sum8_store<kSolveThreads / 64>(r0, r1, red, tid >> 6);
        __syncthreads();
        if (*abort_word) { if (tid == 0) raise_abort(); return false; }
#pragma unroll
        for (int q = 0; q < N; ++q) if (q < n) t[q] = red[q * (kSolveThreads / 64)];
        return true;
    }
};

// One row of a thread, assembled straight from the voxel blocks of the distance sweep (no k_assemble, no H in memory): the 19 coefficients (the diagonal
// damped) into the words of the thread's row slot u (SolveCoefs), the Jacobi weight and the right-hand side returned
template <int R> __device__ __forceinline__ void solve_assemble_row(const SweepArgs& a, int row, int u, int tid, float& inv, double& rhs) {
    double acc[kNQ];
    assemble_row_regs(a, row, acc, rhs);
    float hv[4 * kCoefWords];
#pragma unroll
    for (int q = 0; q < 4 * kCoefWords; ++q) hv[q] = q < kNQ ? (float)acc[q] : 0.f;
    if (a.damping != 0.0f) hv[0] += a.damping * hv[0];
    SolveCoefs<R>::store(u, tid, hv);
    float dg = (float)acc[0];
    if (a.damping != 0.0f) dg += a.damping * dg;
    inv = dg != 0.f ? 1.0f / dg : 1.0f;
}
// the 9 packed column words of a row (two 16-bit deltas each), kept in registers for the whole solve
__device__ __forceinline__ void solve_load_columns(const Band& b, int row, unsigned (&cp)[(kNQ - 1) / 2]) {
    const int plane = b.Spad * 4;
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)b.colp, 0, (kNQ - 1) / 2 * plane, 0x00020000);
#pragma unroll
    for (int wd = 0; wd < (kNQ - 1) / 2; ++wd) cp[wd] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rC, row * 4, wd * plane, 0);
}
// (the packed column deltas are loop-invariant: given the chance, the compiler precomputes all 18 R gather addresses as 64-bit pairs
// ahead of the loop and spills them -- an empty asm per word, once per pass, keeps the three-instruction address arithmetic inside the pass)
template <int R> __device__ __forceinline__ void solve_keep_columns_packed(unsigned (&cp)[R][(kNQ - 1) / 2]) {
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int wd = 0; wd < (kNQ - 1) / 2; ++wd) asm volatile("" : "+v"(cp[u][wd]));
}
// Eigen's info() == Success for a solve that ran to its end, the host's rule (loop.hip: pcg_solve) -- every workgroup holds the same |r|^2 and |b|^2
__device__ __forceinline__ bool solve_converged(int status, float rr_cur, float rhsNorm2) {
    return status == 1 && (rhsNorm2 == 0.f || sqrt((double)rr_cur / (double)rhsNorm2) <= (double)FLT_EPSILON);
}
// Epilogue: x of the own rows and, if asked for, the distance update (k_apply_dist: updateDist's accept rule, OptimizerAux.cpp:162-188) under the rule
// the host applies to the solve's outcome.  The accepted count is a sum of integers: the per-workgroup counts go to the first G entries of the slot,
// the rest of the slot (k_apply_albedo's leftovers) is cleared.
template <bool MR, int R>
__device__ __forceinline__ void solve_apply_and_count(const SolveWg<MR>& wg, const float (&x)[R], const int (&row)[R], const bool (&live)[R], int status, float rr_cur, float rhsNorm2, double* red) {
    const SweepArgs& a = wg.a; const Band& b = a.b;
#pragma unroll
    for (int u = 0; u < R; ++u) if (live[u]) b.x[row[u]] = x[u];
    if (!a.pcg_apply) return;
    const bool apply = status == 1 && (a.pcg_apply == 1 || solve_converged(status, rr_cur, rhsNorm2));
    double cnt = 0;
    if (apply) {
#pragma unroll
        for (int u = 0; u < R; ++u) if (live[u] && (double)fabsf(x[u]) < sqrt(3.0) * (double)a.grid.vs) { b.dist[row[u]] -= x[u]; cnt += 1.0; }
    }
    cnt = wave_sum(cnt);
    __syncthreads();
    if ((wg.tid & 63) == 0) red[wg.tid >> 6] = cnt;
    __syncthreads();
    double* slot = PART(a, SC_ACCEPT);
    if (wg.tid == 0) { double t = 0; for (int i = 0; i < kSolveThreads / 64; ++i) t += red[i]; slot[wg.lb] = t; }
    for (int i = wg.G + wg.lb * kSolveThreads + wg.tid; i < a.acc.PB; i += wg.G * kSolveThreads) slot[i] = 0.0;
}
// The outcome for the host and for the gated kernels behind the solve (ONE thread of the grid).  status 1 = finished, 2 = a wait timed out: a solve
// that gave up leaves BOTH gates closed -- nothing behind it may act on it (the host re-runs the solve, loop.hip)
__device__ __forceinline__ void solve_report(double* fs, double* mb, unsigned long long mb_key, int status, int k, float rr_cur, float rhsNorm2, float thr) {
    int iters = 0;
    if (rhsNorm2 != 0.f && k > 0) iters = (rr_cur < thr) ? k - 1 : k;      // Eigen leaves the loop before ++i when it detects convergence; k == kmax otherwise
    fs[1] = status == 1 ? (double)(k + 1) : 0.0; fs[2] = solve_converged(status, rr_cur, rhsNorm2) ? 1.0 : 0.0;
    const double m0 = (double)iters, m1 = (double)rr_cur, m2 = (double)rhsNorm2, m3 = (double)status;
    mb[0] = m0; mb[1] = m1; mb[2] = m2;
    __threadfence_system();
    mb[3] = m3;                            // the host watches this slot ...
    // ... and takes the four words only together with their check word (engine.h FoldReq)
    if (mb_key) reinterpret_cast<unsigned long long*>(mb)[4] = (unsigned long long)(__double_as_longlong(m0) ^ __double_as_longlong(m1) ^ __double_as_longlong(m2) ^ __double_as_longlong(m3)) ^ mb_key;
    __threadfence_system();
}

// ------------------------------------------------------------------------------------------
// The persistent solve is PIPELINED (round 4): the recurrences of Ghysels & Vanroose's pipelined CG, so that a pass does not
// wait for its own reduction.
//
// With the classic recurrences (k_cgf_pass; round 2's persistent kernel ran them too) the sums of pass k contain t_k = A p_k, i.e. they can only be
// published AFTER the gathers of pass k, and the next pass can only start after they have gone round the device: per pass  tags ~0.9 + gathers ~4.2 +
// sums ~2.7 + finish ~1.1 = 9.5 us (profiles/r02_notes.md), the 2.7 us being a pure wait for the slowest workgroup's publish to arrive.  Here a pass
// publishes, at its END, the next search-direction input
// m_{k+1} = M^-1 w_{k+1} AND the three sums of the NEXT pass -- gamma = r.u, delta = w.u, |r|^2 with u = M^-1 r, w = A u carried by recurrence --
// none of which involves the matrix-vector product n_{k+1} = A m_{k+1} that the next pass gathers for.  The all-gather of the sums therefore runs
// concurrently with the gathers, and is complete when they are:
//     per pass  gathers + finish   (~6 us: profiles/r04_notes.md)
// Recurrences (Jacobi M = diag, so q = M^-1 s and m = M^-1 w need no extra vectors), Eigen's x0 = 0:
//     r_0 = b, u_0 = M^-1 b, w_0 = A u_0 (one extra gather round in front);   pass k:  n = A (M^-1 w)   ||   gamma, delta, |r|^2 over the device
//     beta = gamma / gamma_old (0 in pass 0), alpha = gamma / (delta - beta gamma / alpha_old)
//     z = n + beta z;  s = w + beta s;  p = u + beta p;  x += alpha p;  r -= alpha s;  w -= alpha z;  u = M^-1 r
// In exact arithmetic the iterates ARE Eigen::ConjugateGradient's (alpha equals r.z / p.Ap); in float they differ from it -- and from k_cgf_pass,
// which keeps the round-1 recurrences for bands that do not fit the LDS and as the fallback -- at rounding level (deviation 3;
// measured margins in profiles/r04_parity_margins.json).  Stop rule, iteration count and info() are Eigen's: |r_k|^2 of the recursively updated
// residual against max(eps^2 |b|^2, FLT_MIN), checked before update k + 1.  Gather rounds per solve: iterations + 2 (w_0, and the round that is in
// flight when the stop is detected) instead of iterations + 1.
// What travels: ONE double per row (m) instead of k_cgf_pass's 16-byte record, three tagged sums instead of seven (+ |b|^2 = the |r|^2 of pass 0).
// ------------------------------------------------------------------------------------------
constexpr int kCgpSums = 3;
constexpr int kCgpMaxRows = 4;                // row slots per thread the pipelined kernel supports
#ifndef PSG_CGP_DEPTH
#define PSG_CGP_DEPTH 2
#endif
#ifndef PSG_WIN_BATCH
#define PSG_WIN_BATCH 9                       // windowed instance: window reads of the product in flight per thread, a divisor of 18 (round 10, with the row's five coefficient
#endif                                        // words read up front: 6 and 9 time the same, 5.47 us per pass, at 234 / 241 VGPRs; 18 spills 20 bytes: profiles/r10_notes.md)
static_assert((kNQ - 1) % PSG_WIN_BATCH == 0, "whole batches");
#ifndef PSG_WIN_PREFETCH
#define PSG_WIN_PREFETCH 2                    // windowed instance: the sums are requested 0 = right behind the window's loads, 1 = behind the window's stores, 2 = behind the products of the
#endif                                        // thread's first row (measured, profiles/r07_notes.md: 6.68 / 5.90 / 5.89 us per pass, 2 930 / 3 003 / 3 044 it/s: the earlier, the more often re-polled)
constexpr int kCgpDepth = PSG_CGP_DEPTH;      // gather batches (of 9 doubles) in flight per thread
__device__ __forceinline__ void store8_sys(double* p, double v) { asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory"); }

// SELF-VALIDATING m (round 5; between ranks too).  Every exchanged value carries (solve epoch << 2 | pass tag) in its four lowest mantissa bits
// (2^-48 of a double that multiplies float coefficients), is stored write-through and gathered with agent-scope loads that are re-issued until the tag is
// the pass's: no neighbour-tag wait, no acquire, no drain of the stores in front of the sums -- the hand-off of a pass is ONE trip through memory
// (round 4's ordered hand-off -- store, drain, tag, poll, acquire, gather: three trips -- measured 7.9 us per pass against 6.9-7.0, profiles/r05_notes.md).
__device__ __forceinline__ double m_tag(double v, unsigned tag) { return __longlong_as_double((long long)(((unsigned long long)__double_as_longlong(v) & ~15ull) | tag)); }
__device__ __forceinline__ unsigned m_tag_of(double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) & 15ull); }

// WIN (single rank; PSGSDF_PCG_WINDOW): the neighbour values of a pass come from an LDS WINDOW instead of 18 scattered gathers per row.  The rows of a
// workgroup reference about three times its own row count in distinct band rows, in three contiguous ranges -- the z - 1 columns, the in-plane columns
// (the own rows and their xy halo) and the z + 1 columns; which range a column belongs to is a compile-time property of its index (solve_col_seg).  The
// static table a.pcg_win (k_solve_windows: once per band and partition) holds {first band row, length} of the three ranges of every workgroup; they lie
// back to back in the dynamic LDS behind the coefficients.  Stage B is then: B1 every FOREIGN slot (everything that is not an own row) is fetched once,
// coalesced, with the same self-validating loads as the gathers -- all of a thread's loads issued before the first check, ONE trip past the L2 instead
// of three -- and written into the window; the own rows never travel: stage D (and the prologue) writes the tagged value it publishes into the own
// range as well; one barrier; B2 the products read the window, columns in the order of the gathers, the same multiply-adds: the same bits.  Per row: its
// five coefficient words, then the 18 window values in batches of PSG_WIN_BATCH reads issued back to back with a scheduling barrier between a batch's reads
// and its multiply-adds -- without it the compiler waits for every single read before it issues the next (one LDS round trip per column: stage B took
// 3.1 us where it now takes 2.0, profiles/r10_notes.md).
// ONE window suffices: foreign slots are rewritten in B1 of pass k + 1, behind stage E's barrier of pass k; own slots in stage D of pass k, behind stage
// C's barrier, and every B2 read of the pass lies in front of that barrier.  The prologue round (k = -1) has no stage C: it gets a barrier of its own
// between its B2 and its stage D, once per solve.
constexpr int kWinLoads = 12;                 // foreign slots a thread fetches per pass at most: windows of up to 12 x 512 foreign doubles
constexpr unsigned kWinZm = (1u << 5) | (1u << 8) | (1u << 10) | (1u << 15) | (1u << 17);      // columns jj = q - 1 with a z - 1 offset (q_offset) ...
constexpr unsigned kWinZp = (1u << 4) | (1u << 9) | (1u << 11) | (1u << 14) | (1u << 16);      // ... and with a z + 1 offset; the other eight are in-plane
__host__ __device__ constexpr int solve_col_seg(int jj) { return ((kWinZm >> jj) & 1u) ? 0 : ((kWinZp >> jj) & 1u) ? 2 : 1; }
constexpr bool solve_col_segs_match() { for (int jj = 0; jj < kNQ - 1; ++jj) { int o[3] = {0, 0, 0}; q_offset(jj + 1, o); if (solve_col_seg(jj) != o[2] + 1) return false; } return true; }
static_assert(solve_col_segs_match(), "the window segment of a column is its z offset");
template <int R, bool MR, bool WIN = false>
__global__ void __launch_bounds__(kSolveThreads, 2) k_cgp_solve(SweepArgs a, double* fs, double* gran, int rows_per_wg, int kmax, double* mb, unsigned long long mb_key, int force_passes, XrArgs xr) {
    __shared__ double red[8 * kSolveThreads / 64];
    // TWO workgroup barriers per pass instead of the five of a kernel that waits for its neighbours' tags (round 6: 7.05 -> 6.5 us per
    // pass).  What is left is one barrier per cross-wavefront sum: in front of stage C's reads of `red` and in front of stage E's reads of `red2`.  The sums
    // of C and E meet in buffers of their own, E's alternating by pass parity -- so neither the barrier between C's reads and E's writes nor the one behind
    // E's reads is needed: whoever writes a buffer again is two barriers further on than its last reader.  The 'a wait gave up' flag rotates through three
    // words (pass mod 3): thread 0 clears the word of pass k + 2 behind stage E's barrier of pass k -- its last readers passed that barrier with it, its next
    // raisers are two barriers away -- so the barrier that only published the cleared flag at the top of a pass goes too.  Every read of a pass's word lies
    // behind a barrier of that pass and every raise in front of it: all threads of the workgroup take the same decision.
    // (Multi-rank too: its stage C2 -- the ranks' sums -- gets a third buffer and keeps the one barrier in front of its reads: three per pass instead of seven.)
    __shared__ double red2[2 * 8 * kSolveThreads / 64];
    __shared__ double red3[MR ? 8 * kSolveThreads / 64 : 1];
    __shared__ int s_ab3[3];
#define CGP_ABORT s_ab3[(k + 3) % 3]
    const Band& b = a.b;
    const SolveWg<MR> wg(a, xr, fs, gran, rows_per_wg);
    const int G = wg.G, tid = wg.tid, lb = wg.lb;
    double* const recd[2] = {(double*)b.rec[0], (double*)b.rec[1]};      // m_k lives in recd[k & 1] (u_0 of the prologue in recd[1]): the first Spad doubles of a record plane
    // the neighbour slab's halo row of the same band row.  (xr.lo_rec / hi_rec point at the first halo RECORD, 16 bytes per row: the same row counted in doubles)
    const int lo_row0 = MR && xr.lo_rec[0] ? (int)(xr.lo_rec[0] - xr.lo_base[0]) : 0;
    auto push_record = [&](int buf, int rel, double v) {
        if (MR && rel < xr.give_lo) store8_sys((double*)xr.lo_base[buf] + lo_row0 + rel, v);
        if (MR && rel >= wg.own_n - xr.give_hi) store8_sys((double*)xr.hi_rec[buf] + (rel - (wg.own_n - xr.give_hi)), v);
    };
    using Coefs = SolveCoefs<R>;
    static_assert(!WIN || !MR, "the windowed instance exists for the single-rank kernel only");
    // WIN: the three ranges of this workgroup back to back behind the coefficients; band row i of segment s sits at win[wb<s> + i]
    double* const win = (double*)(psg_dyn_smem + Coefs::kBytes);
    int wb0 = 0, wb1 = 0, wb2 = 0, woff1 = 0, woff2 = 0, own_s = 0, own_cnt = 0, nforeign = 0;
    if constexpr (WIN) {
        const int* wt = a.pcg_win + 6 * lb;
        const int l0 = wt[1], l1 = wt[3], l2 = wt[5];
        woff1 = l0; woff2 = l0 + l1;
        wb0 = -wt[0]; wb1 = woff1 - wt[2]; wb2 = woff2 - wt[4];
        const int first = a.row0 + lb * rows_per_wg;
        own_cnt = max(0, min(a.row1, first + rows_per_wg) - first);
        own_s = own_cnt > 0 ? wb1 + first : 0;      // the own rows' slots [own_s, own_s + own_cnt) lie inside the in-plane range
        nforeign = l0 + l1 + l2 - own_cnt;
    }
    const unsigned mepoch = (1u + a.pcg_epoch % 3u) << 2;      // 1 .. 3, never the epoch of the solve before; 0 = memory no solve has written yet (the planes are zeroed when the band is built)
    unsigned cp[R][(kNQ - 1) / 2]; int row[R]; bool live[R];
    // WIN: a row slot in which no lane of this wavefront has a row (the headline partition: the third slot of wavefronts 5-7) is skipped in stages B2 and
    // D -- its products and updates were computed on a copy of the last own row and thrown away, its terms of the three sums are not added (as before:
    // live[u] guards them).  Wave-uniform; a wavefront in which the band or the workgroup's rows end keeps the per-lane guards.
    bool slot_on[R];
    double x[R], r[R], w[R], z[R], sv[R], pv[R]; float inv[R];      // every vector of the recurrences in double: see "precision" above
    fold_pending<kBlock>(a, red);      // the sums the distance sweep left pending
    // ---- once: assemble the rows of this thread (coefficients -> LDS), r_0 = b, u_0 = M^-1 b out for the neighbours
#pragma unroll
    for (int u = 0; u < R; ++u) {
        row[u] = wg.own_row(u, live[u]);
        double rhs;
        slot_on[u] = !WIN || __builtin_amdgcn_ballot_w64(live[u]) != 0;
        solve_assemble_row<R>(a, row[u], u, tid, inv[u], rhs);
        r[u] = live[u] ? (double)(float)rhs : 0.0;      // (b is the float vector the reference solves for)
        x[u] = 0.0; z[u] = 0.0; sv[u] = 0.0; pv[u] = 0.0; w[u] = 0.0;
        if (live[u]) {
            const double u0 = (double)inv[u] * r[u];
            const double ut = m_tag(u0, mepoch | 0u);
            __hip_atomic_store(recd[1] + row[u], ut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); push_record(1, row[u] - a.row0, ut); if constexpr (WIN) win[wb1 + row[u]] = ut;
        }
        solve_load_columns(b, row[u], cp[u]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) wg.publish_prologue();
    float rhsNorm2 = 0.f, thr = 0.f, rr_cur = 0.f;
    double gamma_old = 0.0, alpha = 0.0;
    int k = -1, status = 1;                   // k = -1: the extra round w_0 = A u_0
    for (;; ++k) {
        SOLVE_STAMP(0);
        const unsigned want = (unsigned)(k + 1) & 3u;      // tag of the sums published for pass k (k >= 0)
        const int pb = k & 1;                              // the buffer they were published in
        const double* gp = wg.gran_plane(pb, 0);
        const int abl = a.pcg_ablate;      // timing ablations (tools/pcg_variants.py; never set in production): 1 = every gather reads the row's own element, 4 = the 8 in-plane columns are not fetched
        solve_keep_columns_packed<R>(cp);
        // ---- A: the neighbours' m_k (k = -1: their u_0) validate themselves: nothing to wait for.  Once per solve: the 'a wait gave up' words
        if (k < 0) {
            if (tid == 0) { s_ab3[0] = 0; s_ab3[1] = 0; s_ab3[2] = 0; }
            __syncthreads();
        }
        SOLVE_STAMP(1);
        if (force_passes > 0 && k == 9 && tid == 0) fs[16 + 1536 + lb] = (double)wall_clock64();      // ... neighbours' tags of pass 9 seen
        // ---- B: n = A m (k = -1: w_0 = A u_0): 18 four-byte gathers per row in two batches of 9, software-pipelined across the rows of the thread
        const double* __restrict__ rin = recd[k >= 0 ? (k & 1) : 1];
        double nres[R];
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.0;
        auto prefetch_sums = [&] {
            if (k >= 0 && tid < G) {
#pragma unroll
                for (int q = 0; q < kCgpSums; ++q) v[q] = __hip_atomic_load(gp + (size_t)q * kSolveMaxBlocks + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
      if constexpr (WIN) {
        // ---- B1: the foreign slots tid, tid + 512, ... of the window (slot -> band row is affine per segment), every load issued before the first check
        const unsigned wantm = mepoch | want;
        double ld[kWinLoads];
        // (sums of masked differences, by value: a chain of selects among the three bases is compiled into a table in scratch memory)
        const int o1 = woff1, o2 = woff2, b2 = wb2, d21 = wb1 - wb2, d10 = wb0 - wb1, os = own_s, oc = own_cnt;
        auto slot_of = [=](int f) { return f + (oc & -(int)(f >= os)); };      // (the own rows' slots are skipped: they never travel)
        auto row_of_slot = [=](int s) { return s - (b2 + (d21 & -(int)(s < o2)) + (d10 & -(int)(s < o1))); };
#pragma unroll
        for (int j = 0; j < kWinLoads; ++j) {
            const int f = tid + j * kSolveThreads;
            ld[j] = f < nforeign ? __hip_atomic_load(rin + row_of_slot(slot_of(f)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
        // the sums of pass k were published when m_k was: requested once (PSG_WIN_PREFETCH says where), checked in stage C
        __builtin_amdgcn_sched_barrier(0);
        if (PSG_WIN_PREFETCH == 0) prefetch_sums();
        __builtin_amdgcn_sched_barrier(0);
        auto refetch = [&](const double* src) {      // a value that is not this pass's yet: ask again (the producer is at most one hand-off behind)
            int spins = 0; double vv;
            do {
                __builtin_amdgcn_s_sleep(1);
                vv = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (++spins > wg.kLocalSpins || ((spins & 255) == 0 && wg.aborted())) { CGP_ABORT = 1; break; }
            } while (m_tag_of(vv) != wantm);
            return vv;
        };
#pragma unroll
        for (int j = 0; j < kWinLoads; ++j) {
            const int f = tid + j * kSolveThreads, s = slot_of(f);
            double vv = ld[j];
            if (f < nforeign && m_tag_of(vv) != wantm) vv = refetch(rin + row_of_slot(s));
            if (f < nforeign) win[s] = vv;
        }
        if (PSG_WIN_PREFETCH == 1) prefetch_sums();
        __syncthreads();
        // ---- B2: the products from the window, the columns in the order of the gathers.  An absent column (delta 0, coefficient 0) points at the row
        // itself, which lies in the in-plane range whatever the column's segment; a row slot without a row reads slot 0 and stores nothing
#pragma unroll
        for (int u = 0; u < R; ++u) {
          nres[u] = 0.0;
          if (slot_on[u]) {
            v4f_t hc[kCoefWords];
            Coefs::template load<0, kCoefWords>(u, tid, hc);      // (the row's five words up front: they do not depend on the window)
            const double mine = (double)inv[u] * (k >= 0 ? w[u] : r[u]);      // (the row's own m: what it published)
            double acc = (double)solve_coef(hc, 0) * mine;
            const int self = wb1 + row[u];
#pragma unroll
            for (int j0 = 0; j0 < kNQ - 1; j0 += PSG_WIN_BATCH) {      // one batch: its window reads issued back to back, then its multiply-adds in column order
                double wv[PSG_WIN_BATCH];
#pragma unroll
                for (int j = 0; j < PSG_WIN_BATCH; ++j) {
                    const int jj = j0 + j;
                    const int pk = (int)cp[u][jj >> 1];
                    const int d = (jj & 1) ? (pk >> 16) : ((pk << 16) >> 16);
                    int idx = solve_col_seg(jj) == 1 ? self + d : (d != 0 ? (solve_col_seg(jj) == 0 ? wb0 : wb2) + row[u] + d : self);
                    if (!live[u]) idx = 0;
                    wv[j] = win[idx];
                }
                __builtin_amdgcn_sched_barrier(0);      // (left to itself the compiler waits for every read before it issues the next: 18 LDS round trips per row)
#pragma unroll
                for (int j = 0; j < PSG_WIN_BATCH; ++j) acc += (double)solve_coef(hc, j0 + j + 1) * wv[j];
                asm volatile("" : "+v"(acc)); __builtin_amdgcn_sched_barrier(0);      // (one batch of LDS reads at a time: all 18 R at once spill)
            }
            nres[u] = acc;
          }
            if (PSG_WIN_PREFETCH == 2 && u == 0) { prefetch_sums(); __builtin_amdgcn_sched_barrier(0); }
        }
        if (k < 0) __syncthreads();      // (no stage C in the prologue round: its B2 reads of the own range end here, stage D rewrites it)
      } else {
        double ob[kCgpDepth][9];
        auto issue = [&](int t) {
            const int u = t >> 1, j0 = (t & 1) * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int jj = j0 + j; const int pk = (int)cp[u][jj >> 1];
                constexpr unsigned kInPlane = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7) | (1u << 12) | (1u << 13);      // columns without a z offset (q_offset: q = jj + 1)
                if ((abl & 4) && ((kInPlane >> jj) & 1u)) { ob[t % kCgpDepth][j] = 0.0; continue; }      // ablation 4: the in-plane columns are not gathered at all
                const int srow = row[u] + ((abl & 1) ? 0 : ((jj & 1) ? (pk >> 16) : ((pk << 16) >> 16)));
                const double* src = rin + srow;
                //  a HALO row's value is written by the neighbour RANK: gathered at system scope from the first attempt on -- the tag alone cannot tell
                // this pass's value from the one of four passes ago (a buffer's tags alternate between two values), so the load itself must not be served from a
                // copy this device cached then.  Own rows: agent scope, as on one rank.
                if (MR && (srow < a.row0 || srow >= a.row1)) ob[t % kCgpDepth][j] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else ob[t % kCgpDepth][j] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        // The sums of pass k were published when m_k was: by the time the last gather batch is on its way they have normally arrived, but FETCHING
        // them is a memory round trip of its own (agent-scope loads past the XCD's L2: ~1.5 us if issued only after the gathers).  So they are
        // requested right behind the last batch and checked in stage C; only a late workgroup's granules are polled for again there.
#pragma unroll
        for (int t = 0; t < kCgpDepth && t < 2 * R; ++t) issue(t);
        if (2 * R - 1 - kCgpDepth < 0) { __builtin_amdgcn_sched_barrier(0); prefetch_sums(); __builtin_amdgcn_sched_barrier(0); }
        double acc = 0;
        v4f_t hc[kCoefWords];      // the row's coefficients: words 0-2 (columns 0-11) with its first batch, words 3-4 with its second
#pragma unroll
        for (int t = 0; t < 2 * R; ++t) {
            const int u = t >> 1, j0 = (t & 1) * 9;
            if (!(t & 1)) { Coefs::template load<0, 3>(u, tid, hc); const double mine = (double)inv[u] * (k >= 0 ? w[u] : r[u]); acc = (double)solve_coef(hc, 0) * mine; }      // (the row's own m: what it published)
            else Coefs::template load<3, kCoefWords>(u, tid, hc);
            {      // a value that is not this pass's yet: ask again (the producer is at most one hand-off behind)
                const unsigned wantm = mepoch | want;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    if (m_tag_of(ob[t % kCgpDepth][j]) == wantm) continue;
                    const int jj = j0 + j; const int pk = (int)cp[u][jj >> 1];
                    if ((abl & 4) && ((0x30cfu >> jj) & 1u)) continue;      // (timing ablation 4: this column was not gathered)
                    const double* src = rin + (row[u] + ((jj & 1) ? (pk >> 16) : ((pk << 16) >> 16)));
                    int spins = 0; double vv;
                    do {
                        __builtin_amdgcn_s_sleep(1);
                        vv = MR ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (a halo row is written by the neighbour RANK)
                        if (++spins > wg.kLocalSpins || ((spins & 255) == 0 && (MR ? wg.aborted_by_rank() : wg.aborted()))) { CGP_ABORT = 1; break; }
                    } while (m_tag_of(vv) != wantm);
                    ob[t % kCgpDepth][j] = vv;
                }
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) acc += (double)solve_coef(hc, j0 + j + 1) * ob[t % kCgpDepth][j];
            asm volatile("" : "+v"(acc));
            if (t & 1) nres[u] = acc;
            __builtin_amdgcn_sched_barrier(0);
            if (t + kCgpDepth < 2 * R) issue(t + kCgpDepth);
            if (t == 2 * R - 1 - kCgpDepth) prefetch_sums();
            __builtin_amdgcn_sched_barrier(0);
        }
      }
        SOLVE_STAMP(2);
        if (force_passes > 0 && k == 9 && tid == 0) { fs[16 + 1024 + lb] = (double)wall_clock64(); fs[16 + 768 + lb] = (double)wg.my_xcc; fs[16 + 1792 + lb] = (double)(gran_tag_of(v[0]) == want && gran_tag_of(v[1]) == want && gran_tag_of(v[2]) == want); }      // timing hook (PSGSDF_SOLVE_DUMP): gathers of pass 9 done; was the prefetch of this thread's granules valid?
        double beta = 0.0;
        bool stop = false;
        if (k >= 0) {
            // ---- C: the three sums for pass k of EVERY workgroup (published at the end of pass k - 1: normally all here by now)
            auto poll3 = [&](const double* base) {      // this thread's three granules at base[q * kSolveMaxBlocks] until they carry the pass's tag (v holds what prefetch_sums asked for)
                int spins = 0;
                bool ok = gran_tag_of(v[0]) == want && gran_tag_of(v[1]) == want && gran_tag_of(v[2]) == want;
                while (!ok) {
                    if (spins) __builtin_amdgcn_s_sleep(1);
                    if (++spins > wg.kLocalSpins || wg.aborted()) { CGP_ABORT = 1; break; }
                    ok = true;
#pragma unroll
                    for (int q = 0; q < kCgpSums; ++q) { v[q] = __hip_atomic_load(base + (size_t)q * kSolveMaxBlocks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ok = ok && gran_tag_of(v[q]) == want; }
                }
            };
            if (tid < G) poll3(gp + tid);
            { const double v4[4] = {v[0], v[1], v[2], 0.0}; wave_sum4_store<kSolveThreads / 64>(wave_sum4(v4), red, tid >> 6); }      // (three sums: the four-value reduce-scatter, the same bits as wave_sum8's)
            __syncthreads();
            if (CGP_ABORT) { if (tid == 0) wg.raise_abort(); status = 2; break; }
            double t[kCgpSums];
#pragma unroll
            for (int q = 0; q < kCgpSums; ++q) { double s_ = 0; for (int i = 0; i < kSolveThreads / 64; ++i) s_ += red[q * (kSolveThreads / 64) + i]; t[q] = s_; }
            if (MR) {
                // ---- C2: the sums just obtained are this RANK's: the sums over all ranks
                if (!wg.exchange_rank_sums(t, kCgpSums, pb, want, red3, &CGP_ABORT)) { status = 2; break; }
            }
            if (k == 0) { rhsNorm2 = (float)t[2]; thr = pcg_threshold(rhsNorm2); if (lb == 0 && tid == 0) fs[0] = t[2]; }
            rr_cur = (float)t[2];
            const bool rhs_zero = rhsNorm2 == 0.f;
            stop = force_passes > 0 ? k >= force_passes : (rhs_zero || k == kmax || (k > 0 && rr_cur < thr));
            if (!stop) {
                // alpha = gamma / (delta - beta gamma / alpha_old): the reference's alpha = r.z / p.Ap without the product that is still being gathered
                beta = k > 0 ? t[0] / gamma_old : 0.0;
                alpha = t[0] / (k > 0 ? t[1] - beta * t[0] / alpha : t[1]);
                gamma_old = t[0];
            }
        }
        SOLVE_STAMP(3);
        if (force_passes > 0 && k == 9 && tid == 0) fs[16 + 256 + lb] = fs[16 + 512 + lb] = (double)wall_clock64();      // ... the sums of pass 9 of all the others seen
        if (stop) break;
        if (force_passes == -7 && k == 2 && lb == 1) { status = 2; break; }      // fault injection: this workgroup never publishes pass 3
        // ---- D: the update (k = -1: w_0 = n), the three sums and m for the next pass
        double s[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] = 0.0;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (!slot_on[u]) continue;
            double ui = (double)inv[u] * r[u];
            if (k < 0) w[u] = nres[u];
            else {
                z[u] = nres[u] + beta * z[u];
                sv[u] = w[u] + beta * sv[u];
                pv[u] = ui + beta * pv[u];
                x[u] = x[u] + alpha * pv[u];
                r[u] = r[u] - alpha * sv[u];
                w[u] = w[u] - alpha * z[u];
                ui = (double)inv[u] * r[u];
            }
            const double mnext = (double)inv[u] * w[u];
            if (live[u]) {
                s[0] += r[u] * ui; s[1] += w[u] * ui; s[2] += r[u] * r[u];
                double* dst = recd[(k + 1) & 1] + row[u];
                const double mt = m_tag(mnext, mepoch | ((unsigned)(k + 2) & 3u));
                __hip_atomic_store(dst, mt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); push_record((k + 1) & 1, row[u] - a.row0, mt); if constexpr (WIN) win[wb1 + row[u]] = mt;
            }
        }
        SOLVE_STAMP(4);
        // ---- E: publish the three sums (m carries its own tag: no drain of its stores in front of them)
        const double s4[4] = {s[0], s[1], s[2], 0.0};
        const double tE = wave_sum4(s4);
        double* const redE = red2 + ((k + 1) & 1) * (8 * kSolveThreads / 64);
        wave_sum4_store<kSolveThreads / 64>(tE, redE, tid >> 6);
        __syncthreads();
        if (CGP_ABORT) { if (tid == 0) wg.raise_abort(); status = 2; break; }      // (a gather of this pass gave up)
        if (tid == 0) s_ab3[(k + 5) % 3] = 0;      // the flag of pass k + 2: its readers (pass k - 1) are past this barrier, its raisers two barriers away
        SOLVE_STAMP(5);
        if (tid < kCgpSums) {
            double tot = 0;
            for (int i = 0; i < kSolveThreads / 64; ++i) tot += redE[tid * (kSolveThreads / 64) + i];
            double* gq = gran + (size_t)((k + 1) & 1) * kSolveGranPlanes * kSolveMaxBlocks + (size_t)tid * kSolveMaxBlocks + lb;
            __hip_atomic_store(gq, gran_tag(tot, (unsigned)(k + 2) & 3u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        SOLVE_STAMP(6);
        if (force_passes > 0 && k == 8 && tid == 0) fs[16 + lb] = (double)wall_clock64();      // ... published at the end of pass 8 (m_9 and the sums of pass 9)
        if (force_passes > 0 && k == 9 && tid == 0) fs[16 + 1280 + lb] = (double)wall_clock64();  // ... and at the end of pass 9
    }
#undef CGP_ABORT
#undef SOLVE_STAMP
    // ---- leave: x of the own rows; the distance update; the outcome for the host and for the gated kernels behind this one
    // (Measured and rejected, profiles/r04_notes.md: the regrad -- k_derive -- in this epilogue behind one more neighbour hand-off.  Same bits, no
    // launch, but 2 648 vs 2 680 it/s: with one workgroup of eight waves per CU the dependent loads of three rows per thread take longer than the
    // 13 us the stand-alone kernel needs at full occupancy.)
    float xf[R];
#pragma unroll
    for (int u = 0; u < R; ++u) xf[u] = (float)x[u];
    solve_apply_and_count<MR, R>(wg, xf, row, live, status, rr_cur, rhsNorm2, red);
    if (lb == 0 && tid == 0) solve_report(fs, mb, mb_key, status, k, rr_cur, rhsNorm2, thr);
}

// ---- host side of the persistent solve: every instance takes the same arguments and the same launch shape
using SolveKernel = void (*)(SweepArgs, double*, double*, int, int, double*, unsigned long long, int, XrArgs);
static_assert(kCgpMaxRows == kSolveMaxRows && kSolveMaxRows == 4, "solve_with_rows lists the row counts");
// > 64 KB of dynamic LDS has to be asked for; returns the resident workgroups per CU (0: the instance cannot run)
static int solve_prepare(SolveKernel kern, size_t lds) {
    int n = 0;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)kern, kSolveThreads, lds) == hipSuccess ? n : 0;
}
// f(std::integral_constant<int, R>) for the R = rows per thread
template <class F> static auto solve_with_rows(int rows, F&& f) {
    switch (rows) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
static size_t solve_lds(int rows) { return solve_with_rows(rows, [](auto rc) -> size_t { return SolveCoefs<decltype(rc)::value>::kBytes; }); }      // the coefficients of `rows` row slots
// the windowed instance of the launch (pcg_window.hip): false = this band's windows do not fit (or the instance cannot be resident): nothing was launched
bool launch_cgp_solve_window(const SweepArgs& a, double* fs, double* gran, int G, int rows_per_wg, int kmax, double* mb, unsigned long long mb_key, int force_passes, hipStream_t s);

}  // namespace psg
