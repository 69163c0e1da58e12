// extract_compare.hip -- the C ABI of include/psgsdf_compare.h: distances between the welded mesh and a reference mesh or cloud (kernels: compare.hip;
// DESIGN.md "Comparison with a reference"), and of include/psgsdf_align.h: the reference's rigid alignment to that mesh (align.hip and compare.hip's
// search; "Alignment of a reference").  The grid's snapping, the statistics, the solve and the composition are compared bit for bit: no FMA contraction.
#pragma clang fp contract(off)
#include "mesh_stages.h"
#include "../../include/psgsdf_compare.h"
#include "../../include/psgsdf_align.h"
#include "compare.h"
#include "align.h"

using namespace psge;

// ---- what both calls start from: the caller's reference checked and uploaded once, the welded mesh (or its kept components) on the device and in
// the slots of the call it mirrors
namespace {
struct RefIn { const float* xyz; int64_t n; const int32_t* faces; int64_t nf; };
// the first checks: null arguments, ranks, counts (a call's own parameters come between these and reference_ready)
int reference_args(psgsdf_ctx* c, const char* me, const void* params, const void* out, const RefIn& r) {
    if (!params || !out || (r.n > 0 && !r.xyz)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, "a slab holds only its own share of the mesh")) return rc;
    if (r.n < 0 || r.n > (int64_t)INT32_MAX || r.nf < 0 || (r.nf > 0 && !r.faces))
        return fail(c, PSGSDF_ERR_ARG, "%s: %lld reference points, %lld faces%s", me, (long long)r.n, (long long)r.nf, r.nf > 0 && !r.faces ? " (null)" : "");
    return PSGSDF_OK;
}
// the last ones: the 64-voxel rule, the face indices (on the host, before anything uses them), the filter, the face count limit, extract_ready
int reference_ready(psgsdf_ctx* c, const char* me, const RefIn& r, double max_dist, const psgsdf_mesh_filter* filter) {
    if (c && c->have_volume && max_dist > 64.0 * (double)c->grid.vs) return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g is more than 64 voxels of %g", me, max_dist, (double)c->grid.vs);
    for (int64_t i = 0; i < 3 * r.nf; ++i)
        if (r.faces[i] < 0 || (int64_t)r.faces[i] >= r.n) return fail(c, PSGSDF_ERR_ARG, "%s: face %lld has the index %d (%lld reference points)", me, (long long)(i / 3), r.faces[i], (long long)r.n);
    if (filter && bad_filter(*filter)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    if (r.nf > (int64_t)INT32_MAX) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld reference faces", me, (long long)r.nf);
    return extract_ready(c, me);
}
int reference_oom(psgsdf_ctx* c, const char* me, const RefIn& r) {
    return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld reference points, %lld faces)", me, (long long)r.n, (long long)r.nf);
}
int upload_reference(psgsdf_ctx* c, DevMem& mem, const char* me, const RefIn& r, float** d_xyz, int** d_faces) {
    if ((r.n > 0 && !mem.get(d_xyz, 3 * (size_t)r.n)) || (r.nf > 0 && !mem.get(d_faces, 3 * (size_t)r.nf))) return reference_oom(c, me, r);
    if ((r.n > 0 && hipMemcpyAsync(*d_xyz, r.xyz, sizeof(float) * 3 * (size_t)r.n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        || (r.nf > 0 && hipMemcpyAsync(*d_faces, r.faces, sizeof(int) * 3 * (size_t)r.nf, hipMemcpyHostToDevice, c->stream) != hipSuccess))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    return PSGSDF_OK;
}
// the search grid's cell, and the margin of its box: max_dist and a little more, so that rounding never drops a pair at the rim
double grid_cell_of(double grid_cell, double vs) { return grid_cell > 0.0 ? grid_cell : 2.0 * vs; }
double grid_margin(double max_dist, double cell) { return max_dist * (1.0 + 1e-6) + 1e-6 * cell; }

// ---- comparison: each direction is a grid build over its targets, the search, and the integer reductions.
struct CmpBox { double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}; bool any = false; };
// the bounding box of the finite points
CmpBox cmp_bbox(const float* xyz, size_t n) {
    CmpBox b;
    for (size_t i = 0; i < n; ++i) {
        const float* p = xyz + 3 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(b.lo[k], (double)p[k]); b.hi[k] = std::max(b.hi[k], (double)p[k]); }
        b.any = true;
    }
    return b;
}
struct CmpOut { XoSlot s_dist, s_nearest, s_side; const float** dist; const int32_t** nearest; const int8_t** side; };
// the uniform grid over a.t_* (a.nt targets) and the box [lo, hi] into a.g (none if !box.any or without a target); waits for the stream once (the
// grid's size).  Shared by psgsdf_compare_reference and psgsdf_align_reference.
int compare_grid(psgsdf_ctx* c, DevMem& mem, const char* me, psg::CompareArgs& a, const CmpBox& box, double cell) {
    psg::CompareGrid& g = a.g;
    g = psg::CompareGrid{};
    if (!(a.nt > 0 && box.any)) return PSGSDF_OK;
    if (!mem.get(&a.total, 1)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me);
    if (hipMemsetAsync(a.total, 0, sizeof(unsigned long long), c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    // the cells: edge `cell`, doubled until the grid fits kCompareMaxCells (acceleration only: no result depends on it)
    // and the lower corner snapped down to a whole number of cells, so that the walls are the multiples of the edge
    double h = cell, nd[3], lo[3];
    for (;;) {
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) { lo[k] = floor(box.lo[k] / h) * h; nd[k] = std::max(1.0, ceil((box.hi[k] - lo[k]) / h)); cells *= nd[k]; }
        if (cells <= (double)psg::kCompareMaxCells) break;
        h *= 2.0;
    }
    g.h = h; g.cells = 1;
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.n[k] = (int)nd[k]; g.cells *= g.n[k]; }
    int* sums = nullptr;
    if (!mem.get(&g.start, (size_t)g.cells + 1) || !mem.get(&g.cursor, (size_t)g.cells) || !mem.get(&sums, (size_t)((g.cells + 1 + psg::kTile - 1) / psg::kTile + 1)))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld grid cells)", me, g.cells);
    if (hipMemsetAsync(g.start, 0, sizeof(int) * ((size_t)g.cells + 1), c->stream) != hipSuccess || hipMemsetAsync(g.cursor, 0, sizeof(int) * (size_t)g.cells, c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    hipError_t e = hipSuccess;
    unsigned long long total = 0;
    timed(c, "compare_total", [&] { e = psg::launch_compare_total(a, c->stream); });
    if (e != hipSuccess || hipMemcpyAsync(&total, a.total, sizeof(total), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: the grid's size", me);
    if (total > (unsigned long long)INT32_MAX)
        return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: the search grid would need %llu entries for %d targets (cells of %g): tessellate it", me, total, a.nt, h);
    timed(c, "compare_count", [&] { e = psg::launch_compare_count(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    int tot = 0;
    if (int rc = scan_counts(c, g.start, g.cells + 1, sums, &tot)) return rc;      // counts -> the cells' first entries; start[cells] = the total
    if ((unsigned long long)tot != total) return fail(c, PSGSDF_ERR_DEVICE, "%s: the grid's counts (%d) and its total (%llu) differ", me, tot, total);
    if (!mem.get(&g.entries, (size_t)tot)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d grid entries)", me, tot);
    timed(c, "compare_fill", [&] { e = psg::launch_compare_fill(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    return PSGSDF_OK;
}
// the per-query arrays the search writes
bool compare_query_arrays(DevMem& mem, psg::CompareArgs& a) {
    const size_t nq = (size_t)a.nq;
    return mem.get(&a.d, nq) && mem.get(&a.dist, nq) && mem.get(&a.nearest, nq) && mem.get(&a.side, nq) && mem.get(&a.pairs, nq);
}
// one direction: a.t_*, a.nt, a.q_xyz, a.nq and the parameters are set; the grid over the box [lo, hi] (none if !box), the search, the
// statistics; the per-query arrays in their pinned slots (the stream has been waited for)
int compare_direction(psgsdf_ctx* c, DevMem& mem, const char* me, psg::CompareArgs a, const CmpBox& box, double cell, int dir, const CmpOut& o, psgsdf_compare_side* S) {
    *S = psgsdf_compare_side{};
    S->n = a.nq;
    c->cmp_queries[dir] = a.nq; c->cmp_pairs[dir] = 0;
    if (a.nq == 0) return PSGSDF_OK;
    const size_t nq = (size_t)a.nq;
    if (!compare_query_arrays(mem, a) || !mem.get(&a.stats, (size_t)psg::kCmpStats)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq);
    if (hipMemsetAsync(a.stats, 0, sizeof(unsigned long long) * psg::kCmpStats, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    if (int rc = compare_grid(c, mem, me, a, box, cell)) return rc;
    hipError_t e = hipSuccess;
    timed(c, dir ? "compare_query_rec" : "compare_query_ref", [&] { e = psg::launch_compare_query(a, c->knob.compare_chunk, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch of %lld queries: %s", me, a.nq, hipGetErrorString(e));
    timed(c, "compare_stats", [&] { e = psg::launch_compare_stats(a, c->stream); });
    if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
    unsigned long long st[psg::kCmpStats] = {};
    if (hipMemcpyAsync(st, a.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the statistics", me);
    if (int rc = download(c, me, {{o.s_dist, a.dist, sizeof(float) * nq, o.dist}, {o.s_nearest, a.nearest, sizeof(int) * nq, o.nearest}, {o.s_side, a.side, nq, o.side}})) return rc;
    S->n_valid = (int64_t)st[psg::CS_VALID]; S->n_matched = (int64_t)st[psg::CS_MATCHED]; S->n_within_tau = (int64_t)st[psg::CS_TAU];
    S->sum_d = (int64_t)st[psg::CS_SUM_D]; S->sum_d2 = (int64_t)st[psg::CS_SUM_D2]; S->sum_signed = (int64_t)st[psg::CS_SIGNED];
    for (int b = 0; b < 16; ++b) S->hist[b] = (int64_t)st[psg::CS_HIST + b];
    memcpy(&S->max, &st[psg::CS_MAX], sizeof(double));
    if (S->n_matched > 0) {
        const double m = (double)S->n_matched, unit = 1048576.0;
        S->mean = a.vs * ((double)S->sum_d / unit) / m;
        S->rms = a.vs * sqrt(((double)S->sum_d2 / unit) / m);
        S->mean_signed = a.vs * ((double)S->sum_signed / unit) / m;
    }
    c->cmp_pairs[dir] = (long long)st[psg::CS_PAIRS];
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_compare_reference(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float* ref_xyz, int64_t n_ref, const int32_t* ref_faces, int64_t n_ref_faces,
                                        const psgsdf_compare_params* params, psgsdf_compare* out) {
    const char* me = "compare_reference";
    const RefIn ref{ref_xyz, n_ref, ref_faces, n_ref_faces};
    if (int rc = reference_args(c, me, params, out, ref)) return rc;
    const psgsdf_compare_params& P = *params;
    if (!(P.max_dist > 0.0) || std::isinf(P.max_dist) || !(P.tau > 0.0) || !(P.tau <= P.max_dist) || !(P.grid_cell >= 0.0) || std::isinf(P.grid_cell) || P.reserved[0] != 0 || P.reserved[1] != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g, tau %g, grid_cell %g, reserved %d %d (finite, 0 < tau <= max_dist, grid_cell >= 0, reserved 0)", me, P.max_dist, P.tau, P.grid_cell, P.reserved[0], P.reserved[1]);
    if (int rc = reference_ready(c, me, ref, P.max_dist, filter)) return rc;
    *out = psgsdf_compare{};
    const double vs = (double)c->grid.vs;
    DevMem mem(c);
    MeshView mv;
    if (int rc = compared_mesh(c, mem, me, filter, &mv)) return rc;
    const size_t nv = (size_t)mv.nv, nf = (size_t)mv.nf;
    psgsdf_compare r{};
    if (int rc = download_mesh(c, me, mv, {&r.xyz, &r.normals, &r.rgb, &r.faces})) return rc;
    r.n_vertices = (int64_t)nv; r.n_faces = (int64_t)nf;
    float* d_rxyz = nullptr; int* d_rfaces = nullptr;
    if (int rc = upload_reference(c, mem, me, ref, &d_rxyz, &d_rfaces)) return rc;
    // one box for both grids: a matching pair has its query in the queries' box and its closest point within max_dist of it and in the targets'
    // box, so both lie in the intersection of the two boxes inflated by max_dist
    const double cell = grid_cell_of(P.grid_cell, vs), grow = grid_margin(P.max_dist, cell);
    const CmpBox bm = cmp_bbox(r.xyz, nv), br = cmp_bbox(ref_xyz, (size_t)n_ref);
    CmpBox box; box.any = bm.any && br.any;
    for (int k = 0; k < 3 && box.any; ++k) {
        box.lo[k] = std::max(bm.lo[k], br.lo[k]) - grow; box.hi[k] = std::min(bm.hi[k], br.hi[k]) + grow;
        if (!(box.lo[k] <= box.hi[k])) box.any = false;      // the two are farther apart than 2 max_dist: nothing matches
    }
    psg::CompareArgs a{};
    a.max_dist = P.max_dist; a.tau = P.tau; a.vs = vs;
    // the mesh's vertices against the reference
    a.q_xyz = mv.xyz; a.nq = (long long)nv;
    a.t_xyz = d_rxyz; a.t_faces = d_rfaces; a.nt = (int)(n_ref_faces > 0 ? n_ref_faces : n_ref);
    if (int rc = compare_direction(c, mem, me, a, box, cell, 0, CmpOut{XO_CMP_VDIST, XO_CMP_VNEAREST, XO_CMP_VSIDE, &r.vertex_dist, &r.vertex_nearest, &r.vertex_side}, &r.to_reference)) return rc;
    // the reference's points against the mesh's faces
    a.q_xyz = d_rxyz; a.nq = (long long)n_ref;
    a.t_xyz = mv.xyz; a.t_faces = mv.faces; a.nt = (int)nf;
    if (int rc = compare_direction(c, mem, me, a, box, cell, 1, CmpOut{XO_CMP_RDIST, XO_CMP_RNEAREST, XO_CMP_RSIDE, &r.ref_dist, &r.ref_nearest, &r.ref_side}, &r.to_reconstruction)) return rc;
    if (r.to_reference.n_valid > 0) r.precision = (double)r.to_reference.n_within_tau / (double)r.to_reference.n_valid;
    if (r.to_reconstruction.n_valid > 0) r.recall = (double)r.to_reconstruction.n_within_tau / (double)r.to_reconstruction.n_valid;
    if (r.precision + r.recall > 0.0) r.fscore = 2.0 * r.precision * r.recall / (r.precision + r.recall);
    *out = r;
    return PSGSDF_OK;
}

// ---- alignment: the two grids are built once, every evaluation moves the points, searches, reduces the rows to one 6x6 system on the device and
// brings 32 doubles to the host, which solves and composes in double.
namespace {
// the step of the header: 0 and xi, or 1 (a pivot <= 1e-6: degenerate); *min_pivot the smallest pivot met
int align_solve(const double* sys, double* min_pivot, double* xi) {
    double A[6][6], S[6][6], L[6][6] = {}, s[6], b[6], z[6], w[6];
    for (int i = 0, k = 0; i < 6; ++i) for (int j = i; j < 6; ++j, ++k) A[i][j] = A[j][i] = sys[psg::AL_A + k];
    *min_pivot = 0.0;
    for (int i = 0; i < 6; ++i) { if (!(A[i][i] > 0.0)) return 1; s[i] = sqrt(A[i][i]); }
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) S[i][j] = A[i][j] / (s[i] * s[j]);
    double mp = INFINITY;
    for (int j = 0; j < 6; ++j) {
        double d = S[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d >= mp)) mp = d;
        *min_pivot = mp;
        if (!(d > 1e-6)) return 1;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = S[i][j];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) b[i] = -(sys[psg::AL_G + i] / s[i]);
    for (int i = 0; i < 6; ++i) { double v = b[i]; for (int k = 0; k < i; ++k) v = v - L[i][k] * z[k]; z[i] = v / L[i][i]; }
    for (int i = 5; i >= 0; --i) { double v = z[i]; for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * w[k]; w[i] = v / L[i][i]; }
    for (int i = 0; i < 6; ++i) xi[i] = w[i] / s[i];
    return 0;
}
inline double aln_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// T <- Delta o T with Delta(x) = c + Exp(omega)(x - c) + v; T is 3x4 row-major
void align_compose(double* T, const double* om, const double* v, const double* c) {
    const double th2 = aln_dot(om, om), th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; } else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double K[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double E[3][3], N[12];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * (om[i] * om[j] - (i == j ? th2 : 0.0));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N[4 * i + j] = (E[i][0] * T[j] + E[i][1] * T[4 + j]) + E[i][2] * T[8 + j];
        const double t[3] = {T[3], T[7], T[11]};
        N[4 * i + 3] = aln_dot(E[i], t) + ((c[i] - aln_dot(E[i], c)) + v[i]);
    }
    memcpy(T, N, sizeof(N));
}
}  // namespace

extern "C" int psgsdf_align_reference(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, const float* ref_xyz, int64_t n_ref, const int32_t* ref_faces, int64_t n_ref_faces,
                                      const psgsdf_align_params* params, psgsdf_align* out) {
    const char* me = "align_reference";
    const RefIn ref{ref_xyz, n_ref, ref_faces, n_ref_faces};
    if (int rc = reference_args(c, me, params, out, ref)) return rc;
    const psgsdf_align_params& P = *params;
    {   // init: finite, last row 0 0 0 1, R^T R = I to 1e-6
        bool rigid = P.init[12] == 0.0 && P.init[13] == 0.0 && P.init[14] == 0.0 && P.init[15] == 1.0;
        for (int i = 0; i < 12; ++i) rigid = rigid && std::isfinite(P.init[i]);
        for (int i = 0; i < 3 && rigid; ++i)
            for (int j = 0; j < 3; ++j) {
                const double g = (P.init[i] * P.init[j] + P.init[4 + i] * P.init[4 + j]) + P.init[8 + i] * P.init[8 + j];
                rigid = rigid && fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-6;
            }
        if (!rigid) return fail(c, PSGSDF_ERR_ARG, "%s: init is not a rigid transform (finite, last row 0 0 0 1, R^T R = I to 1e-6)", me);
    }
    if (!(P.max_dist > 0.0) || std::isinf(P.max_dist) || !(P.min_dist > 0.0) || !(P.min_dist <= P.max_dist) || !(P.shrink > 0.0) || !(P.shrink <= 1.0) || !(P.eps_rot >= 0.0) || std::isinf(P.eps_rot)
        || !(P.eps_trans >= 0.0) || std::isinf(P.eps_trans) || !(P.grid_cell >= 0.0) || std::isinf(P.grid_cell) || P.directions < 1 || P.directions > 3 || P.max_iters < 0 || P.max_iters > 64
        || P.reserved[0] != 0 || P.reserved[1] != 0)
        return fail(c, PSGSDF_ERR_ARG, "%s: max_dist %g, min_dist %g, shrink %g, eps_rot %g, eps_trans %g, grid_cell %g, directions %d, max_iters %d, reserved %d %d (finite, 0 < min_dist <= max_dist, 0 < shrink <= 1, "
                    "eps >= 0, grid_cell >= 0, directions 1 .. 3, max_iters 0 .. 64, reserved 0)", me, P.max_dist, P.min_dist, P.shrink, P.eps_rot, P.eps_trans, P.grid_cell, P.directions, P.max_iters, P.reserved[0], P.reserved[1]);
    if (int rc = reference_ready(c, me, ref, P.max_dist, filter)) return rc;
    *out = psgsdf_align{};
    const double vs = (double)c->grid.vs;
    c->aln_evals = c->aln_iters = 0; c->aln_pairs[0] = c->aln_pairs[1] = c->aln_queries[0] = c->aln_queries[1] = 0;
    DevMem mem(c);
    MeshView mv;
    if (int rc = compared_mesh(c, mem, me, filter, &mv)) return rc;
    const size_t nv = (size_t)mv.nv, nf = (size_t)mv.nf;
    psgsdf_align r{};
    if (int rc = download_mesh(c, me, mv, {&r.xyz, &r.normals, &r.rgb, &r.faces})) return rc;
    r.n_vertices = (int64_t)nv; r.n_faces = (int64_t)nf; r.n_ref = n_ref;
    memcpy(r.transform, P.init, sizeof(r.transform));
    // the reference and the moved points of both directions
    const bool dir1 = (P.directions & 1) != 0, dir2 = (P.directions & 2) != 0;
    float *d_rxyz = nullptr, *d_mref = nullptr, *d_mvert = nullptr; int* d_rfaces = nullptr;
    if ((n_ref > 0 && !mem.get(&d_mref, 3 * (size_t)n_ref)) || (dir2 && nv > 0 && !mem.get(&d_mvert, 3 * nv))) return reference_oom(c, me, ref);
    if (int rc = upload_reference(c, mem, me, ref, &d_rxyz, &d_rfaces)) return rc;
    // each grid covers its targets' box inflated by max_dist: the radius only shrinks, and the search clamps or skips a query outside the box
    const double cell = grid_cell_of(P.grid_cell, vs), grow = grid_margin(P.max_dist, cell);
    CmpBox bm = cmp_bbox(r.xyz, nv), br = cmp_bbox(ref_xyz, (size_t)n_ref);
    double ctr[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3 && bm.any; ++k) ctr[k] = (bm.lo[k] + bm.hi[k]) / 2.0;
    memcpy(r.centre, ctr, sizeof(ctr));
    for (int k = 0; k < 3; ++k) { bm.lo[k] -= grow; bm.hi[k] += grow; br.lo[k] -= grow; br.hi[k] += grow; }
    psg::AlignRowArgs R1{}, R2{};
    int nb1 = 0, nb2 = 0;
    double* d_sys = nullptr;
    if (!mem.get(&d_sys, (size_t)psg::kAlignSys)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory", me);
    if (dir1 && n_ref > 0) {      // the moved reference points against the mesh's faces
        psg::CompareArgs& a = R1.s;
        a.vs = vs; a.tau = P.max_dist; a.max_dist = P.max_dist;
        a.q_xyz = d_mref; a.nq = (long long)n_ref; a.t_xyz = mv.xyz; a.t_faces = mv.faces; a.nt = (int)nf;
        nb1 = (int)psg::align_row_blocks(a.nq);
        if (!compare_query_arrays(mem, a) || !mem.get(&R1.partial, (size_t)nb1 * psg::kAlignRow)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq);
        if (int rc = compare_grid(c, mem, me, a, bm, cell)) return rc;
    }
    if (dir2 && nv > 0) {         // the mesh's vertices, moved into the reference's units, against the reference's targets
        psg::CompareArgs& a = R2.s;
        a.vs = vs; a.tau = P.max_dist; a.max_dist = P.max_dist;
        a.q_xyz = d_mvert; a.nq = (long long)nv; a.t_xyz = d_rxyz; a.t_faces = d_rfaces; a.nt = (int)(n_ref_faces > 0 ? n_ref_faces : n_ref);
        nb2 = (int)psg::align_row_blocks(a.nq);
        if (!compare_query_arrays(mem, a) || !mem.get(&R2.partial, (size_t)nb2 * psg::kAlignRow)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld queries)", me, a.nq);
        if (int rc = compare_grid(c, mem, me, a, br, cell)) return rc;
    }
    for (psg::AlignRowArgs* R : {&R1, &R2}) { memcpy(R->c, ctr, sizeof(ctr)); R->vs = vs; R->v_xyz = mv.xyz; R->v_nrm = mv.nrm; }
    double T[12];
    memcpy(T, P.init, sizeof(T));
    // one evaluation at T with the radius: 32 doubles and one wait
    auto evaluate = [&](double radius, double* sys) -> int {
        double Ti[12];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Ti[4 * i + j] = T[4 * j + i];
            Ti[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
        }
        hipError_t e = hipSuccess;
        psg::AlignMoveArgs m{};
        memcpy(m.M, T, sizeof(T)); m.src = d_rxyz; m.dst = d_mref; m.n = (long long)n_ref;
        timed(c, "align_move", [&] { e = psg::launch_align_move(m, c->stream); });
        if (e == hipSuccess && nb2 > 0) {
            memcpy(m.M, Ti, sizeof(Ti)); m.src = mv.xyz; m.dst = d_mvert; m.n = (long long)nv;
            timed(c, "align_move", [&] { e = psg::launch_align_move(m, c->stream); });
        }
        if (e == hipSuccess && nb1 > 0) {
            R1.s.max_dist = radius;
            timed(c, "align_query_1", [&] { e = psg::launch_compare_query(R1.s, c->knob.compare_chunk, c->stream); });
            if (e == hipSuccess) timed(c, "align_rows_1", [&] { e = psg::launch_align_rows(R1, 1, c->stream); });
        }
        if (e == hipSuccess && nb2 > 0) {
            R2.s.max_dist = radius; memcpy(R2.T, T, sizeof(T));
            timed(c, "align_query_2", [&] { e = psg::launch_compare_query(R2.s, c->knob.compare_chunk, c->stream); });
            if (e == hipSuccess) timed(c, "align_rows_2", [&] { e = psg::launch_align_rows(R2, 2, c->stream); });
        }
        if (e == hipSuccess) timed(c, "align_fold", [&] { e = psg::launch_align_fold(R1.partial, nb1, R2.partial, nb2, d_sys, c->stream); });
        if (e != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch: %s", me, hipGetErrorString(e));
        if (hipMemcpyAsync(sys, d_sys, sizeof(double) * psg::kAlignSys, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(c, PSGSDF_ERR_DEVICE, "%s: download of the system", me);
        c->aln_evals += 1;
        c->aln_queries[0] += nb1 > 0 ? R1.s.nq : 0; c->aln_queries[1] += nb2 > 0 ? R2.s.nq : 0;
        c->aln_pairs[0] += (long long)sys[psg::AS_PAIRS]; c->aln_pairs[1] += (long long)sys[psg::AS_PAIRS + 1];
        return PSGSDF_OK;
    };
    r.status = PSGSDF_ALIGN_MAX_ITERS;
    bool last = P.max_iters == 0;
    double pw = 1.0;
    for (int k = 0;; ++k) {
        const double radius = std::max(P.min_dist, P.max_dist * pw);
        double sys[psg::kAlignSys];
        if (int rc = evaluate(radius, sys)) return rc;
        if (k == 0) memcpy(r.system0, sys, sizeof(r.system0));
        psgsdf_align_iter it{};
        const double n = sys[psg::AS_N] + sys[psg::AS_N + 1];
        it.radius = radius; it.rms = n > 0.0 ? vs * sqrt(sys[psg::AL_E] / n) : 0.0;
        it.n_pairs[0] = (int64_t)sys[psg::AS_N]; it.n_pairs[1] = (int64_t)sys[psg::AS_N + 1];
        r.final = it;
        if (last) { if (r.n_iters == 0 && n < 6.0) r.status = PSGSDF_ALIGN_TOO_FEW; break; }
        if (n < 6.0) { r.status = PSGSDF_ALIGN_TOO_FEW; r.iters[k] = it; break; }
        double xi[6];
        const int deg = align_solve(sys, &it.min_pivot, xi);
        if (deg) { r.status = PSGSDF_ALIGN_DEGENERATE; r.iters[k] = it; break; }
        const double v[3] = {xi[3] * vs, xi[4] * vs, xi[5] * vs};
        for (int i = 0; i < 3; ++i) { it.step[i] = xi[i]; it.step[3 + i] = v[i]; }
        r.iters[k] = it; r.n_iters = k + 1;
        align_compose(T, xi, v, ctr);
        memcpy(r.transform, T, sizeof(T));
        const bool conv = sqrt(aln_dot(xi, xi)) <= P.eps_rot && sqrt(aln_dot(v, v)) <= P.eps_trans;
        if (conv) r.status = PSGSDF_ALIGN_CONVERGED;
        last = conv || k + 1 == P.max_iters;
        pw *= P.shrink;
    }
    c->aln_iters = r.n_iters;
    if (int rc = download(c, me, {{XO_ALN_XYZ, d_mref, sizeof(float) * 3 * (size_t)n_ref, &r.aligned_xyz}})) return rc;
    *out = r;
    return PSGSDF_OK;
}
