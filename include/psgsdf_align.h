/* psgsdf_align.h -- bring a reference surface (a scanner's ground truth, a CAD model, another run's mesh) into the coordinates of the welded mesh
 * by rigid point-to-plane ICP on the device (psgsdf_align_reference), with the nearest-point rule of psgsdf_compare.h, so that
 * psgsdf_compare_reference can then measure what is left.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has no registration.
 *
 * Definition (DESIGN.md "Alignment of a reference"; tests/_align_ref.py is its executable statement).  All arithmetic in double without contraction,
 * with IEEE / and sqrt, except where a float is named; vs is the context's float32 voxel size widened to double.  A dot product is
 * (x x' + y y') + z z'; a cross product has the components y z' - z y', z x' - x z', x y' - y x' (psgsdf_compare.h).
 *   Transform: T = [R | t], the upper 3x4 of a row-major 4x4 that takes reference units to mesh units.  Its inverse [R^T | -R^T t] is formed on the
 *     host in double: row i of R^T is column i of R, (-R^T t)_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2).
 *   Moved point: M(p) = (float)(((r0 x + r1 y) + r2 z) + t) per row (r0 r1 r2 | t) of a 3x4 transform M, p widened to double.  Direction 1's
 *     queries are T(ref_i), direction 2's are T^-1(vertex_j).  Both always start from the caller's points and the mesh's vertices, never from
 *     points moved before.  A NaN coordinate stays NaN.
 *   Correspondence: psgsdf_compare.h's nearest target within the iteration's radius -- smallest D2 over ALL targets, ties to the smaller index --
 *     and the closest point q of the same pair function.  Direction 1: the targets are the compared mesh's faces.  Direction 2: the targets are the
 *     reference's faces, or its points if it has none.  Invalid and unmatched queries give no row.
 *   Row, direction 1: x = the moved point widened to double; m = (b - a) x (c - a) of the winning face, n = m / sqrt(m . m) (each component
 *     divided); r = n . (x - q).
 *   Row, direction 2: x = T q in double, ((r0 qx + r1 qy) + r2 qz) + t per row, not rounded to float; m = the vertex's stored normal widened,
 *     n = m / sqrt(m . m); r = n . (x - vertex).  The planes are always the reconstruction's, so a cloud reference works in both directions.
 *   A row whose n has a non-finite component is skipped.
 *   System: c = the centre of the bounding box of the compared mesh's finite vertices, (lo + hi) / 2 per axis (zero without one);
 *     y = (x - c) / vs per component, rho = r / vs, J = [y x n, n];
 *     A = sum J J^T, g = sum J rho, e = sum rho^2, n = sum 1 over the rows of both directions.  The sums are added in one fixed order that depends only
 *     on the numbers of queries -- no floating-point atomics, nothing depends on the launch chunk or the search grid -- so two calls on the same
 *     state give the same bytes.
 *   Step (host, double): radius_k = max(min_dist, max_dist shrink^k), the power by k multiplications.  From the system at T with radius_k:
 *     n < 6 ends with status TOO_FEW.  Else with s_i = sqrt(A_ii), the Cholesky factorisation of S_ij = A_ij / (s_i s_j), pivot by pivot;
 *     a pivot <= 1e-6 (or not a number) ends with status DEGENERATE.  Neither takes a step: transform stays the last one.  Else
 *     S z = -(g_i / s_i), xi_i = z_i / s_i, xi = (omega, u), v = u vs, and with Delta(x) = c + Exp(omega)(x - c) + v: T <- Delta o T, that is
 *     R <- E R, t <- E t + ((c - E c) + v), E = Exp(omega) = I + a K + b K K, K the cross-product matrix of omega, theta = |omega|,
 *     a = sin theta / theta, b = (1 - cos theta) / theta^2, and below theta = 1e-8 the series a = 1 - theta^2 / 6, b = 1/2 - theta^2 / 24.
 *     CONVERGED when |omega| <= eps_rot and |v| <= eps_trans hold for the step just taken, else MAX_ITERS after max_iters steps.  After the
 *     last step the system is evaluated once more, at `transform` with the radius of the next iteration, into `final`.  max_iters = 0 gives
 *     system0 and final at init, status MAX_ITERS (TOO_FEW with fewer than 6 rows).  When TOO_FEW or DEGENERATE end the call, `final` is the
 *     evaluation that ended it and iters[n_iters] holds its radius, rms, n_pairs and min_pivot (the pivot that refused) with a zero step.
 *   min_pivot 1e-6: on the five-piece test scene the smallest pivot is >= 0.6, on a plane (three free motions) <= 1e-11.
 *
 * The compared mesh is bit for bit psgsdf_extract_mesh_indexed's (filter == NULL) or psgsdf_extract_mesh_components' kept mesh (filter != NULL), as
 * in psgsdf_compare_reference.  grid_cell sizes the two search grids (0: the engine's choice); acceleration only: no result depends on it.
 * Limits: ICP is local -- init must lie in the basin of the answer, there is no global search; direction 2 alone needs a reference that covers
 * the reconstruction (vertices of uncovered parts match whatever is within the radius); rigid only, no scale; single contexts only.
 *
 * Valid once a volume exists; a band is not required.  Two calls on the same state give the same bytes, and the call changes no result of any other
 * call.  The arrays are engine-owned pinned host memory, valid until the next extraction call on the context.  An empty reconstruction, n_ref == 0
 * or fewer than 6 rows is not an error: PSGSDF_OK with status TOO_FEW and transform = init.
 * PSGSDF_ERR_STATE before a volume exists.  PSGSDF_ERR_ARG for a NULL params, out, or ref_xyz with n_ref > 0; n_ref < 0 or > 2^31 - 1, n_ref_faces
 * < 0, or NULL ref_faces with n_ref_faces > 0; a face index outside [0, n_ref) (checked before anything uses it); parameters outside their ranges
 * below, non-zero reserved included; a filter psgsdf_extract_mesh_components refuses.  PSGSDF_ERR_UNSUPPORTED if n_ref_faces or a search grid's
 * entries exceed 2^31 - 1.  PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused (everything is freed).  A call that fails its
 * argument checks leaves *out untouched; one that fails later leaves it zeroed.
 * On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_ALIGN_H_
#define PSGSDF_ALIGN_H_

#include "psgsdf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgsdf_align_params {
    double init[16];      /* row-major 4x4, reference units -> mesh units; rigid: last row 0 0 0 1, every entry of R^T R - I within 1e-6, all finite */
    double max_dist;      /* matching radius of iteration 0; finite, 0 < max_dist <= 64 vs */
    double min_dist;      /* floor of the radius; finite, 0 < min_dist <= max_dist */
    double shrink;        /* radius_k = max(min_dist, max_dist * shrink^k); 0 < shrink <= 1 */
    double eps_rot;       /* stop when |omega| <= eps_rot (rad) and |v| <= eps_trans (mesh units); finite, >= 0 */
    double eps_trans;
    double grid_cell;     /* as in psgsdf_compare_params: acceleration only; finite, >= 0 */
    int32_t directions;   /* 1 reference points -> mesh faces, 2 mesh vertices -> reference targets, 3 both */
    int32_t max_iters;    /* 0 .. 64; 0 = evaluate at init only */
    int32_t reserved[2];  /* 0 */
} psgsdf_align_params;

typedef struct psgsdf_align_iter {   /* the state the step was computed from, and the step */
    double radius, rms;              /* rms = vs * sqrt(e / n) over both directions' rows (0 without a row) */
    int64_t n_pairs[2];              /* rows of direction 1, direction 2 */
    double min_pivot;                /* smallest pivot of the scaled system's Cholesky factorisation */
    double step[6];                  /* omega (rad), v (mesh units) */
} psgsdf_align_iter;

enum { PSGSDF_ALIGN_CONVERGED = 0, PSGSDF_ALIGN_MAX_ITERS = 1, PSGSDF_ALIGN_DEGENERATE = 2, PSGSDF_ALIGN_TOO_FEW = 3 };

typedef struct psgsdf_align {
    double transform[16];            /* reference -> mesh units, row-major */
    double centre[3];                /* c above */
    int32_t status, n_iters;         /* n_iters = steps taken = filled entries of iters[] */
    psgsdf_align_iter iters[64];
    double system0[28];              /* at init: A's upper triangle row-major (21), g (6), e (1) */
    psgsdf_align_iter final;         /* the evaluation at `transform` (radius of the next iteration); step and min_pivot 0 */
    const float* aligned_xyz; int64_t n_ref;   /* the reference points under `transform` as float32: what the last search saw; pinned, valid until the next extraction call */
    /* the reconstruction's mesh the reference was aligned to, as in psgsdf_compare */
    const float* xyz; const float* normals; const uint8_t* rgb; const int32_t* faces; int64_t n_vertices, n_faces;
} psgsdf_align;

int psgsdf_align_reference(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, const float* ref_xyz, int64_t n_ref,
                           const int32_t* ref_faces, int64_t n_ref_faces, const psgsdf_align_params* params, psgsdf_align* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_ALIGN_H_ */
