/* psgsdf_compare.h -- how far the reconstructed surface is from a surface the caller trusts (a scanner's ground truth, a CAD model, the synthetic
 * scene's analytic shape, last week's reconstruction): two-sided nearest distances between the welded mesh and a reference mesh or point cloud,
 * and accuracy / completeness / F-score at a threshold, computed on the device (psgsdf_compare_reference).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  psgsdf_render.h and psgsdf_fit.h say how well the
 * reconstruction explains its photographs; this is their geometric twin.
 *
 * Definition (DESIGN.md "Comparison with a reference"; tests/_compare_ref.py is its executable statement).  All arithmetic in double without
 * contraction except where a float is named; vs is the context's float32 voxel size widened to double; coordinates are in the mesh's units
 * (psgsdf_mesh.h).
 *   Targets: with n_ref_faces > 0 the reference is a triangle set, face f has the corners ref_xyz[ref_faces[f][0..2]]; with n_ref_faces == 0
 *     (ref_faces may be NULL) it is a cloud, target i is the degenerate triangle a = b = c = ref_xyz[i].  The reconstruction's targets are the
 *     faces of the compared mesh.  Queries are always points: the compared mesh's vertices one way (to_reference), all n_ref reference points
 *     the other way (to_reconstruction; also when the reference has faces).
 *   Pair (p, triangle abc): the closest point q by the region walk of Ericson, Real-Time Collision Detection 5.1.5.  A dot product is
 *     (x x' + y y') + z z'.  With ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
 *     d5 = ab.cp, d6 = ac.cp, vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the tests in this order, the first that holds decides:
 *       vertex a   d1 <= 0 and d2 <= 0                          q = a
 *       vertex b   d3 >= 0 and d4 <= d3                         q = b
 *       edge ab    vc <= 0 and d1 >= 0 and d3 <= 0              q = a + ab (d1 / (d1 - d3))
 *       vertex c   d6 >= 0 and d5 <= d6                         q = c
 *       edge ac    vb <= 0 and d2 >= 0 and d6 <= 0              q = a + ac (d2 / (d2 - d6))
 *       edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    q = b + (c - b) ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
 *       interior   denom = 1 / ((va + vb) + vc), v = vb denom, w = vc denom, q = (a + ab v) + ac w
 *     D2 = |p - q|^2 with that dot product.  A vertex region returns the vertex itself, so two faces that share the winning vertex give the same
 *     bits.  A pair whose D2 is not finite (collinear corners met in the interior, a non-finite corner) takes no part.
 *   Nearest: over ALL targets the smallest D2, ties to the smaller target index, so the result does not depend on any traversal order.
 *     d = sqrt(D2).  The query is matched iff d <= max_dist.
 *       matched    dist = (float) d, nearest = that target's index, side = the sign of (p - q) . ((b - a) x (c - a)) as -1 / 0 / +1 (the cross
 *                  product's components are y z' - z y', z x' - x z', x y' - y x').  The welded mesh's winding points outward, so +1 means
 *                  outside.  side is 0 for a cloud target.
 *       unmatched  dist = +inf, nearest = -1, side = 0.
 *     A query with a non-finite coordinate is invalid: dist = NaN, nearest = -1, side = 0, and no part in anything but n.
 *   Per side, with u = d / vs over the matched queries: sum_d = sum llrint(u 2^20), sum_d2 = sum llrint(u u 2^20), sum_signed = sum side
 *     llrint(u 2^20); hist[min(15, (int)(16 d / max_dist))] is incremented; max is the largest d; n_within_tau counts d <= tau; n counts the
 *     queries, n_valid the valid ones, n_matched the matched ones.  mean = vs (sum_d / 2^20) / n_matched, rms = vs sqrt((sum_d2 / 2^20) / n_matched),
 *     mean_signed is formed like mean from sum_signed; all are zero without a match.  The sums are integers, so they are the same bits in
 *     whatever order the device adds them.  The bound max_dist <= 64 vs keeps sum_d2 below 2^63 for 2^31 - 1 queries (u u 2^20 <= 2^32 each).
 *   Scores: precision = to_reference.n_within_tau / to_reference.n_valid, recall the same from to_reconstruction, fscore = 2 P R / (P + R); each
 *     is zero where its denominator is zero.
 *
 * The compared mesh (xyz, normals, rgb, faces) is bit for bit psgsdf_extract_mesh_indexed's (filter == NULL) or psgsdf_extract_mesh_components' kept
 * mesh (filter != NULL).  grid_cell sizes the uniform search grid over the targets; it is acceleration only: no result depends on it.
 * Limits: both sides are sampled at vertices only, so a coarse reference mesh should be passed densely sampled (its large triangles are targets
 * everywhere, but queries only at their corners); single contexts only.
 *
 * Valid once a volume exists; a band is not required.  Two calls on the same state give the same bits, and the call changes no result of any other
 * call.  The arrays are engine-owned pinned host memory, valid until the next extraction call on the context; a later psgsdf_extract_mesh_* call
 * returns what it returned before.  An empty reconstruction or n_ref == 0 is not an error: that side's sizes are 0 and the other side's queries are
 * all unmatched.
 * PSGSDF_ERR_STATE before a volume exists.  PSGSDF_ERR_ARG for a NULL params, out, or ref_xyz with n_ref > 0; n_ref < 0 or > 2^31 - 1, n_ref_faces
 * < 0, or NULL ref_faces with n_ref_faces > 0; a face index outside [0, n_ref) (checked before anything uses it); parameters outside their ranges
 * below, non-zero reserved included; a filter psgsdf_extract_mesh_components refuses.  PSGSDF_ERR_UNSUPPORTED if n_ref_faces or the search grid's
 * entries exceed 2^31 - 1 (a coarse reference with huge triangles: tessellate it).  PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch
 * is refused (everything is freed).  A call that fails its argument checks leaves *out untouched; one that fails later leaves it zeroed.
 * On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_COMPARE_H_
#define PSGSDF_COMPARE_H_

#include "psgsdf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgsdf_compare_params {
    double max_dist;    /* a pair farther apart than this is no match; finite, 0 < max_dist <= 64 vs */
    double tau;         /* threshold of precision / recall; finite, 0 < tau <= max_dist */
    double grid_cell;   /* edge of the search grid's cells, mesh units; 0 = the engine's choice; finite, >= 0.
                           Acceleration only: no result depends on it */
    int32_t reserved[2];/* 0 */
} psgsdf_compare_params;

typedef struct psgsdf_compare_side {      /* one direction */
    int64_t n, n_valid, n_matched, n_within_tau;
    int64_t sum_d, sum_d2, sum_signed;    /* fixed point, units of vs 2^-20 (sum_d2: vs^2 2^-20) */
    int64_t hist[16];
    double max, mean, rms, mean_signed;   /* derived from the integers */
} psgsdf_compare_side;

typedef struct psgsdf_compare {
    /* the reconstruction's mesh that was compared: psgsdf_extract_mesh_indexed's arrays (filter == NULL) or
       psgsdf_extract_mesh_components' kept mesh (filter != NULL), bit for bit */
    const float* xyz; const float* normals; const uint8_t* rgb; const int32_t* faces; int64_t n_vertices, n_faces;
    /* per vertex of that mesh -> the reference */
    const float* vertex_dist; const int32_t* vertex_nearest; const int8_t* vertex_side;
    /* per reference point -> that mesh */
    const float* ref_dist; const int32_t* ref_nearest; const int8_t* ref_side;
    psgsdf_compare_side to_reference, to_reconstruction;
    double precision, recall, fscore;
} psgsdf_compare;

int psgsdf_compare_reference(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter,
                             const float* ref_xyz, int64_t n_ref, const int32_t* ref_faces, int64_t n_ref_faces,
                             const psgsdf_compare_params* params, psgsdf_compare* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_COMPARE_H_ */
