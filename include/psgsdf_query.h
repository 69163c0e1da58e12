/* psgsdf_query.h -- the field itself, asked on the device: distance, normal and albedo at the caller's points (psgsdf_query_points), the nearest
 * surface point of each (psgsdf_project_points) and what the caller's rays hit (psgsdf_cast_rays).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  Two models answer: the per-cell first-order model
 * the renderer, the bake, the occlusion and the relighting see (psgsdf_render.h), and the trilinear cell the mesher cuts (psgsdf_mesh.h).
 *
 * Definitions (DESIGN.md 22 "Field queries").  vs is the context's float32 voxel size widened to double.  Positions are in the mesh's units, as
 * psgsdf_occlusion_points takes them: the centre of voxel (i, j, k) is at vs (i, j, k).  The state is what psgsdf_download_volume would return:
 * dist, grad[3], weight, rgb[3]; lin = (k ny + j) nx + i.  m(v) is the stored gradient of v normalised in double as in psgsdf_fill.h:
 * g / sqrt((gx gx + gy gy) + gz gz), and (0, 0, 0) where that sum is not > 0.  All arithmetic in double without contraction, IEEE + - * / sqrt floor
 * in the order written, rounded to float32 only where stated.  Every query is independent of every other.
 *
 *   Model 0, PSGSDF_Q_CELL (the renderer's): u[a] = q[a] / vs + 0.5, c[a] = floor(u[a]); the point is outside unless 0 <= c[a] < dim[a] for every a
 *     (compared as doubles, before any conversion to an integer; a coordinate that is not a number is outside); v is voxel c; the point is
 *     unobserved if weight[v] is not > 0; e[a] = q[a] - vs c[a]; phi = (double) dist[v] + ((m(v)[0] e[0] + m(v)[1] e[1]) + m(v)[2] e[2]); the normal
 *     is m(v), the colour rgb[v], the weight weight[v], the voxel lin(v).
 *   Model 1, PSGSDF_Q_TRILINEAR (the mesher's cell): u[a] = q[a] / vs, b[a] = floor(u[a]), f[a] = u[a] - b[a]; outside unless
 *     0 <= b[a] < dim[a] - 1 for every a; the corners are v_xyz = b + (x, y, z); unobserved if some corner's weight is not > 0;
 *     lerp(A, B, t) = A + t (B - A); for a per-voxel quantity X: X_yz = lerp(X_0yz, X_1yz, f[0]), X_z = lerp(X_0z, X_1z, f[1]),
 *     X = lerp(X_0, X_1, f[2]).  phi is that of (double) dist; S that of m(v) per component, the normal S / sqrt((S0 S0 + S1 S1) + S2 S2), and
 *     (0, 0, 0) where that sum is not > 0; the colour that of rgb, the weight that of weight; the voxel is lin(b).
 *   Status byte of a point or projection: 0 ok, 1 outside the grid, 2 unobserved, 3 one of the caller's floats is not finite, 4 (projection only)
 *     not converged.
 *
 * psgsdf_query_points: xyz [n][3] float32, model 0 or 1.  status [n] uint8; dist [n] = (float) phi; normal [n][3], rgb [n][3], weight [n] the
 *   model's, rounded to float32; voxel [n] int64: lin for status 0, and for status 2 under the cell model, -1 otherwise.  Every float output is 0
 *   unless the status is 0.  counts: n, n_ok, n_outside, n_unobserved, n_invalid.
 *
 * psgsdf_project_points: params { model; max_iters 1 .. 64; tol, mesh units, finite and >= 0; reserved 0 }.  p_0 = (double) q.  For k = 0, 1, ..:
 *   the model at p_k gives status s_k, phi_k and normal n_k; stop at the first of: s_k != 0 (status s_k), |phi_k| <= tol (status 0),
 *   k == max_iters (status 4); otherwise p_{k+1}[a] = p_k[a] - phi_k n_k[a].  status [n]: at the stop; xyz [n][3] = (float) p_k at the stop;
 *   residual [n] = (float) phi_k if s_k == 0, else 0; normal [n][3]: of the last evaluation, 0 if s_k != 0; voxel [n]: as above, at the last
 *   evaluation; iterations [n] uint8 = k, the moves made; distance [n] = (float)(sg sqrt((dx dx + dy dy) + dz dz)) with d = p_k - p_0, sg = -1 if
 *   phi_0 < 0 and +1 otherwise.  A point with status 3, or with s_0 != 0, keeps its input position; its iterations and distance are 0.
 *   counts: n, n_converged, n_left (status 1 or 2), n_not_converged, n_invalid.
 *   What prototyping showed: the cell model is discontinuous across cell walls, so a point can hop between two cells for ever, and status 4 is then
 *   the honest answer (10 of 4000 points near a sphere of radius 10 voxels at tol 1e-3 voxel); the trilinear model converged in at most 3 moves on
 *   every test point.
 *
 * psgsdf_cast_rays: params { t_min, finite and >= 0; t_max > t_min, +infinity allowed }.  For ray j, o is the origin and w the direction, widened
 *   and divided by its length sqrt((x x + y y) + z z); the ray is invalid (status 3) when one of its six floats is not finite or that length is
 *   zero (the rule of psgsdf_occlusion_points).  o' = o + t_min w; in the renderer's coordinates uo[a] = (float)(o'[a] / vs + 0.5),
 *   uw[a] = (float)(w[a] / vs); the walk is the renderer's (psgsdf_render.h), cut at (float)(t_max - t_min) (no cut if t_max is infinite).  The
 *   ray hits iff the walk finds a hit with (double) t <= t_max - t_min.  status [n]: 0 hit, 1 miss, 2 buried (a hit with t == 0: the shifted
 *   origin is already at or below some cell's model; it counts as a hit), 3 invalid.  With T = (double) t + t_min: t [n] = (float) T,
 *   xyz [n][3] = (float)(o[a] + T w[a]), normal [n][3] = (float) m(voxel), rgb [n][3] = rgb[voxel], voxel [n] int64 the hit cell, -1 otherwise.
 *   Float outputs are 0 on a miss or an invalid ray.  counts: n, n_valid, n_hits (buried ones included), n_buried.  Cells with weight 0 never stop
 *   a ray, as everywhere else.
 *
 * Valid once a volume exists; no band is needed.  No call changes the context's state or the result of any other call: a call between two
 * psgsdf_iterate calls leaves the following iterations bit-identical.  Two calls on the same state give the same bits.  The arrays are engine-owned
 * pinned host memory, valid until the next extraction call on the context.  The caller's order is kept; the number of queries is bounded by memory
 * alone (they go out in launches of at most 2^30; PSGSDF_QUERY_CHUNK, a multiple of 64, lets a test send a small call through several launches).
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for n < 0, a NULL pointer, a bad parameter or reserved != 0; PSGSDF_ERR_DEVICE if memory
 * cannot be allocated or a launch is refused (everything is freed); PSGSDF_ERR_UNSUPPORTED on a context attached to a rank: at once, on the calling
 * rank alone, before any exchange and device work.  A call that fails its argument checks leaves the caller's outputs untouched; one that fails
 * later leaves the pointers NULL and the counts zero.  n == 0 returns 0 with empty arrays.
 */
#ifndef PSGSDF_QUERY_H_
#define PSGSDF_QUERY_H_

#include "psgsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PSGSDF_Q_CELL 0
#define PSGSDF_Q_TRILINEAR 1

#define PSGSDF_Q_OK 0
#define PSGSDF_Q_OUTSIDE 1
#define PSGSDF_Q_UNOBSERVED 2
#define PSGSDF_Q_INVALID 3
#define PSGSDF_Q_NOT_CONVERGED 4

#define PSGSDF_RAY_HIT 0
#define PSGSDF_RAY_MISS 1
#define PSGSDF_RAY_BURIED 2
#define PSGSDF_RAY_INVALID 3

typedef struct psgsdf_query_counts {
    int64_t n, n_ok, n_outside, n_unobserved, n_invalid;
} psgsdf_query_counts;

int psgsdf_query_points(psgsdf_ctx* ctx, const float* xyz, int64_t n, int32_t model,
                        const uint8_t** status, const float** dist, const float** normal, const float** rgb, const float** weight, const int64_t** voxel,
                        psgsdf_query_counts* counts);

typedef struct psgsdf_project_params {
    int32_t model;                 /* PSGSDF_Q_CELL or PSGSDF_Q_TRILINEAR */
    int32_t max_iters;             /* 1 .. 64 */
    double tol;                    /* mesh units, finite, >= 0 */
    double reserved;               /* 0 */
} psgsdf_project_params;

typedef struct psgsdf_project_counts {
    int64_t n, n_converged, n_left, n_not_converged, n_invalid;      /* n_left: status 1 or 2 */
} psgsdf_project_counts;

int psgsdf_project_points(psgsdf_ctx* ctx, const float* xyz, int64_t n, const psgsdf_project_params* params,
                          const uint8_t** status, const float** out_xyz, const float** residual, const float** normal, const int64_t** voxel,
                          const uint8_t** iterations, const float** distance, psgsdf_project_counts* counts);

typedef struct psgsdf_ray_params {
    double t_min;                  /* finite, >= 0 */
    double t_max;                  /* > t_min; +infinity allowed */
} psgsdf_ray_params;

typedef struct psgsdf_ray_counts {
    int64_t n, n_valid, n_hits, n_buried;      /* a buried ray is also a hit */
} psgsdf_ray_counts;

int psgsdf_cast_rays(psgsdf_ctx* ctx, const float* origins, const float* directions, int64_t n, const psgsdf_ray_params* params,
                     const uint8_t** status, const float** t, const float** xyz, const float** normal, const float** rgb, const int64_t** voxel,
                     psgsdf_ray_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_QUERY_H_ */
