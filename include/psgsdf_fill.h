/* psgsdf_fill.h -- unobserved voxels filled on the device, and the welded mesh of the filled state: the filled voxels themselves
 * (psgsdf_fill_voxels) and psgsdf_extract_mesh_components' mesh and component list with the holes closed (psgsdf_extract_mesh_filled).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  psgsdf_extract_mesh_indexed keeps a cell only if
 * all eight corners have weight > 0, so every patch the depth camera never saw is a hole.  A Gradient-SDF stores a distance and a unit gradient
 * per voxel, and its first-order extension into a neighbouring voxel is the model the renderer already uses inside a cell (psgsdf_render.h): the
 * filling is a front propagation of that model plus a few relaxation sweeps.
 *
 * What it is not.  It closes gaps up to about 2 R voxels wide, and nothing wider.  It also extends the field R voxels beyond the observed band
 * everywhere, and a large R can create spurious sheets where the extensions of unrelated surfaces meet.  R and K are the caller's choice.
 *
 * Definition (DESIGN.md "Hole filling").  All arithmetic is in double, without FMA contraction, with IEEE + - * / sqrt, in exactly the order
 * written, and rounded to float32 where stated.
 *   The state is what psgsdf_download_volume would return at the time of the call: dist, grad (3 planes), weight, rgb (3 planes).
 *   h is the context's float32 voxel size, widened.
 *   Linear index: lin = (k ny + j) nx + i.
 *   The six neighbours of a voxel, in this fixed order: -x, +x, -y, +y, -z, +z.  A neighbour outside the grid does not exist.
 *   m(v) is the stored gradient of v normalised in double: g / sqrt((gx gx + gy gy) + gz gz), and (0, 0, 0) where that sum is not > 0.
 *   Every sum below starts from 0 and takes its terms in the neighbour order.
 * Parameters.  rounds R with 0 <= R <= 255, sweeps K with 0 <= K <= 4096.
 * Known set.  Known_0 = {weight > 0}.
 * Front rounds, r = 1 .. R.  Every voxel u outside Known_{r-1} with at least one neighbour in Known_{r-1} joins Known_r with round[u] = r.  Its
 *   values come from those neighbours only, as they stood at the END of round r - 1.  With n such neighbours v = u + s e_a:
 *     dist[u]   = (float)( sum( (double) dist[v] - (s h) m(v)[a] ) / n )
 *     grad[u]   = (float) of S / sqrt((Sx Sx + Sy Sy) + Sz Sz), S = sum m(v), and (0, 0, 0) where that sum of squares is not > 0
 *     rgb[u][c] = (float)( sum (double) rgb[v][c] / n )
 *   Filled = Known_R \ Known_0.
 * Relaxation, K Jacobi sweeps.  In each sweep every filled voxel is replaced from the PREVIOUS sweep's values of its neighbours in Known_R
 *   (a filled voxel always has one); observed voxels never change:
 *     dist = (float)( sum (double) dist[v] / n ),  grad = (float) of the normalised sum of m(v) as above,  rgb[c] = (float)( sum (double) rgb[v][c] / n )
 * Filled state.  The state with those values at the filled voxels and weight = 1.0f there.  Every other voxel is bit for bit as before.
 * With R = 0 nothing is filled and every result equals its unfilled counterpart bit for bit.
 *
 * psgsdf_fill_voxels: the filled voxels in ascending lin; no filled voxel: *n_filled = 0, NULL arrays, return 0.
 * psgsdf_extract_mesh_filled: psgsdf_extract_mesh_components' definition and outputs (psgsdf_mesh.h), applied to the filled state -- the crop box,
 *   and with it the cells, keys and faces, is the filled distances' -- plus vertex_filled.  One thing is taken from the UNFILLED state: the vertex frame.
 *   A crop voxel's position is (q - lo) voxel - origin with voxel = (vs d) / d and origin = -vs lo in float32 (q the voxel's grid index), and lo, d
 *   here are the first voxel and the extent of the UNFILLED state's crop box whenever it has one (else the filled state's).  Filling can move the crop
 *   box, and from another corner the same point rounds differently; in the unfilled frame a vertex between two unfilled voxels has the position,
 *   normal and colour it has in psgsdf_extract_mesh_indexed's mesh of the state, bit for bit, and the unfilled mesh's vertices appear in their order.
 *   Against the filled box's own frame a coordinate differs by float32 rounding only.  With the same crop box, R = 0 included, nothing differs.
 *   A vertex with key 4 lin + e has the end voxels lin and its +x / +y / +z neighbour (e = 0, 1, 2), or lin alone (a snapped corner, e = 3);
 *   vertex_filled is the number of its end voxels that are filled: 0, 1 or 2, for a snapped corner 0 or 2.
 *
 * Valid once a volume exists; a band is not required.  No call changes the context's state or a result of any other call: a call between two
 * psgsdf_iterate calls leaves the following iterations bit-identical, and two calls on the same state give the same bits.  The arrays are
 * engine-owned pinned host memory, valid until the next extraction call on the context.
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for rounds or sweeps out of range, a NULL pointer, a filter with a NaN min_area or
 * keep_largest < 0; PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused (everything is freed).  A call that fails its argument
 * checks leaves the caller's outputs untouched; one that fails later leaves the pointers NULL and the counts 0.  On a context attached to a rank:
 * PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 * Device memory of a call: a working copy of the eight float planes and one byte per voxel, per filled voxel 89 B (113 B in psgsdf_fill_voxels), and
 * what psgsdf_extract_mesh_components takes for the mesh.
 */
#ifndef PSGSDF_FILL_H_
#define PSGSDF_FILL_H_

#include "psgsdf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PSGSDF_FILL_MAX_ROUNDS 255
#define PSGSDF_FILL_MAX_SWEEPS 4096

/* lin [n] int64 ascending, dist [n], grad [n][3], rgb [n][3] float32, round [n] uint8 (1 .. rounds). */
int psgsdf_fill_voxels(psgsdf_ctx* ctx, int32_t rounds, int32_t sweeps,
                       const int64_t** lin, const float** dist, const float** grad, const float** rgb, const uint8_t** round, int64_t* n_filled);

/* the nine outputs of psgsdf_extract_mesh_components, then vertex_filled [n_vertices] uint8.  An empty mesh: all sizes 0, return 0. */
int psgsdf_extract_mesh_filled(psgsdf_ctx* ctx, int32_t rounds, int32_t sweeps, const psgsdf_mesh_filter* filter,
                               const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                               const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component,
                               const psgsdf_mesh_component** components, int64_t* n_components, const uint8_t** vertex_filled);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_FILL_H_ */
