/* psgsdf_fit.h -- how well the reconstruction explains its photographs, per band voxel and per vertex of the welded mesh.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h), like psgsdf_render.h and psgsdf_mesh.h.  psgsdf_render_report answers the question per
 * keyframe; these two calls answer it per place on the surface: how many keyframes saw this spot, and how well the model reproduces what they saw.
 * Neither call changes any result of any other call: a call between two psgsdf_iterate calls leaves the following iterations bit-identical.
 *
 * Definition (DESIGN.md "Photometric fit per voxel and vertex").  For band row j (psgsdf_download_band's order) the loop of the photometric energy
 * (psgsdf_energy) and nothing else: over the set bits of the row's visibility words in ascending frame order, f < n_frames; an observation counts iff
 * the projection of the row's surface point into frame f lies in the image; per counted observation I = the bilinear sample of keyframe f, ren = the
 * model's rendered colour with the row's finite-difference normal and albedo, r[c] = I[c] - ren[c].
 *   n_obs      the number of counted observations;
 *   loss       exactly what the row contributes to the sum behind psgsdf_energy's E_ps: sum over the observations of (sum_c robust_loss(r[c])), the
 *              inner sum in float, the outer one in the engine's observation accumulator (float; double in a PSG_STRICT & 8 build), widened to double:
 *              sum_j loss[j] / n_band is E_ps up to the order of a double summation;
 *   sum_r2[c]  the float sum of r[c] * r[c] in the same order.
 * A row without a counted observation holds zeros.
 *
 * A vertex of the welded mesh (psgsdf_mesh.h) with key 4 * lin + e has the end voxels lin and its +x / +y / +z neighbour (e = 0, 1, 2), or lin alone
 * (a snapped corner, e = 3).  An end voxel that is not a band row contributes nothing.  With n = the sum of the ends' n_obs:
 *   vertex_n_obs = n
 *   vertex_rms   = (float) sqrt((sum over the ends and the three channels of (double) sum_r2) / (3.0 * n))
 *   vertex_loss  = (float) ((loss_lo + loss_hi) / (double) n)
 * in double with IEEE division and square root, no contraction; all three are zero where n == 0.
 *
 * The component filter (psgsdf_extract_mesh_components) and the level-of-detail mesh (psgsdf_extract_mesh_lod) do not carry these attributes.
 *
 * The arrays are engine-owned pinned host memory, valid until the next extraction call (psgsdf_extract_*, psgsdf_band_fit) on the context.
 * Both calls: PSGSDF_ERR_STATE before psgsdf_init (no band: also after psgsdf_upload_volume alone); PSGSDF_ERR_DEVICE if a temporary cannot be
 * allocated; on a context attached to a rank PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and before any device work.
 */
#ifndef PSGSDF_FIT_H_
#define PSGSDF_FIT_H_

#include "psgsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_obs [n_band] int32, loss [n_band] float64, sum_r2 [n_band][3] float32. */
int psgsdf_band_fit(psgsdf_ctx* ctx, const int32_t** n_obs, const double** loss, const float** sum_r2, int64_t* n_band);

/* xyz, normals, rgb, faces: psgsdf_extract_mesh_indexed's arrays bit for bit; vertex_n_obs [n_vertices] int32, vertex_rms and vertex_loss
 * [n_vertices] float32.  An empty mesh: all sizes 0, return 0. */
int psgsdf_extract_mesh_fit(psgsdf_ctx* ctx, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                            const int32_t** faces, int64_t* n_faces,
                            const int32_t** vertex_n_obs, const float** vertex_rms, const float** vertex_loss);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_FIT_H_ */
