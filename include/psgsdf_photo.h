/* psgsdf_photo.h -- an albedo texture of the level-of-detail mesh solved from the keyframes themselves, at texel resolution, on the device.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  The albedo map of psgsdf_bake_lod is the albedo of
 * the voxel a texel's ray hits: it can never be sharper than one voxel, while the photographs usually are.  This call solves, for every texel of the
 * bake's atlas, the albedo that best explains the keyframes that actually see that spot: the shading of the engine's own model under the current
 * poses and lights, the engine's own robust weights, and one ray through the reconstruction per (texel, keyframe) pair to decide visibility.  It is
 * one reweighting step of the energy's albedo update at texel resolution instead of voxel resolution.
 *
 * Definition (DESIGN.md "Photometric albedo texture").  All arithmetic in double without contraction except where a float is named; vs is the
 * context's float32 voxel size widened to double, origin is psgsdf_info.origin (float32), positions are in the mesh's units (psgsdf_mesh.h): the
 * mesh frame is the world frame minus the grid origin.
 *   Parameters: bias, the lift of the visibility ray's origin off the surface in mesh units, finite and > 0; cos_min, finite, -1 <= cos_min < 1;
 *     shade_min, finite and > 0; want_status 0 or 1; reserved 0.
 *   The sample of a texel exists for an owned texel whose voxel >= 0 (a hit of the bake).  With p and n as in psgsdf_bake.h, from the bake's public
 *     planes (as psgsdf_bake_lod_ao defines its own): q = p + (double) displacement n; m = the texel's float normal from the bake's normal plane,
 *     widened and divided by its length sqrt((x^2 + y^2) + z^2) (m = n if that length is zero); a0[c] = albedo byte / 255.0.  World point
 *     xw[k] = q[k] + (double) origin[k], xs[k] = (float) xw[k].
 *   Every other texel (missed, buried, padding) is PSGSDF_PHOTO_NO_SAMPLE for every frame: photo = (float)(albedo byte / 255.0), photo_rgb = that
 *     byte, n_obs = 0; padding stays all zero.
 *   Per keyframe f = 0 .. n_frames - 1, with its current pose R, t and its current light; the first step that fails gives the status:
 *     1. OUTSIDE.  pr = the energy's projection of xs into frame f in its float arithmetic (p = R^T (xs - t), z_inv = 1 / p[2],
 *        (m, n) = (fx p[0] z_inv + cx, fy p[1] z_inv + cy), ok = 0 <= m < W and 0 <= n < H).  OUTSIDE unless p[2] > 0 and ok.
 *     2. GRAZING.  wc = (t - xw) / |t - xw|, cosv = (m[0] wc[0] + m[1] wc[1]) + m[2] wc[2].  GRAZING unless cosv > cos_min.
 *     3. OCCLUDED.  psgsdf_relight's ray towards a point light at the camera centre with one sample, spread 0 and no reach: o = q + bias m,
 *        d = ((double) t - (double) origin) - o, len = |d|, w = d / len; in the renderer's coordinates uo[k] = (float)(o[k] / vs + 0.5),
 *        uw[k] = (float)(w[k] / vs).  OCCLUDED iff the walk returns a hit with (double) t_hit <= len; a hit with t_hit == 0 is also counted in
 *        n_buried.  len == 0: not occluded.
 *     4. DARK.  s[c] = the forward model's rendered intensity of frame f at pr for the texel's float normal as stored in the plane, its SH basis and
 *        albedo (1, 1, 1), in float exactly as the forward model sums it.  DARK unless s[c] >= (float) shade_min in all three channels.
 *     5. USED.  I = the energy's bilinear sample of keyframe f at (pr.m, pr.n), border rule included; r[c] = I[c] - (float) a0[c] * s[c] in float;
 *        wgt[c] = the robust weight of r[c] under the context's loss and lambda; num[c] += (double) wgt[c] * (double) s[c] * (double) I[c];
 *        den[c] += (double) wgt[c] * (double) s[c] * (double) s[c].  Both sums run over the frames in ascending order.
 *   Result: n_obs = the number of USED frames; photo[c] = (float)(num[c] / den[c]) where n_obs > 0 and den[c] > 0, otherwise (float) a0[c];
 *     photo_rgb[c] = floor(255 clamp(photo[c], 0, 1) + 0.5) in float.  A texel counts in n_texels_solved when n_obs > 0.
 *     n_pairs = n_samples n_frames = n_used + n_outside + n_grazing + n_occluded + n_dark.
 *
 * Limits: one reweighting step from the voxel albedo, not a converged IRLS; hard visibility, one ray per pair; no inter-reflection and no specular
 * term; the seams between atlas blocks bleed under bilinear filtering, as in the bake.
 *
 * Valid after psgsdf_init: it needs the keyframes, their images and lights.  Two calls on the same state give the same bits; a call between two
 * psgsdf_iterate calls leaves the later iterations bit-identical.  out->bake is bit for bit what psgsdf_bake_lod returns for the same arguments,
 * and a later psgsdf_extract_* or psgsdf_bake_lod* call returns what it returned before.  The arrays are engine-owned pinned host memory, valid
 * until the next extraction call on the context.  An empty level-of-detail mesh: all sizes 0 (n_frames is still set), return 0.
 * PSGSDF_ERR_ARG for a NULL pointer, a broken rule of the params and anything psgsdf_bake_lod refuses that way (the outputs stay untouched);
 * PSGSDF_ERR_STATE before psgsdf_init, also after psgsdf_upload_volume alone; PSGSDF_ERR_UNSUPPORTED for what psgsdf_bake_lod refuses that way and
 * for want_status with n_frames H W > 2^30; PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused (everything is freed, *out is
 * zeroed).  On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_PHOTO_H_
#define PSGSDF_PHOTO_H_

#include "psgsdf_bake.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgsdf_photo_params {
    double bias;                   /* lift of the visibility ray's origin off the surface, mesh units: finite, > 0 */
    double cos_min;                /* a keyframe counts only if (normal . direction to its camera) > cos_min: finite, -1 <= cos_min < 1 */
    double shade_min;              /* ... and only if the model's shading is >= shade_min in all three channels: finite, > 0 */
    int32_t want_status, reserved; /* want_status 0 / 1; reserved 0 */
} psgsdf_photo_params;

enum { PSGSDF_PHOTO_USED = 0, PSGSDF_PHOTO_OUTSIDE = 1, PSGSDF_PHOTO_GRAZING = 2, PSGSDF_PHOTO_OCCLUDED = 3, PSGSDF_PHOTO_DARK = 4,
       PSGSDF_PHOTO_NO_SAMPLE = 255 };

typedef struct psgsdf_photo_counts {
    int64_t n_samples, n_pairs, n_used, n_outside, n_grazing, n_occluded, n_buried, n_dark, n_texels_solved;
} psgsdf_photo_counts;

typedef struct psgsdf_bake_photo {
    psgsdf_bake bake;              /* psgsdf_bake_lod's result for the same arguments, bit for bit */
    const float* photo;            /* [H][W][3] the solved albedo, unclamped */
    const uint8_t* photo_rgb;      /* [H][W][3] floor(255 clamp(photo, 0, 1) + 0.5) */
    const int32_t* n_obs;          /* [H][W] keyframes used */
    const uint8_t* status;         /* [n_frames][H][W], NULL unless want_status */
    int32_t n_frames, reserved;
    psgsdf_photo_counts counts;
} psgsdf_bake_photo;

int psgsdf_bake_lod_photo(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach,
                          const psgsdf_photo_params* params, psgsdf_bake_photo* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_PHOTO_H_ */
