/* psgsdf_relight.h -- one view of the reconstruction under lights of the caller's, with the shadows the reconstructed surface casts on itself,
 * computed on the device by rays through the volume (psgsdf_relight).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has no renderer.  psgsdf_render shades a view with the light the engine
 * estimated for one keyframe, and the forward model has no self-occlusion term.  Here the primary hit of every pixel is found once, by psgsdf_render's
 * own kernel, and every light then gets its own shadow rays from the hit points through the renderer's cell walk and first-order surface model
 * (psgsdf_render.h, psgsdf_occlusion.h): a `visibility` and a `rendered` plane per light.
 *
 * Definition.  All arithmetic in double without contraction except where a float is named; vs is the context's float32 voxel size
 * widened to double, origin is psgsdf_info.origin widened; unit(v) = v / sqrt((v0^2 + v1^2) + v2^2); a . b = (a0 b0 + a1 b1) + a2 b2.
 *   Primary hit: depth t, voxel, normal and albedo of a pixel are bit for bit psgsdf_render's planes for the same view (light_frame is ignored); a
 *     miss is 0 in every output plane (geometry: psgsdf_render's miss, voxel -1).  The pixel's ray direction is the renderer's
 *     w = R dc in float, w[k] = (R[k][0] dc[0] + R[k][1] dc[1]) + R[k][2] dc[2] without contraction, dc = (((float) x - cx) / fx, ((float) y - cy) / fy, 1);
 *     the hit point q[k] = (double) pose_t[k] + (double) t (double) w[k]; m is the
 *     float normal widened, m = unit(m).  A normal of length zero leaves the pixel unlit.
 *   SH light: irr = sum_i sh[i] b_i(n) in float on the float normal n, b the engine's basis 1, nx, ny, nz (n_sh 4) and nx ny, nx nz, ny nz,
 *     nx^2 - ny^2, nx^2 - nz^2 (n_sh 9), summed as the forward model sums it.  No rays; visibility 1 on every hit; n_lit = n_hits, n_rays = 0.
 *   Directional and point lights: the centre direction wc = unit(vec) (directional) or unit(L - q) with L = vec (point); cosv = m . wc;
 *     fall = 1 (directional) or 1 / r2 with r2 = ((L0 - q0)^2 + (L1 - q1)^2) + (L2 - q2)^2 (point).  A hit with cosv <= 0, or a point light with
 *     r2 = 0, is unlit: visibility 0, no rays.  Otherwise the pixel is lit and sends K = n_shadow rays from o = q + bias m.
 *   Shadow rays: (t1, t2) is the frame of wc by psgsdf_occlusion.h's formula; (a_i, b_i) are the first two components of its direction table D_i for
 *     K >= 8 (the uniform disc), (0, 0) for K = 1.  With e_i = a_i t1 + b_i t2:
 *       directional: w_i = unit(wc + spread e_i), limit_i = reach, or infinity when reach is 0;
 *       point: the target T_i = L + spread e_i, d_i = T_i - o, len_i = sqrt((d_i0^2 + d_i1^2) + d_i2^2), w_i = d_i / len_i,
 *         limit_i = min(reach or infinity, len_i): an occluder behind the light casts no shadow; len_i = 0: not occluded.
 *     In the renderer's coordinates uo[k] = (float)((o[k] - origin[k]) / vs + 0.5), uw[k] = (float)(w_i[k] / vs): the ray parameter is a length in
 *     world units.  The ray is occluded iff the walk finds a hit with (double) t <= limit_i; it is buried iff that hit has t == 0 (counted as
 *     occluded, and separately).  With c the occluded rays of the pixel, visibility = (float)(K - c) / (float) K.
 *   Rendered, on a hit pixel: rendered[ch] = (float)((double) albedo[ch] * ((double) ambient[ch] + (double) colour[ch] * s)) with s = (double) irr
 *     (SH), s = (cosv * fall) * (double) visibility (lit), s = 0 (unlit).
 *   Hence an SH light holding keyframe f's light (psgsdf_download_light) with colour 1 and ambient 0, on keyframe f's view of an SH context, gives
 *     psgsdf_render's `rendered` plane bit for bit.
 *   Counts per light: n_hits (hit pixels), n_lit (lit pixels), n_rays = K n_lit, n_occluded and n_buried (rays).
 *
 * Limits: shadows are hard per ray; the sample table is the same for every pixel, so the error of a soft shadow is structured, not noisy.  The
 * surface model is discontinuous across cell walls (see DESIGN.md 15 on the bias).  Cells with weight 0 never shadow.  No inter-reflections.
 *
 * Valid after psgsdf_init, where psgsdf_render is.  Two calls on the same state give the same bits; the engine's state is not disturbed.
 * PSGSDF_ERR_ARG for a NULL pointer, a view psgsdf_render refuses, or a broken rule of the structs below (the outputs are untouched);
 * PSGSDF_ERR_STATE before psgsdf_init; PSGSDF_ERR_UNSUPPORTED for a view of more than 2^24 pixels, and on a context attached to a rank (on every
 * rank, at once, before any exchange and device work); PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused (everything is freed).
 */
#ifndef PSGSDF_RELIGHT_H_
#define PSGSDF_RELIGHT_H_

#include "psgsdf_render.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PSGSDF_LIGHT_SH = 0, PSGSDF_LIGHT_DIRECTIONAL = 1, PSGSDF_LIGHT_POINT = 2 };
enum { PSGSDF_RELIGHT_MAX_LIGHTS = 64 };

typedef struct psgsdf_light {
    int32_t kind;
    int32_t n_sh;                  /* SH: 4 or 9, else 0 */
    float sh[9];                   /* SH: the coefficients in the engine's basis of the world normal (finite) */
    float vec[3];                  /* DIRECTIONAL: direction from the surface towards the light (finite, any length > 0); POINT: position; the world frame of the poses */
    float colour[3], ambient[3];   /* finite, >= 0 */
    float spread;                  /* DIRECTIONAL: tangent of the light's angular radius; POINT: radius of the light's disc, world units; finite, >= 0 (SH: 0) */
    int32_t n_shadow;              /* K: 1, 8, 16, 32 or 64 (SH: 0); spread > 0 needs K >= 8 */
} psgsdf_light;

typedef struct psgsdf_relight_params {
    double bias;                   /* the shadow rays' origin is lifted off the hit by this length along the normal: finite, > 0 */
    double reach;                  /* a ray occludes up to this length: finite, >= 0; 0: no limit (the walk ends where the ray leaves the occupied bricks' box) */
    int32_t n_lights;              /* 1 .. 64 */
    int32_t reserved;              /* 0 */
} psgsdf_relight_params;

typedef struct psgsdf_relight_counts {
    int64_t n_hits, n_lit, n_rays, n_occluded, n_buried;
} psgsdf_relight_counts;

/* view: as psgsdf_render takes it (the planes' size: psgsdf_render_size).
 * out_host: [n_lights][4][H][W] float32: rendered r g b, visibility.
 * geometry_host (nullable): [8][H][W] float32: depth, normal 3, albedo 3, voxel (int32 bits).  per_light (nullable): [n_lights]. */
int psgsdf_relight(psgsdf_ctx* ctx, const psgsdf_view* view, const psgsdf_light* lights, const psgsdf_relight_params* params,
                   float* out_host, float* geometry_host, psgsdf_relight_counts* per_light);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_RELIGHT_H_ */
