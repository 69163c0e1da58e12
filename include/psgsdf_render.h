/* psgsdf_render.h -- view rendering and a per-keyframe photometric report of the engine's current state.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h): the reference has no renderer.  Everything here
 * re-renders the state the engine holds (geometry, albedo, one light per keyframe, poses) with the forward
 * model the energy uses, so that a reconstruction can be compared with the photographs it was fitted to.
 *
 * Semantics (DESIGN.md "View rendering"):
 *   - a ray per pixel from the camera centre through the pixel centre, camera direction ((x-cx)/fx, (y-cy)/fy, 1);
 *   - the grid is a set of cells, one per voxel (the nearest-voxel region, VoxelGrid::world2voxel rounding); only
 *     voxels with weight > 0 take part;  inside the cell of voxel v the distance is phi_v(p) = d_v + g_v.(p - x_v)
 *     with g_v the normalised stored gradient and x_v the voxel centre;
 *   - the hit is the smallest ray parameter at which phi <= 0 inside an observed cell (at the cell's entry point,
 *     or at the linear zero inside it); depth = camera z of the hit;
 *   - shading at the hit uses the hit cell's voxel: inside the surface band the normalised finite-difference normal
 *     and the band albedo (what the energy renders with), outside it the normalised stored gradient and the fused
 *     colour; rendered = albedo x shading (x the LED intensity), residual = keyframe pixel - rendered.
 *
 * Both calls are valid after psgsdf_init.  On a context attached to a rank, psgsdf_render and psgsdf_render_report are collective calls:
 * every rank makes them in the same order with the same arguments (the same view on every rank), and every rank gets the whole planes and stats,
 * bit for bit what a single-rank context holding the same state returns; each rank traces its own slab, the ranks exchange per-pixel hit masks and
 * the winners' records through the context's communicator ("Multi-rank contexts").  Ranks that pass different views all get PSGSDF_ERR_ARG.
 * psgsdf_render_size stays local.
 */
#ifndef PSGSDF_RENDER_H_
#define PSGSDF_RENDER_H_

#include "psgsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* frame >= 0: keyframe `frame` with its current pose, its light and its image (the other fields are ignored).
 * frame < 0 : a caller's camera: pose = 4x4 row-major camera->world (the layout of psgsdf_download_poses), intrinsics
 *             fx fy cx cy, width x height pixels, shaded with the light of keyframe `light_frame`. */
typedef struct psgsdf_view {
    int32_t frame;
    float pose[16];
    float fx, fy, cx, cy;
    int32_t width, height;
    int32_t light_frame;
} psgsdf_view;

/* output planes, in bit order, each [H][W] float32: depth 1 (camera z), normal 3 (world), albedo 3, shading 1,
 * rendered 3, residual 3 (keyframe views only), voxel 1 (linear voxel index as int32 bits).
 * A miss holds 0 in every plane, -1 in the voxel plane. */
enum {
    PSGSDF_R_DEPTH = 1, PSGSDF_R_NORMAL = 2, PSGSDF_R_ALBEDO = 4, PSGSDF_R_SHADING = 8,
    PSGSDF_R_RENDERED = 16, PSGSDF_R_RESIDUAL = 32, PSGSDF_R_VOXEL = 64
};

/* sums over the hit pixels (residuals: keyframe views only, zero otherwise); robust = sum over hit pixels and
 * channels of the context's loss (settings loss / lambda) of the residual.  Summed in one fixed order: reproducible bit for bit. */
typedef struct psgsdf_render_stats {
    int64_t n_pixels, n_hits, n_hits_off_band;
    double sum_r2[3], sum_abs_r[3], robust;
} psgsdf_render_stats;

/* width x height of the planes psgsdf_render writes for `view` (a keyframe view: the keyframes' size) */
int psgsdf_render_size(psgsdf_ctx* ctx, const psgsdf_view* view, int32_t* width, int32_t* height);
/* out_host: the requested planes, [plane][height][width] float32 (may be NULL when channels == 0); stats: nullable. */
int psgsdf_render(psgsdf_ctx* ctx, const psgsdf_view* view, uint32_t channels, float* out_host, psgsdf_render_stats* stats);
/* one row per keyframe ([n_frames]) in one batched pass, no images; row f equals the stats of psgsdf_render on keyframe f bit for bit */
int psgsdf_render_report(psgsdf_ctx* ctx, psgsdf_render_stats* per_keyframe);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_RENDER_H_ */
