/* psgsdf_occlusion.h -- ambient occlusion of the reconstructed surface, computed on the device by short rays through the volume: at points and
 * normals of the caller's (psgsdf_occlusion_points) and as a fourth map of the bake onto the level-of-detail mesh (psgsdf_bake_lod_ao).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  The photometric model has no self-occlusion term,
 * so neither has the albedo the engine recovers; the occlusion of the reconstructed surface with its sub-voxel detail cannot be recomputed from the
 * coarse mesh downstream.  Every ray runs through the renderer's own cell walk and first-order surface model (psgsdf_render.h, psgsdf_bake.h).
 *
 * Definition (DESIGN.md "Ambient occlusion").  All arithmetic in double without contraction except where a float is named; vs is the context's
 * float32 voxel size widened to double; positions are in the mesh's units (psgsdf_mesh.h).
 *   Parameters: n_dirs (K) one of 8, 16, 32, 64; radius and bias lengths in mesh units, finite and > 0; reserved 0.
 *   Direction table dirs [K][3], computed once per call on the host and returned to the caller: for i = 0 .. K - 1, u = (i + 0.5) / K, r = sqrt(u),
 *     z = sqrt(1 - u), phi = 2 pi (i g - floor(i g)) with g = 0.6180339887498949, D_i = (r cos phi, r sin phi, z): cosine-weighted, every ray has
 *     weight 1 / K.
 *   Frame of a unit normal m: sg = copysign(1, m[2]), a = -1 / (sg + m[2]), b = m[0] m[1] a, t1 = (1 + sg m[0] m[0] a, sg b, -sg m[0]),
 *     t2 = (b, sg + m[1] m[1] a, -m[1]).
 *   Ray i of a sample (q, m): origin o = q + bias m, direction w = (D_i[0] t1 + D_i[1] t2) + D_i[2] m; in the renderer's coordinates
 *     uo[k] = (float)(o[k] / vs + 0.5), uw[k] = (float)(w[k] / vs), so the ray parameter t is a length in mesh units.  The ray is occluded iff the
 *     walk finds a hit with (double) t <= radius; it is buried iff the hit has t == 0 (the origin is already at or below some cell's surface model):
 *     a buried ray counts as occluded and is also counted separately.
 *   Per sample: mask, a uint64 with bit i set iff ray i is occluded (bits >= K zero), and with c = popcount(mask) the byte
 *     occlusion = (510 (K - c) + K) / (2 K) in integer arithmetic = floor(255 (K - c) / K + 1/2); 255 means open.
 *   An invalid sample has mask 0 and byte 255 and takes no part in n_valid, n_rays, n_occluded and n_buried.  n_rays = K n_valid.
 *
 * psgsdf_occlusion_points: sample j is q = xyz[j], m = normals[j] divided by its length sqrt((x^2 + y^2) + z^2); it is invalid when one of its six
 *   floats is not finite or that length is zero.  n == 0 returns 0 with empty arrays (dirs is still filled).
 * psgsdf_bake_lod_ao: out->bake is bit for bit what psgsdf_bake_lod returns for the same arguments.  The sample of an owned texel is defined from
 *   the bake's public planes, with p and n as in psgsdf_bake.h: a hit texel (voxel >= 0) has q = p + (double) displacement n and m = the texel's
 *   float normal widened and normalised as above (m = n if its length is zero); a missed or buried texel has q = p, m = n; an owned texel without a
 *   ray (n is zero) is invalid.  Padding: byte 0, mask 0.  counts.n_samples is the number of owned texels.
 *
 * Limits: the direction set is the same for every sample (no per-sample rotation), so the error is structured, not noisy.  The surface model is
 * discontinuous across cell walls: with a small bias a neighbouring cell's model can bury an origin on a convex surface (DESIGN.md has figures).
 * Cells with weight 0 never occlude.
 *
 * Valid once a volume exists; a band is not required (only dist, grad and weight are read).  Two calls on the same state give the same bits.  The
 * arrays are engine-owned pinned host memory, valid until the next extraction call on the context; a later psgsdf_bake_lod or
 * psgsdf_extract_mesh_* call returns what it returned before.
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for bad parameters, n < 0 or a NULL pointer, and for anything psgsdf_bake_lod refuses
 * that way; PSGSDF_ERR_UNSUPPORTED for what psgsdf_bake_lod refuses that way; PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused
 * (everything is freed).  The number of rays is bounded by memory alone: they are launched in chunks of 2^30.  A call that fails its argument
 * checks leaves the caller's outputs untouched, as psgsdf_bake_lod does; one that fails later leaves the pointers NULL and the structs zeroed.
 * On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_OCCLUSION_H_
#define PSGSDF_OCCLUSION_H_

#include "psgsdf_bake.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgsdf_ao_params {
    int32_t n_dirs;                /* K: 8, 16, 32 or 64 */
    int32_t reserved;              /* 0 */
    double radius;                 /* a ray occludes up to this length */
    double bias;                   /* the origin's offset along the normal */
} psgsdf_ao_params;

typedef struct psgsdf_ao_counts {
    int64_t n_samples, n_valid, n_rays, n_occluded, n_buried;      /* n_rays = n_dirs n_valid; n_occluded and n_buried count rays */
} psgsdf_ao_counts;

int psgsdf_occlusion_points(psgsdf_ctx* ctx, const float* xyz, const float* normals, int64_t n, const psgsdf_ao_params* params,
                            const uint64_t** mask, const uint8_t** occlusion, const double** dirs, psgsdf_ao_counts* counts);

typedef struct psgsdf_bake_ao {
    psgsdf_bake bake;              /* psgsdf_bake_lod's result */
    const uint8_t* occlusion;      /* [H][W] */
    const uint64_t* mask;          /* [H][W] */
    const double* dirs;            /* [n_dirs][3] */
    int32_t n_dirs, reserved;
    psgsdf_ao_counts counts;
} psgsdf_bake_ao;

int psgsdf_bake_lod_ao(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, const psgsdf_ao_params* params,
                       psgsdf_bake_ao* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_OCCLUSION_H_ */
