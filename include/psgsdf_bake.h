/* psgsdf_bake.h -- albedo, normal and displacement maps of the reconstruction, baked onto the level-of-detail mesh on the device.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  psgsdf_extract_mesh_lod makes the surface small by
 * averaging its detail away; this call keeps the detail in a texture atlas: one texel is one short ray from the coarse triangle onto the
 * reconstructed surface, through the renderer's own cell walk and first-order surface model (psgsdf_render.h).
 *
 * Definition (DESIGN.md "Baked detail maps"):
 *   Input mesh: exactly what psgsdf_extract_mesh_lod(ctx, filter, cell) returns: xyz, normals, rgb, faces with V vertices and F faces.
 *   Parameters: res (R) an int32 >= 1; reach a double in mesh units, finite and > 0; vs the context's float32 voxel size widened to double.
 *   Atlas layout, pure integer arithmetic: B = R + 1, nblk = (F + 1) / 2, bpr the smallest integer with bpr^2 >= nblk, W = bpr B,
 *     H = ceil(nblk / bpr) B; W or H above 16384: PSGSDF_ERR_UNSUPPORTED.  Face f lives in block q = f >> 1, at block column q % bpr and block row
 *     q / bpr.  Texel (X, Y) has local (i, j) = (X mod B, Y mod B); row 0 is the top row of the image.  The even face of a block owns the texels
 *     with i + j <= R, with (a, b) = (i, j); the odd face owns those with i + j >= R + 1, with (a, b) = (R - i, R - j).  The texels of a missing odd
 *     face (the last block when F is odd) and of blocks beyond nblk are padding.
 *   Sample, in double without contraction: w1 = (3a + 1) / (3 (R + 1)), w2 = (3b + 1) / (3 (R + 1)), w0 = 1 - w1 - w2 (all strictly inside the
 *     triangle); p = (w0 x0 + w1 x1) + w2 x2; n = (w0 n0 + w1 n1) + w2 n2 divided by its length sqrt((nx^2 + ny^2) + nz^2).  If that length is zero,
 *     n = (x1 - x0) x (x2 - x0) divided by its length; if that is zero as well the texel is a miss with normal (0, 0, 0).
 *   Ray: origin o = p + reach n, direction -n; in the renderer's coordinates uo[k] = (float)(o[k] / vs + 0.5), uw[k] = (float)(-n[k] / vs), so the
 *     ray parameter t is a length in mesh units.  The walk is the renderer's: the same occupied-brick map, cells, crossings and surface model.
 *   Hit: the walk returns t with 0 < t <= 2 reach.  Buried: t == 0 (the origin itself is at or below the surface): treated as a miss, counted
 *     separately.  Anything else is a miss.
 *   A hit texel: voxel = the hit cell's linear index; displacement = (float)(reach - t), positive where the surface lies outside the coarse
 *     triangle; normal and albedo are what psgsdf_render gathers for a hit: of a band voxel the band's finite-difference normal and albedo, otherwise
 *     the normalised stored gradient and the fused colour (counted in n_hits_off_band); albedo byte = floor(255 clamp(c, 0, 1) + 0.5).
 *   A missed or buried texel: voxel = -1, displacement 0, normal = the ray's n as float, albedo bytes = floor((w0 c0 + w1 c1) + w2 c2 + 0.5) of the
 *     three vertices' bytes, in double.
 *   Padding: all zero, voxel = -1, face = -1.
 *   Texture coordinates uv [F][3][2]: u = x / W, v = y / H with y pointing down, the affine continuation of the texel centres (i + 0.5 <-> a): the
 *     corners of an even face at local (1/6, 1/6), (R + 7/6, 1/6), (1/6, R + 7/6), of an odd face at (R + 5/6, R + 5/6), (-1/6, R + 5/6),
 *     (R + 5/6, -1/6); each coordinate is (float)((double) m / (double)(6 W)) with the integer m = 6 x (6 H and 6 y for v).  The corners overhang
 *     the block by a sixth of a texel: under bilinear filtering the seams between blocks bleed -- a stated limit, as is this: a ray that starts
 *     `reach` outside a thin part may hit the wrong sheet (voxelPS uses reach = cell).
 *
 * Valid once a volume exists; a band is not required (without one every hit is off-band).  Two calls on the same state give the same bits.  The
 * arrays are engine-owned pinned host memory, valid until the next extraction call on the context; the level-of-detail arrays are bit-equal to
 * psgsdf_extract_mesh_lod with the same arguments, and a later psgsdf_extract_mesh_* call returns what it returned before.  An empty
 * level-of-detail mesh: all sizes 0, return 0.
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for res < 1, a reach that is NaN, infinite or <= 0 and anything psgsdf_extract_mesh_lod
 * refuses; PSGSDF_ERR_UNSUPPORTED for an atlas beyond 16384 (before the atlas is allocated); PSGSDF_ERR_DEVICE if memory cannot be allocated
 * (everything is freed).  On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_BAKE_H_
#define PSGSDF_BAKE_H_

#include "psgsdf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psgsdf_bake {
    /* the level-of-detail mesh (psgsdf_extract_mesh_lod's outputs) */
    const float* xyz; const float* normals; const uint8_t* rgb; const int32_t* faces; const int32_t* vertex_map;
    int64_t n_vertices, n_faces, n_vertices_in, n_faces_in;
    const float* uv;               /* [n_faces][3][2] */
    int32_t width, height;         /* W, H */
    const uint8_t* albedo;         /* [H][W][3] */
    const float* normal;           /* [H][W][3] */
    const float* displacement;     /* [H][W] */
    const int32_t* voxel;          /* [H][W] */
    const int32_t* face;           /* [H][W] */
    int64_t n_texels, n_hits, n_hits_off_band, n_buried, n_misses;      /* n_texels: the owned ones = n_hits + n_buried + n_misses */
} psgsdf_bake;

int psgsdf_bake_lod(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_BAKE_H_ */
