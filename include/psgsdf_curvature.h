/* psgsdf_curvature.h -- curvature of the reconstructed surface, computed on the device from the signed distance field: at voxels of the caller's
 * (psgsdf_curvature_voxels), per vertex of the welded mesh (psgsdf_extract_mesh_curvature) and as one more map of the bake onto the level-of-detail
 * mesh (psgsdf_bake_lod_curvature).
 *
 * Not part of the reference-mirroring boundary (psgsdf.h); the reference has nothing comparable.  Photometric stereo exists to recover fine relief,
 * and curvature is how that relief is inspected and segmented.  It cannot be recomputed downstream at the quality the engine has: the welded mesh's
 * triangles are marching-cubes slivers, the coarse mesh has averaged the relief away, and the engine holds a signed distance field whose second
 * derivatives are one 19-point stencil away.
 *
 * Definition (DESIGN.md "Surface curvature").  All arithmetic is in double, without FMA contraction, with IEEE + - * / sqrt, in exactly the order
 * written.  Results are rounded to float32 at the end.
 *   h is the context's float32 voxel size, widened.
 *   The dense state is what psgsdf_download_volume would return at the time of the call.
 *   Linear index: lin = (k ny + j) nx + i.
 *   D(o) = (double) dist[lin + o].
 * Validity.  A voxel is valid iff all of the following hold:
 *   0 <= lin < nvox;
 *   1 <= i <= nx-2, and likewise for j and k;
 *   weight > 0 at all 19 stencil voxels: itself, the 6 axis neighbours, and the 12 in-plane diagonals (+-a, +-b);
 *   G2 > 0, with G2 defined below.
 *   An invalid voxel has valid = 0 and zeros everywhere.  It is never an error.
 * Stencil.
 *   g[a] = (D(+a) - D(-a)) / (2 h)
 *   H[a][a] = ((D(+a) + D(-a)) - 2 D(0)) / (h h)
 *   H[a][b] = ((D(+a+b) + D(-a-b)) - (D(+a-b) + D(-a+b))) / (4 h h)
 *   G2 = (gx gx + gy gy) + gz gz
 *   G = sqrt(G2)
 *   m = g / G, component by component
 * Tangent frame of m.  This is the frame of psgsdf_occlusion.h: sg = copysign(1, m[2]), a_ = -1 / (sg + m[2]), b_ = m[0] m[1] a_,
 *   t1 = (1 + sg m[0] m[0] a_, sg b_, -sg m[0]), t2 = (b_, sg + m[1] m[1] a_, -m[1]).
 * Shape operator.
 *   u1 = H t1 and u2 = H t2, each row as (H[r][0] t[0] + H[r][1] t[1]) + H[r][2] t[2]
 *   a = (t1.u1) / G, b = (t1.u2) / G, c = (t2.u2) / G, with dots as (x + y) + z
 * Results.
 *   mean = (a + c) / 2
 *   gauss = a c - b b
 *   hd = (a - c) / 2
 *   s = sqrt(hd hd + b b)
 *   k1 = mean + s
 *   k2 = mean - s
 * Direction of k1.
 *   If s == 0: e = (1, 0).  Else if hd >= 0: e = (hd + s, b).  Else: e = (b, s - hd).
 *   e is divided by sqrt(e0 e0 + e1 e1), and dir1 = e0 t1 + e1 t2.
 * Sign and units.
 *   dist grows outward.  A convex sphere of radius r through the voxel centre has mean = k1 = k2 = +1/r and gauss = 1/r^2.  Units are inverse
 *   mesh units.
 * This is the curvature of the level set through the voxel CENTRE.  At distance d from the zero set of a sphere of radius R it is 1/(R + d).  No
 * correction is applied.
 *
 * psgsdf_curvature_voxels: entry q of the results belongs to lin[q]; duplicates and any order are fine; n == 0 returns 0 with empty arrays.
 * psgsdf_extract_mesh_curvature: xyz, normals, rgb, faces are psgsdf_extract_mesh_indexed's arrays bit for bit.  A vertex with key 4 lin + e
 *   (psgsdf_mesh.h) has the end voxels lin and its +x / +y / +z neighbour (e = 0, 1, 2), or lin alone (a snapped corner, e = 3); its attributes are
 *   defined from the FLOAT per-voxel results of the end voxels.  With both ends valid every scalar is
 *   (float)((double) c_lo + (double) m ((double) c_hi - (double) c_lo)), m the float interpolation parameter of the vertex,
 *   (float) clamp((double)((0 - tl) / (th - tl)), 0, 1) with tl = -dist[lo], th = -dist[hi] in float, and vertex_valid = 2.  With one end valid the
 *   vertex takes that end's values and vertex_valid = 1.  With no end valid the values are zeros and vertex_valid = 0.  A snapped corner takes its
 *   own voxel's values and vertex_valid is 2 or 0.  No direction is carried onto vertices.
 * psgsdf_bake_lod_curvature: out->bake is bit for bit what psgsdf_bake_lod returns for the same arguments.  A texel with voxel >= 0 gets that
 *   voxel's mean and valid; missed, buried and padding texels get 0 / 0.  n_valid is the number of texels with valid != 0.
 *
 * Valid once a volume exists; a band is not required (only dist and weight are read).  No call changes a result of any other call: a call between
 * two psgsdf_iterate calls leaves the following iterations bit-identical, and two calls on the same state give the same bits.  The arrays are
 * engine-owned pinned host memory, valid until the next extraction call on the context.
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for n < 0, a NULL pointer, and whatever psgsdf_bake_lod refuses that way;
 * PSGSDF_ERR_UNSUPPORTED for what psgsdf_bake_lod refuses that way; PSGSDF_ERR_DEVICE if memory cannot be allocated or a launch is refused
 * (everything is freed).  A call that fails its argument checks leaves the caller's outputs untouched; one that fails later leaves the pointers
 * NULL and the struct zeroed.  On a context attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and device work.
 */
#ifndef PSGSDF_CURVATURE_H_
#define PSGSDF_CURVATURE_H_

#include "psgsdf_bake.h"

#ifdef __cplusplus
extern "C" {
#endif

/* valid [n] uint8, mean, gauss, k1, k2 [n] float32, dir1 [n][3] float32. */
int psgsdf_curvature_voxels(psgsdf_ctx* ctx, const int64_t* lin, int64_t n,
                            const uint8_t** valid, const float** mean, const float** gauss, const float** k1, const float** k2, const float** dir1);

/* vertex_valid [n_vertices] uint8 (0, 1 or 2 valid end voxels), vertex_mean, vertex_gauss, vertex_k1, vertex_k2 [n_vertices] float32.  An empty
 * mesh: all sizes 0, return 0. */
int psgsdf_extract_mesh_curvature(psgsdf_ctx* ctx, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                  const int32_t** faces, int64_t* n_faces,
                                  const uint8_t** vertex_valid, const float** vertex_mean, const float** vertex_gauss,
                                  const float** vertex_k1, const float** vertex_k2);

typedef struct psgsdf_bake_curvature {
    psgsdf_bake bake;              /* psgsdf_bake_lod's result */
    const float* mean;             /* [H][W] */
    const uint8_t* valid;          /* [H][W] */
    int64_t n_valid;
} psgsdf_bake_curvature;

int psgsdf_bake_lod_curvature(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake_curvature* out);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_CURVATURE_H_ */
