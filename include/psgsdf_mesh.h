/* psgsdf_mesh.h -- a welded, indexed triangle mesh with vertex normals, extracted on the device.
 *
 * Not part of the reference-mirroring boundary (psgsdf.h): psgsdf_extract_mesh keeps the reference's non-indexed output (three new vertices per
 * face, 8-bit colours with its index quirks), byte for byte.  This call returns the same surface as a mesh a downstream tool expects.
 *
 * Definition (DESIGN.md "Welded meshes"):
 *   - the cells of psgsdf_extract_mesh: its crop box (|d| <= sqrt(3) vs) and cell range (x < d0 - 2, y < d1 - 2, z < d2 - 2), a cell is valid iff
 *     all 8 corners have weight > 0, a corner is inside iff t = -dist > 0, the classic table; cells in (z, y, x) order, faces in table order;
 *     coordinates in its grid-local frame: voxel[a] = (vs d[a]) / d[a], origin[a] = -vs lo[a] (position = index * voxel - origin);
 *   - one vertex per intersected grid edge: the edge from voxel (i, j, k) to its +x / +y / +z neighbour is interpolated by the reference's
 *     interpolation with the LOWER end point first; where that snaps onto an end point (|t| < 1e-7), the vertex is that corner's, shared by every
 *     edge that snaps there.  Key = 4 * (global linear index of the lower end point, or of the corner) + {0 x-edge, 1 y-edge, 2 z-edge, 3 corner};
 *   - a face is dropped iff two of its three keys are equal; the vertices are exactly the keys of the kept faces, numbered in ascending key order;
 *   - normal = normalise(g_lo + mu (g_hi - g_lo)) of the two end points' normalised stored gradients (mu: the interpolation parameter; a snapped
 *     corner: its own), pointing outward (increasing dist; also the faces' winding); (0, 0, 0) where that is zero;
 *   - colour = the albedo interpolated with the same mu, clamped to [0, 1], byte = floor(255 c + 0.5).
 * A volume without a crop box, or with fewer than 3 voxels along an axis, gives 0 vertices and 0 faces.
 *
 * The arrays are engine-owned pinned host memory, valid until the next extraction call on the context.  On a context attached to a rank this is a
 * collective call: every rank returns its share (the cells whose lower plane it owns, the keys of the planes it owns), the shares concatenated in
 * rank order are the single context's arrays, and face indices are global (first_vertex = the global number of this share's vertex 0).
 */
#ifndef PSGSDF_MESH_H_
#define PSGSDF_MESH_H_

#include "psgsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xyz, normals: [n_vertices][3] float32; rgb: [n_vertices][3] uint8; faces: [n_faces][3] int32 (global vertex numbers).
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_UNSUPPORTED beyond 2^31 - 1 vertices. */
int psgsdf_extract_mesh_indexed(psgsdf_ctx* ctx, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
                                const int32_t** faces, int64_t* n_faces, int64_t* first_vertex);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_MESH_H_ */
