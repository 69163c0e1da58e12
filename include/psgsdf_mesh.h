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

/* ---- connected components of that mesh, and the mesh without its small pieces (DESIGN.md "Mesh components"; kernels: csrc/mesh_cc.hip)
 *
 * Starts from the welded mesh exactly as psgsdf_extract_mesh_indexed defines it (same cells, keys, vertex numbers, face order).
 *   - Two vertices are connected iff some kept face uses both; a component is a connected component of that graph.  Every vertex belongs to a face,
 *     so every component has at least one face.  Pieces that touch only in a shared (snapped-corner) vertex are one component.
 *   - A component's identity is first_vertex, the smallest vertex number in it (counted in the UNFILTERED mesh); components are listed in ascending
 *     first_vertex, so the labelling does not depend on thread scheduling.
 *   - Per component: n_vertices, n_faces, n_edges (distinct undirected edges), n_boundary_edges (used by exactly one face), n_nonmanifold_edges (used
 *     by more than two), area, the bounding box lo / hi of the float32 positions, kept.  Euler characteristic = n_vertices - n_edges + n_faces;
 *     closed means n_boundary_edges == 0 && n_nonmanifold_edges == 0.
 *   - area is defined in fixed point so that it is the same bits on every call: area = vs^2 2^-24 sum over the faces of llrint(2^24 A_f / vs^2),
 *     A_f the triangle's area computed in double from the returned float32 positions, vs the context's float32 voxel size widened to double.
 *   - filter: a component passes if n_faces >= min_faces and area >= min_area.  If keep_largest > 0, of those that pass only the keep_largest with
 *     the most faces are kept; ties go to the smaller first_vertex.  A NULL filter, or all zeros, keeps everything.
 *   - output: the vertices of the kept components in their original order, renumbered densely; the kept faces in their original order with the new
 *     numbers; vertex_component[v] for every returned vertex, an index into the component list; the component list with ALL components, dropped ones
 *     too (kept = 0).  With everything kept, xyz / normals / rgb / faces are bit-equal to psgsdf_extract_mesh_indexed on the same state.  Nothing
 *     kept: 0 vertices, 0 faces, the list still filled.  An empty mesh: 0 components.
 * The arrays are engine-owned pinned host memory, valid until the next extraction call on the context.  PSGSDF_ERR_STATE before a volume exists;
 * PSGSDF_ERR_ARG for a NaN min_area or a negative keep_largest; PSGSDF_ERR_DEVICE if a temporary cannot be allocated.  On a context attached to a
 * rank the call returns PSGSDF_ERR_UNSUPPORTED on every rank before any exchange (components across z-slabs are not merged yet). */
typedef struct psgsdf_mesh_filter { int64_t min_faces; double min_area; int32_t keep_largest; } psgsdf_mesh_filter;
typedef struct psgsdf_mesh_component { int64_t first_vertex, n_vertices, n_faces, n_edges, n_boundary_edges,
    n_nonmanifold_edges; double area; float lo[3], hi[3]; int32_t kept, reserved; } psgsdf_mesh_component;
int psgsdf_extract_mesh_components(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter,
    const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
    const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component,
    const psgsdf_mesh_component** components, int64_t* n_components);

/* ---- a level-of-detail mesh by vertex clustering (DESIGN.md "Level of detail"; kernels: csrc/mesh_lod.hip)
 *
 * Input mesh (V_in vertices, F_in faces): with filter == NULL the welded mesh exactly as psgsdf_extract_mesh_indexed defines it (no component pass);
 * otherwise exactly what psgsdf_extract_mesh_components(ctx, filter) returns, the kept components renumbered.  vs: the context's float32 voxel size at
 * the time of the call, widened to double (it halves with the 2x refinement).  cell: the cluster size, a double in the mesh's units.
 *   - Cluster of a vertex: per axis c[a] = (int64) floor((double) xyz[a] / cell), a true IEEE double division (vertices sit exactly on cell walls
 *     when cell is a whole number of voxels: the quotient's bits decide).  Same cluster iff all three are equal.  |c[a]| >= 2^20 for any vertex:
 *     PSGSDF_ERR_UNSUPPORTED and no output.
 *   - Faces: a face is dropped if two of its three vertices' clusters are equal; of the remaining faces with the same unordered triple of clusters
 *     only the one with the smallest input index is kept, in its own orientation; kept faces stay in input order.
 *   - Vertices: one per cluster that a kept face uses, numbered in ascending order of the cluster's smallest member (an input vertex number), so the
 *     numbering does not depend on thread scheduling.  Members of the other clusters get vertex_map = -1.
 *   - Attributes of a cluster of n members, all order-independent integer sums:
 *       position  S[a] = sum llrint((double) xyz[a] * 2^20 / vs);   pos[a] = (float)((double) S[a] / (double) n * (vs / 2^20))
 *       normal    T[a] = sum llrint((double) normal[a] * 2^20);     T / sqrt((Tx^2 + Ty^2) + Tz^2) in double, rounded to float; (0, 0, 0) if T = 0
 *       colour    per channel (2 * sum of the bytes + n) / (2 n) in integer arithmetic
 *     a single-member cluster keeps its member's position, normal and colour bit for bit.
 * Output: xyz, normals [n_vertices][3] float32, rgb [n_vertices][3] uint8, faces [n_faces][3] int32 in output numbers, vertex_map [n_vertices_in] int32
 * (the output vertex of every input vertex, or -1), n_vertices_in = V_in, n_faces_in = F_in.  An empty input mesh: all sizes 0, return 0.  The arrays
 * are engine-owned pinned host memory, valid until the next extraction call on the context; a later psgsdf_extract_mesh_indexed or
 * psgsdf_extract_mesh_components returns what it returned before.
 * PSGSDF_ERR_STATE before a volume exists; PSGSDF_ERR_ARG for a cell that is NaN, infinite or <= 0, or a filter psgsdf_extract_mesh_components
 * refuses; PSGSDF_ERR_UNSUPPORTED for the coordinate bound; PSGSDF_ERR_DEVICE if a temporary cannot be allocated (everything is freed).  On a context
 * attached to a rank: PSGSDF_ERR_UNSUPPORTED on every rank, at once, before any exchange and before any device work. */
int psgsdf_extract_mesh_lod(psgsdf_ctx* ctx, const psgsdf_mesh_filter* filter, double cell,
    const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices,
    const int32_t** faces, int64_t* n_faces, const int32_t** vertex_map,
    int64_t* n_vertices_in, int64_t* n_faces_in);

#ifdef __cplusplus
}
#endif
#endif /* PSGSDF_MESH_H_ */
