// mesh_stages.h -- the stages the mesh calls of extract_mesh.hip (which defines them), extract_bake.hip and extract_compare.hip are chained from:
// welded mesh -> components -> clusters.  A CALL owns all device memory of its stages in one DevMem, which waits for the stream and frees when the
// call returns, whichever way it returns: a stage allocates from it and never frees, and the arrays it hands on may still be in flight.
#pragma once
#include "extract_internal.h"
#include "../../include/psgsdf_mesh.h"

namespace psge {
// a mesh as device arrays, the kernels that write them launched on the stream and not waited for
struct MeshView { const float *xyz = nullptr, *nrm = nullptr; const unsigned char* rgb = nullptr; const int* faces = nullptr; int nv = 0, nf = 0; };

// ---- stage 1: the welded mesh of the context's state (this rank's share; collective on a multi-rank context).  nv == 0 && nf == 0: nothing was
// launched for it.  grid, num: the key slots and their vertex numbers (the scan of the used-key flags)
// pv (single-rank contexts only): the planes the mesh is made from instead of the context's
struct WMeshDev : MeshView { long long first = 0; psg::WMeshGrid grid{}; const int* num = nullptr; };
int wmesh_device(psgsdf_ctx* c, DevMem& mem, WMeshDev* m, const PlaneView* pv = nullptr);

// ---- stage 2: the components of the welded mesh and the mesh without the ones the filter drops (the welded arrays themselves if all are kept); the
// component list is written to its pinned host slot.  nc == 0: an empty mesh, the stream has been waited for.  welded: the stage-1 mesh it came
// from; vkeep: the exclusive scan of the kept flags of the welded vertices (their numbers in this mesh), nullptr if all are kept
struct MCompDev : MeshView { const int* vertex_component = nullptr; int nc = 0; psgsdf_mesh_component* list = nullptr; WMeshDev welded; const int* vkeep = nullptr; };
bool bad_filter(const psgsdf_mesh_filter& flt);
int mcomp_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter& flt, MCompDev* d, const PlaneView* pv = nullptr);

// the mesh a call goes on from: the welded mesh as it is (no filter: no component pass) or its kept components; an empty view for an empty mesh or a
// filter that drops everything
int compared_mesh(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, MeshView* mv);

// a call's mesh into the XO_IMESH_* slots and the caller's four pointers, `more` (the call's own arrays) behind it: ONE download, one wait
struct MeshOut { const float** xyz; const float** normals; const uint8_t** rgb; const int32_t** faces; };
int download_mesh(psgsdf_ctx* c, const char* me, const MeshView& mv, const MeshOut& o, std::initializer_list<XoCopy> more = {});

// ---- stage 3: the input mesh `in` (nv > 0, nf > 0) clustered, and the result in its pinned host slots; dev (if asked for): the result's device arrays
struct LodOut {
    const float** xyz; const float** normals; const uint8_t** rgb; int64_t* n_vertices; const int32_t** faces; int64_t* n_faces; const int32_t** vertex_map;
    int64_t* n_vertices_in; int64_t* n_faces_in;
};
int lod_from_device(psgsdf_ctx* c, DevMem& mem, const MeshView& in, double cell, const LodOut& o, MeshView* dev = nullptr);
// what psgsdf_extract_mesh_lod and the bakes check first (ranks, cell, filter) ...
int lod_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell);
// ... and the stages they run: compared_mesh, then the clusters unless it is empty (then the stream has been waited for and `o` is untouched)
int lod_stages(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, const LodOut& o, MeshView* dev = nullptr);
}  // namespace psge

// ---- stage 4 (extract_bake.hip defines it; extract_curvature.hip goes on from it): the clusters baked
struct psgsdf_bake;
namespace psg { struct BakeArgs; }
namespace psge {
// what psgsdf_bake_lod and every call that starts with its bake check first
int bake_ready(psgsdf_ctx* c, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach);
int bake_device(psgsdf_ctx* c, DevMem& mem, const char* me, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake* out, psg::BakeArgs* dev = nullptr,
                long long max_texels = 0);
}  // namespace psge
