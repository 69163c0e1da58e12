// extract_internal.h -- what the extraction calls of extract.hip (mesh, point clouds, SDF block; it defines the functions below), of the mesh
// calls' files (extract_mesh.hip, extract_bake.hip, extract_compare.hip; their stages: mesh_stages.h) and of api_render.hip share on the host.
#pragma once
#include "engine_internal.h"
#include <initializer_list>
#include <vector>

namespace psg {
constexpr int kTile = 1024;      // elements per workgroup of the count scan
}
namespace psge {
// exclusive scan of int counts on the stream: v becomes the offsets, *total_host their sum (sums: one int per tile + 1); waits for the stream
int scan_counts(psgsdf_ctx* c, int* v, long long n, int* sums, int* total_host);
// engine-owned pinned host buffer that lives until the next extraction on this context
int host_out(psgsdf_ctx* c, XoSlot slot, size_t bytes, void** p);
// the eight float planes a mesh is made from, where a call puts its own in the place of the context's (extract_fill.hip: the filled state).  Every
// stage that takes a `const PlaneView*` reads c->dense for nullptr; a view is in the layout of c->dense and of a single-rank context.  framed: the
// vertices are placed in the frame of the box [flo, flo + fd) instead of the view's own crop box (the cells, keys and faces are the view's own)
struct PlaneView { const float* dist; const float* g[3]; const float* weight; const float* rho[3]; bool framed = false; int flo[3] = {0, 0, 0}, fd[3] = {0, 0, 0}; };
// the crop box of |d| <= sqrt(3) vs; any = false if no voxel qualifies (collective on a multi-rank context; waits for the stream); dist: the plane
// looked at, the context's if nullptr
int crop_box_dev(psgsdf_ctx* c, int lo[3], int hi[3], bool* any, const float* dist = nullptr);
// state checks of every extraction call, pending work flushed, the band's state scattered into the dense arrays
int extract_ready(psgsdf_ctx* c, const char* what);
// the calls that are not collective refuse a multi-rank context, `why` behind the colon.  A call checks this before anything collective and before
// any device work: every rank that calls leaves at once, and none waits for a rank that never called
inline int single_rank_only(psgsdf_ctx* c, const char* me, const char* why) {
    if (!c || c->n_ranks <= 1) return PSGSDF_OK;
    return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: not on a context attached to a rank (rank %d of %d): %s", me, c->rank, c->n_ranks, why);
}

// api_render.hip: the renderer's prepare path for a single-rank call -- dense planes, band state and grid into `a`, the occupied-brick map and its box
// built into `m` (k_render_bricks on the stream)
int render_prepare(psgsdf_ctx* c, DevMem& m, RenderArgs& a, const char* what);

// one result array of a call: `bytes` at `dev` go to the pinned slot, whose address goes to *out (nothing happens for 0 bytes)
struct XoCopy {
    template <class T> XoCopy(XoSlot slot, const void* dev, size_t bytes, const T** out) : slot(slot), dev(dev), bytes(bytes), out(out) {}
    XoSlot slot; const void* dev; size_t bytes; void* out;      // (out: the address of a pointer of the caller's)
};
// the results of call `me` to the host: pinned slots, copies behind whatever is in flight on the stream, ONE wait; the caller's pointers are
// written only if all of it worked
int download(psgsdf_ctx* c, const char* me, const std::vector<XoCopy>& list);

// the frame of the crop box [lo, hi] both meshes are built in (McGrid / WMeshGrid): the dense planes, the box, the voxel size and origin of
// MarchingCubes as write_mesh sets them up (host/ps_optimizer.hpp, operation for operation: the meshes are compared bit for bit) and this
// context's cell planes [g.zc0, *zc1): the cells whose lower plane it owns.  false: the box has no cell (computeIsoSurface runs to dim - 2).
// pv: the planes the frame points at instead of the context's
template <class Grid> bool crop_frame(const psgsdf_ctx* c, const int lo[3], const int hi[3], Grid& g, int* zc1, const PlaneView* pv = nullptr) {
#pragma clang fp contract(off)
    g.dist = pv ? pv->dist : c->dense.dist; g.weight = pv ? pv->weight : c->dense.weight;
    g.nx = c->grid.dim[0]; g.ny = c->grid.dim[1]; g.zlo = c->zlo;
    const float vs = c->grid.vs;
    for (int a = 0; a < 3; ++a) {
        g.rho[a] = pv ? pv->rho[a] : c->dense.rho[a];
        g.lo[a] = lo[a]; g.d[a] = hi[a] - lo[a] + 1;
        const float size = vs * g.d[a];                    // write_mesh: size[] = {vs * d[0], ..}, org[] = {-vs * lo[0], ..}
        g.voxel[a] = size / g.d[a];                        // MarchingCubes ctor: voxel_ = size / dim
        g.origin[a] = -vs * lo[a];
    }
    g.zc0 = std::max(0, c->z0 - lo[2]);
    *zc1 = std::min(g.d[2] - 2, c->z1 - lo[2]);
    return g.d[0] >= 3 && g.d[1] >= 3 && g.d[2] >= 3;
}
}  // namespace psge
