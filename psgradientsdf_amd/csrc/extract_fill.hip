// extract_fill.hip -- the C ABI of include/psgsdf_fill.h: the unobserved voxels next to observed ones filled by front propagation of the first-order
// model and relaxed by Jacobi sweeps (kernels: fill.hip; DESIGN.md "Hole filling"), returned as a list or meshed.  The filling works on a copy of the
// context's planes that the call owns; the mesh comes from stages 1 and 2 of mesh_stages.h, pointed at that copy through a PlaneView.  The context's
// own arrays are only read.
#include "mesh_stages.h"
#include "../../include/psgsdf_fill.h"
#include "fill.h"

using namespace psge;

namespace {
const char* kWhy = "a slab holds only its own planes of the volume";

// the filling on the device, everything in the call's DevMem: the working copy and the byte plane of rounds (always), and the n filled voxels in
// ascending lin with their final values val[a n + q] (n > 0)
struct FillDev {
    psg::FillPlanes w{}; unsigned char* round = nullptr;
    int n = 0; long long* lin = nullptr; unsigned char* rnd = nullptr; float* val = nullptr;
};

int fill_args(psgsdf_ctx* c, const char* me, int32_t rounds, int32_t sweeps) {
    if (rounds < 0 || rounds > PSGSDF_FILL_MAX_ROUNDS) return fail(c, PSGSDF_ERR_ARG, "%s: %d rounds (0 .. %d)", me, (int)rounds, PSGSDF_FILL_MAX_ROUNDS);
    if (sweeps < 0 || sweeps > PSGSDF_FILL_MAX_SWEEPS) return fail(c, PSGSDF_ERR_ARG, "%s: %d sweeps (0 .. %d)", me, (int)sweeps, PSGSDF_FILL_MAX_SWEEPS);
    return PSGSDF_OK;
}

// to_planes: the final values also go into the working copy (the mesh reads it; the list alone does not need it)
int fill_device(psgsdf_ctx* c, DevMem& mem, const char* me, int R, int K, bool to_planes, FillDev* f) {
    const int nx = c->grid.dim[0], ny = c->grid.dim[1], nz = c->grid.dim[2];
    const long long nvox = (long long)nx * ny * nz;
    if (nvox > INT32_MAX) return fail(c, PSGSDF_ERR_UNSUPPORTED, "%s: %lld voxels", me, nvox);      // (voxels are numbered in ints: the neighbour codes of fill.h)
    const size_t nv = (size_t)nvox;
    psg::FillPlanes& w = f->w;
    float** dst[8] = {&w.dist, &w.g[0], &w.g[1], &w.g[2], &w.weight, &w.rho[0], &w.rho[1], &w.rho[2]};
    const float* src[8] = {c->dense.dist, c->dense.g[0], c->dense.g[1], c->dense.g[2], c->dense.weight, c->dense.rho[0], c->dense.rho[1], c->dense.rho[2]};
    int* part = nullptr;
    bool ok = mem.get(&f->round, nv) && mem.get(&part, 6 * (size_t)psg::kFillBoxBlocks + 6);
    for (int a = 0; a < 8 && ok; ++a) ok = mem.get(dst[a], nv);
    if (!ok) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld voxels)", me, nvox);
    for (int a = 0; a < 8; ++a)
        if (hipMemcpyAsync(*dst[a], src[a], sizeof(float) * nv, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: copy of the planes", me);
    if (hipMemsetAsync(f->round, 0, nv, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: memset", me);
    if (R == 0) return PSGSDF_OK;
    int box[6];
    int* d_box = part + 6 * (size_t)psg::kFillBoxBlocks;
    timed(c, "fill_box", [&] { psg::launch_fill_box(c->dense.weight, nx, ny, nvox, part, d_box, c->stream); });
    if (hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, PSGSDF_ERR_DEVICE, "%s: the box of the observed voxels", me);
    if (box[3] < box[0]) return PSGSDF_OK;      // nothing observed: nothing to extend
    const int dim[3] = {nx, ny, nz};
    const int Re = std::min(R, nx + ny + nz - 3);      // (no voxel is farther from another than that)
    psg::FillGrid g{};
    g.weight0 = c->dense.weight; g.w = w; g.round = f->round; g.nx = nx; g.ny = ny; g.nz = nz; g.vs = c->grid.vs;
    auto grown = [&](int r) {
        for (int a = 0; a < 3; ++a) { g.lo[a] = std::max(0, box[a] - r); g.d[a] = std::min(dim[a] - 1, box[3 + a] + r) - g.lo[a] + 1; }
    };
    for (int r = 1; r <= Re; ++r) {
        grown(r);
        timed(c, "fill_round", [&] { psg::launch_fill_round(g, r, c->stream); });
    }
    grown(Re);      // every filled voxel lies in it
    const long long ncell = (long long)g.d[0] * g.d[1] * g.d[2];
    int *flag = nullptr, *sums = nullptr;
    if (!mem.get(&flag, (size_t)ncell) || !mem.get(&sums, (size_t)((ncell + psg::kTile - 1) / psg::kTile + 1))) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld voxels)", me, ncell);
    timed(c, "fill_flags", [&] { psg::launch_fill_flags(g, flag, c->stream); });
    int n = 0;
    if (int rc = scan_counts(c, flag, ncell, sums, &n)) return rc;      // flags -> list positions in ascending lin
    if (n == 0) return PSGSDF_OK;
    const size_t N = (size_t)n;
    int* nb = nullptr; float *v0 = nullptr, *v1 = nullptr;      // temporaries: 89 B per filled voxel
    if (!mem.get(&f->lin, N) || !mem.get(&f->rnd, N) || !mem.get(&nb, 6 * N) || !mem.get(&v0, psg::kFillVals * N) || (K > 0 && !mem.get(&v1, psg::kFillVals * N)))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d filled voxels)", me, n);
    timed(c, "fill_list", [&] { psg::launch_fill_list(g, flag, n, f->lin, f->rnd, nb, v0, c->stream); });
    for (int k = 0; k < K; ++k) {
        timed(c, "fill_sweep", [&] { psg::launch_fill_sweep(w, nb, n, v0, v1, c->stream); });
        std::swap(v0, v1);
    }
    if (K > 0 && to_planes) timed(c, "fill_scatter", [&] { psg::launch_fill_scatter(w, f->lin, n, v0, c->stream); });
    if (hipGetLastError() != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch (%d rounds, %d sweeps, %d filled voxels)", me, R, K, n);
    f->n = n; f->val = v0;
    return PSGSDF_OK;
}
}  // namespace

extern "C" int psgsdf_fill_voxels(psgsdf_ctx* c, int32_t rounds, int32_t sweeps, const int64_t** lin, const float** dist, const float** grad, const float** rgb, const uint8_t** round,
                                  int64_t* n_filled) {
    const char* me = "fill_voxels";
    if (!lin || !dist || !grad || !rgb || !round || !n_filled) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, kWhy)) return rc;
    if (int rc = fill_args(c, me, rounds, sweeps)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *lin = nullptr; *dist = nullptr; *grad = nullptr; *rgb = nullptr; *round = nullptr; *n_filled = 0;
    DevMem mem(c);
    FillDev f;
    if (int rc = fill_device(c, mem, me, rounds, sweeps, false, &f)) return rc;
    if (f.n == 0) return PSGSDF_OK;
    const size_t n = (size_t)f.n;
    float *d_grad = nullptr, *d_rgb = nullptr;      // temporaries: 24 B per filled voxel
    if (!mem.get(&d_grad, 3 * n) || !mem.get(&d_rgb, 3 * n)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d filled voxels)", me, f.n);
    timed(c, "fill_pack", [&] { psg::launch_fill_pack(f.val, f.n, d_grad, d_rgb, c->stream); });
    if (int rc = download(c, me, {{XO_FILL_LIN, f.lin, sizeof(long long) * n, lin}, {XO_FILL_DIST, f.val, sizeof(float) * n, dist}, {XO_FILL_GRAD, d_grad, sizeof(float) * 3 * n, grad},
                                  {XO_FILL_RGB, d_rgb, sizeof(float) * 3 * n, rgb}, {XO_FILL_ROUND, f.rnd, n, round}})) return rc;
    *n_filled = f.n;
    return PSGSDF_OK;
}

extern "C" int psgsdf_extract_mesh_filled(psgsdf_ctx* c, int32_t rounds, int32_t sweeps, const psgsdf_mesh_filter* filter, const float** xyz, const float** normals, const uint8_t** rgb,
                                          int64_t* n_vertices, const int32_t** faces, int64_t* n_faces, const int32_t** vertex_component, const psgsdf_mesh_component** components,
                                          int64_t* n_components, const uint8_t** vertex_filled) {
    const char* me = "extract_mesh_filled";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_component || !components || !n_components || !vertex_filled) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, kWhy)) return rc;
    if (int rc = fill_args(c, me, rounds, sweeps)) return rc;
    psgsdf_mesh_filter flt{0, 0.0, 0};
    if (filter) flt = *filter;
    if (bad_filter(flt)) return fail(c, PSGSDF_ERR_ARG, "%s: min_area is NaN or keep_largest < 0", me);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_component = nullptr; *components = nullptr; *vertex_filled = nullptr;
    *n_vertices = 0; *n_faces = 0; *n_components = 0;
    DevMem mem(c);
    FillDev f;
    if (int rc = fill_device(c, mem, me, rounds, sweeps, true, &f)) return rc;
    PlaneView pv{f.w.dist, {f.w.g[0], f.w.g[1], f.w.g[2]}, f.w.weight, {f.w.rho[0], f.w.rho[1], f.w.rho[2]}};
    {      // the vertex frame is the UNFILLED state's, if it has a crop box: a vertex between unfilled voxels keeps the bits it has in the unfilled mesh
        int lo[3], hi[3]; bool any = false;
        if (int rc = crop_box_dev(c, lo, hi, &any)) return rc;
        pv.framed = any;
        for (int a = 0; a < 3 && any; ++a) { pv.flo[a] = lo[a]; pv.fd[a] = hi[a] - lo[a] + 1; }
    }
    MCompDev d;
    int rc = mcomp_device(c, mem, me, flt, &d, &pv);
    if (rc || d.nc == 0) return rc;      // (failed, or an empty mesh)
    MeshView kept = d;
    if (!(d.nv > 0 && d.nf > 0)) kept.nv = kept.nf = 0;      // (a filter may drop everything)
    unsigned char* v_filled = nullptr;      // temporary: 1 B per vertex
    if (kept.nv > 0) {
        if (!mem.get(&v_filled, (size_t)kept.nv)) return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices)", me, kept.nv);
        timed(c, "wmesh_filled", [&] { psg::launch_wmesh_filled(d.welded.grid, d.welded.num, d.welded.nv, f.round, d.vkeep, kept.nv, v_filled, c->stream); });
    }
    rc = download_mesh(c, me, kept, {xyz, normals, rgb, faces}, {{XO_VERTEX_COMPONENT, d.vertex_component, sizeof(int) * (size_t)kept.nv, vertex_component},
                                                                 {XO_FILL_VERTEX, v_filled, (size_t)kept.nv, vertex_filled}});
    if (rc) return rc;
    *n_vertices = kept.nv; *n_faces = kept.nf; *components = d.list; *n_components = d.nc;
    return PSGSDF_OK;
}
