// extract_curvature.hip -- the C ABI of include/psgsdf_curvature.h: curvature of the distance field's level sets at the caller's voxels, per vertex
// of the welded mesh and as one more map of the bake (kernels: curvature.hip; DESIGN.md "Surface curvature").  One device function, three consumers:
// the mesh comes from stage 1 and the atlas from stage 4 of mesh_stages.h, whose planes are still on the device when the texels are evaluated.
#include "mesh_stages.h"
#include "../../include/psgsdf_curvature.h"
#include "bake.h"
#include "curvature.h"

using namespace psge;

namespace {
// what the three calls read: the dense planes of a single-rank context (local plane 0 is global plane 0)
psg::CurvGrid curv_grid(const psgsdf_ctx* c) { return psg::CurvGrid{c->dense.dist, c->dense.weight, c->grid.dim[0], c->grid.dim[1], c->grid.dim[2], c->grid.vs}; }
const char* kWhy = "a slab holds only its own planes of the volume";
}  // namespace

extern "C" int psgsdf_curvature_voxels(psgsdf_ctx* c, const int64_t* lin, int64_t n, const uint8_t** valid, const float** mean, const float** gauss,
                                       const float** k1, const float** k2, const float** dir1) {
    const char* me = "curvature_voxels";
    if (!valid || !mean || !gauss || !k1 || !k2 || !dir1 || (n > 0 && !lin)) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, kWhy)) return rc;
    if (n < 0) return fail(c, PSGSDF_ERR_ARG, "%s: %lld voxels", me, (long long)n);
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *valid = nullptr; *mean = nullptr; *gauss = nullptr; *k1 = nullptr; *k2 = nullptr; *dir1 = nullptr;
    if (n == 0) return PSGSDF_OK;
    DevMem mem(c);
    const size_t N = (size_t)n;
    long long* d_lin = nullptr; unsigned char* d_valid = nullptr; float *d_mean = nullptr, *d_gauss = nullptr, *d_k1 = nullptr, *d_k2 = nullptr, *d_dir = nullptr;      // temporaries: 37 B per entry
    if (!mem.get(&d_lin, N) || !mem.get(&d_valid, N) || !mem.get(&d_mean, N) || !mem.get(&d_gauss, N) || !mem.get(&d_k1, N) || !mem.get(&d_k2, N) || !mem.get(&d_dir, 3 * N))
        return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%lld voxels)", me, (long long)n);
    if (hipMemcpyAsync(d_lin, lin, sizeof(long long) * N, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: upload", me);
    timed(c, "curv_voxels", [&] { psg::launch_curv_voxels(curv_grid(c), d_lin, (long long)n, d_valid, d_mean, d_gauss, d_k1, d_k2, d_dir, c->stream); });
    if (hipGetLastError() != hipSuccess) return fail(c, PSGSDF_ERR_DEVICE, "%s: launch over %lld voxels", me, (long long)n);
    return download(c, me, {{XO_CURV_VALID, d_valid, N, valid}, {XO_CURV_MEAN, d_mean, sizeof(float) * N, mean}, {XO_CURV_GAUSS, d_gauss, sizeof(float) * N, gauss},
                            {XO_CURV_K1, d_k1, sizeof(float) * N, k1}, {XO_CURV_K2, d_k2, sizeof(float) * N, k2}, {XO_CURV_DIR1, d_dir, sizeof(float) * 3 * N, dir1}});
}

extern "C" int psgsdf_extract_mesh_curvature(psgsdf_ctx* c, const float** xyz, const float** normals, const uint8_t** rgb, int64_t* n_vertices, const int32_t** faces, int64_t* n_faces,
                                             const uint8_t** vertex_valid, const float** vertex_mean, const float** vertex_gauss, const float** vertex_k1, const float** vertex_k2) {
    const char* me = "extract_mesh_curvature";
    if (!xyz || !normals || !rgb || !n_vertices || !faces || !n_faces || !vertex_valid || !vertex_mean || !vertex_gauss || !vertex_k1 || !vertex_k2)
        return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = single_rank_only(c, me, kWhy)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *xyz = nullptr; *normals = nullptr; *rgb = nullptr; *faces = nullptr; *vertex_valid = nullptr; *vertex_mean = nullptr; *vertex_gauss = nullptr; *vertex_k1 = nullptr; *vertex_k2 = nullptr;
    *n_vertices = 0; *n_faces = 0;
    DevMem mem(c);
    WMeshDev m;
    if (int rc = wmesh_device(c, mem, &m)) return rc;
    const size_t nv = (size_t)m.nv;
    unsigned char* v_valid = nullptr; float *v_mean = nullptr, *v_gauss = nullptr, *v_k1 = nullptr, *v_k2 = nullptr;      // temporaries: 17 B per vertex
    if (nv > 0) {
        if (!mem.get(&v_valid, nv) || !mem.get(&v_mean, nv) || !mem.get(&v_gauss, nv) || !mem.get(&v_k1, nv) || !mem.get(&v_k2, nv))
            return fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d vertices)", me, m.nv);
        timed(c, "wmesh_curv", [&] { psg::launch_wmesh_curv(curv_grid(c), m.grid, m.num, m.nv, v_valid, v_mean, v_gauss, v_k1, v_k2, c->stream); });
    }
    if (int rc = download_mesh(c, me, m, {xyz, normals, rgb, faces}, {{XO_VCURV_VALID, v_valid, nv, vertex_valid}, {XO_VCURV_MEAN, v_mean, sizeof(float) * nv, vertex_mean},
                                                                      {XO_VCURV_GAUSS, v_gauss, sizeof(float) * nv, vertex_gauss}, {XO_VCURV_K1, v_k1, sizeof(float) * nv, vertex_k1},
                                                                      {XO_VCURV_K2, v_k2, sizeof(float) * nv, vertex_k2}})) return rc;
    *n_vertices = m.nv; *n_faces = m.nf;
    return PSGSDF_OK;
}

extern "C" int psgsdf_bake_lod_curvature(psgsdf_ctx* c, const psgsdf_mesh_filter* filter, double cell, int32_t res, double reach, psgsdf_bake_curvature* out) {
    const char* me = "bake_lod_curvature";
    if (!out) return fail(c, PSGSDF_ERR_ARG, "%s: null argument", me);
    if (int rc = bake_ready(c, me, filter, cell, res, reach)) return rc;
    { int rc = extract_ready(c, me); if (rc) return rc; }
    *out = psgsdf_bake_curvature{};
    DevMem mem(c);
    psg::BakeArgs b{};
    if (int rc = bake_device(c, mem, me, filter, cell, res, reach, &out->bake, &b)) return rc;
    if (b.nf <= 0) return PSGSDF_OK;      // an empty level-of-detail mesh: nothing was baked
    const size_t n = (size_t)b.W * (size_t)b.H;
    float* d_mean = nullptr; unsigned char* d_valid = nullptr;      // temporaries: 5 B per texel
    auto give_up = [&](int rc) { *out = psgsdf_bake_curvature{}; return rc; };
    if (!mem.get(&d_mean, n) || !mem.get(&d_valid, n)) return give_up(fail(c, PSGSDF_ERR_DEVICE, "%s: out of memory (%d x %d texels)", me, b.W, b.H));
    timed(c, "bake_curv", [&] { psg::launch_bake_curv(curv_grid(c), b.voxel, (long long)n, d_mean, d_valid, c->stream); });
    if (int rc = download(c, me, {{XO_BAKE_CURV_MEAN, d_mean, sizeof(float) * n, &out->mean}, {XO_BAKE_CURV_VALID, d_valid, n, &out->valid}})) return give_up(rc);
    int64_t nvld = 0;
    for (size_t t = 0; t < n; ++t) nvld += out->valid[t] != 0;
    out->n_valid = nvld;
    return PSGSDF_OK;
}
