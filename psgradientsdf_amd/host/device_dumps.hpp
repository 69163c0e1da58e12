// device_dumps.hpp — the dumps that come from the device-side extraction (include/psgsdf.h psgsdf_extract_* and the result families beside it):
// compact arrays come back, valid until the next extraction call; a copy of them goes to the background writer (dump_queue.hpp), which formats the
// file (ply_io.hpp).  Every routine takes the context and the name of the <name>_mesh.ply (or the file) it belongs to; false: nothing was queued.
// What to dump is one record, DumpOptions: filled in by voxelPS (checked there) and voxelps_scene (taken as given).  Every flag is documented here, at
// its member; <name> is a dump's name without `_mesh.ply`.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/psgsdf.h"
#include "../../include/psgsdf_mesh.h"
#include "../../include/psgsdf_fit.h"
#include "../../include/psgsdf_bake.h"
#include "../../include/psgsdf_occlusion.h"
#include "../../include/psgsdf_photo.h"
#include "../../include/psgsdf_compare.h"
#include "../../include/psgsdf_align.h"
#include "../../include/psgsdf_curvature.h"
#include "../../include/psgsdf_fill.h"
#include "../../include/psgsdf_query.h"
#include "../../include/psgsdf_relight.h"
#include "dump_queue.hpp"
#include "obj_writer.hpp"
#include "ply_io.hpp"
#include "png_writer.hpp"

namespace psgsdf_host {

// --compare-ply FILE [--compare-tau T] [--compare-max D]: next to every <name>_mesh.ply a <name>_compare.txt (both directions' counts, mean / rms /
// max / signed mean, histogram, precision / recall / F) and a <name>_mesh_compare.ply (the welded mesh -- the filtered one, if a filter flag is given --
// with every vertex's distance to the reference and the side it lies on): psgsdf_compare_reference against the mesh or cloud read from FILE, whose
// coordinates are those of <name>_mesh_indexed.ply (the mesh's units: that writer adds no offset); T and D in voxels; single process only
// --compare-align [--compare-align-iters K]: before each comparison the reference is aligned to that dump's mesh from the identity (psgsdf_align_reference:
// both directions, the filter flags applied, the radius of --compare-max, at most K = 30 steps), the comparison runs on the aligned points, and a
// <name>_align.txt is written next to <name>_compare.txt: the status word, one line per iteration, the final evaluation, the 4x4 transform with %.17g
struct CompareRef { bool on = false; std::string file; std::vector<float> xyz; std::vector<int32_t> faces; double tau_voxels = 1.0, max_voxels = 8.0; bool align = false; int align_iters = 30; };
// --query-ply FILE [--query-model cell|trilinear] [--query-project]: next to every <name>_mesh.ply a <name>_query.ply, the vertices of FILE (read by
// the reader of --compare-ply; coordinates as in <name>_mesh_indexed.ply) with the field there (psgsdf_query_points: float distance nx ny nz red green
// blue weight, uchar status) or, with --query-project, moved onto the surface (psgsdf_project_points, tolerance 1e-3 voxel, at most 16 moves: the
// projected positions with float distance -- signed, the length moved -- and residual, uchar iterations and status); the model defaults to trilinear;
// single process only
struct QueryRef { bool on = false; std::string file; std::vector<float> xyz; int model = PSGSDF_Q_TRILINEAR; bool project = false; };
// --relight FILE: the lights of the file (include/psgsdf_relight.h), bias and reach in voxels
struct RelightSpec { bool on = false; double bias_voxels = 1.0, reach_voxels = 0.0; std::vector<psgsdf_light> lights; };

struct DumpOptions {
    // --host-writers: round 4's dump path (dense download, host marching cubes, iostream; every dump written where it is issued) and frame path (serial
    // decode, normals through the host): the single-process cross-check of the device / threaded one
    bool host_writers = false;
    // --indexed-mesh: a <name>_mesh_indexed.ply (welded, normals, binary; psgsdf_extract_mesh_indexed) next to every <name>_mesh.ply
    bool indexed_mesh = false;
    // --mesh-min-faces N / --mesh-keep-largest K: next to every <name>_mesh.ply a <name>_mesh_clean.ply (the welded mesh without the connected components
    // the filter drops, psgsdf_extract_mesh_components) and a <name>_mesh_components.txt (every component, one per line); single process only
    bool clean_mesh = false;
    psgsdf_mesh_filter mesh_filter{0, 0.0, 0};
    const psgsdf_mesh_filter* filter() const { return clean_mesh ? &mesh_filter : nullptr; }      // what the other mesh dumps hand the engine: null without a filter flag
    // --mesh-lod S: next to every <name>_mesh.ply a <name>_mesh_lod.ply, the welded mesh (the filtered one, if a filter flag is given) with the vertices
    // of every cube of S voxels merged into one (psgsdf_extract_mesh_lod); 0: off; single process only
    double lod_voxels = 0.0;
    // --mesh-bake R (with --mesh-lod S): next to every <name>_mesh_lod.ply the same mesh as <name>_mesh_lod.obj / .mtl with the reconstruction's detail
    // baked into <name>_mesh_lod_albedo.png and <name>_mesh_lod_normal.png (object space), R texels along a triangle's edge, rays from one cell outside
    // (psgsdf_bake_lod); 0: off; single process only
    int bake_res = 0;
    // --mesh-bake-ao K (with --mesh-bake): <name>_mesh_lod_ao.png next to the other maps (grey, 255 = open) and one `map_Ka` line in the .mtl: the
    // ambient occlusion of the reconstructed surface from K rays per texel, radius 8 voxels, origins 1 voxel off the surface (psgsdf_bake_lod_ao); 0: off
    int bake_ao_dirs = 0;
    // --mesh-bake-photo (with --mesh-bake): <name>_mesh_lod_photo.png next to the other maps, the albedo of every texel solved from the keyframes that
    // see it (psgsdf_bake_lod_photo: rays lifted 1 voxel, cos_min 0.2, shade_min 0.05), and `map_Kd` in the .mtl names it; _albedo.png is still written.  A
    // dump taken before psgsdf_init (the fused volume's) has no keyframes to solve from and is baked as without the flag
    bool bake_photo = false;
    // --mesh-bake-curvature S (with --mesh-bake): <name>_mesh_lod_curvature.png next to the other maps, 8-bit grey: the mean curvature of every hit
    // texel's voxel (psgsdf_bake_lod_curvature), mean * vs = S white, -S black, flat and every texel without a value 128; convex is bright; 0: off
    double bake_curvature_scale = 0.0;
    // --mesh-fit: next to every <name>_mesh.ply a <name>_mesh_fit.ply, the welded mesh with the photometric fit of every vertex (psgsdf_extract_mesh_fit):
    // how many keyframes saw it, the rms residual and the mean robust loss; single process only
    bool fit = false;
    // --mesh-curvature: next to every <name>_mesh.ply a <name>_mesh_curvature.ply, the welded mesh with the curvature of every vertex
    // (psgsdf_extract_mesh_curvature): mean, Gaussian and the two principal curvatures, and how many of its end voxels could be evaluated; single process only
    bool curvature = false;
    // --mesh-fill R [--mesh-fill-sweeps K]: next to every <name>_mesh.ply a <name>_mesh_filled.ply, the welded mesh of the state with its unobserved
    // voxels filled over R front rounds (holes up to about 2 R voxels wide close) and K relaxation sweeps (psgsdf_extract_mesh_filled; the filter flags
    // apply to it) and how many of every vertex's end voxels are filled; -1: off; single process only
    int fill_rounds = -1, fill_sweeps = 4;
    CompareRef compare;
    QueryRef query;
    RelightSpec relight;
    // voxelPS reads nothing of the refined volume after alternatingOptimize (main_ps.cpp:330-343 ends there): the executable skips the whole-volume download
    // that mirrors the reference's in-place mutation of tSDF_ (a host that goes on using tSDF_ keeps it: the default)
    bool skip_sync_back = false;
};
inline DumpOptions& dump_options() { static DumpOptions o; return o; }

// the mean curvature of a baked texel as a grey byte (--mesh-bake-curvature S): mean * vs = S white, -S black, no value 128
inline uint8_t curvature_to_u8(float mean, uint8_t valid, double vs, double S) {
    if (!valid) return 128;
    const double x = 0.5 + 0.5 * (double)mean * vs / S;
    return (uint8_t)std::floor(255.0 * (!(x > 0.0) ? 0.0 : x > 1.0 ? 1.0 : x) + 0.5);
}

// An owned copy of a welded mesh of the engine's, with the grid's origin and voxel size and whatever columns go with its vertices: what a queued
// job writes from after the engine's arrays have been reused.
struct MeshSnapshot {
    std::vector<float> xyz, normals; std::vector<uint8_t> rgb; std::vector<int32_t> faces; std::array<float, 3> origin; float vs;
    std::vector<std::vector<char>> owned; std::vector<PlyColumn> columns;      // columns[k].data points into owned[k]
    MeshSnapshot(psgsdf_ctx* ctx, const float* x, const float* n, const uint8_t* c, int64_t nv, const int32_t* f, int64_t nf)
        : xyz(x, x + 3 * nv), normals(n, n + 3 * nv), rgb(c, c + 3 * nv), faces(f, f + 3 * nf) {
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        origin = {info.origin[0], info.origin[1], info.origin[2]}; vs = info.voxel_size;
    }
    MeshSnapshot(const MeshSnapshot&) = delete;
    size_t nv() const { return xyz.size() / 3; }
    size_t nf() const { return faces.size() / 3; }
    template <class T> const T* add(const char* name, const T* values) {      // one value per vertex; null: zeros
        owned.emplace_back(nv() * sizeof(T), '\0');
        if (values) memcpy(owned.back().data(), values, owned.back().size());
        const T* own = reinterpret_cast<const T*>(owned.back().data());
        columns.push_back(ply_column(name, own));
        return own;
    }
    bool write(const std::string& file, const std::string& comments) const {
        return write_mesh_indexed_ply(file, MeshView{xyz.data(), normals.data(), rgb.data(), nv(), faces.data(), nf()}, origin.data(), vs, comments, columns);
    }
};
using MeshSnapshotPtr = std::shared_ptr<MeshSnapshot>;

// <name>_mesh.ply -> <name>
inline std::string dump_base(const std::string& mesh_file) {
    const std::string tail = "_mesh.ply";
    return mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
}
// onto the queue; --host-writers: written here and now
inline void push_dump(std::function<void()> job) { if (dump_options().host_writers) job(); else DumpQueue::get().push(std::move(job)); }
// one job; false from it: `couldn't save <what> <name>` and one more failure of the run (DumpQueue::failures)
inline void queue_dump(const char* what, const std::string& name, std::function<bool()> job) {
    push_dump([=] { if (!job()) { std::cout << "couldn't save " << what << " " << name << std::endl; DumpQueue::get().report_failure(); } });
}
inline void queue_welded_ply(const std::string& file, MeshSnapshotPtr mesh, const std::string& comments, const char* what, const std::string& name) {
    queue_dump(what, name, [=] { return mesh->write(file, comments); });
}
inline void queue_text(const std::string& file, const std::string& text, const char* what, const std::string& name) {
    queue_dump(what, name, [=] { return save_text(file, text); });
}

// <name>_mesh_indexed.ply: the welded mesh of the same state (include/psgsdf_mesh.h), binary.  A multi-rank run: every rank writes its records at their
// place in the one file, which is byte for byte the single-process file.
inline bool device_mesh_indexed(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: welded mesh (device) + binary PLY");
    const std::string file = dump_base(mesh_file) + "_mesh_indexed.ply";
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; int64_t nv = 0, nf = 0, first = 0;
    const bool ok = psgsdf_extract_mesh_indexed(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &first) == 0;
    if (!ok) { nv = 0; nf = 0; }
    if (multi_rank()) {
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        std::vector<double> before, total;
        if (!scan_over_ranks(ctx, {(double)nv, (double)nf}, before, total, ok) || total[1] == 0) return false;
        const std::string h = mesh_indexed_header((size_t)total[0], (size_t)total[1], info.origin, info.voxel_size);
        auto V = std::make_shared<std::vector<TextOut>>(1); (*V)[0].s = mesh_indexed_vertices(xyz, nrm, rgb, (size_t)nv);
        auto F = std::make_shared<std::vector<TextOut>>(1); (*F)[0].s = mesh_indexed_faces(faces, (size_t)nf);
        const long long fbase = (long long)(h.size() + kPlyVertexBytes * (size_t)total[0]);
        write_shared_file(file, h, fbase + (long long)(kPlyFaceBytes * (size_t)total[1]),
                          {{(long long)(h.size() + kPlyVertexBytes * (size_t)before[0]), V}, {fbase + (long long)(kPlyFaceBytes * (size_t)before[1]), F}});
        return true;
    }
    if (!ok || nf == 0) return false;
    queue_welded_ply(file, std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf), "", "mesh", file);
    return true;
}
// <name>_mesh_clean.ply (one more comment line) + <name>_mesh_components.txt: first_vertex n_vertices n_faces n_edges n_boundary_edges
// n_nonmanifold_edges area lo[3] hi[3] kept, one component per line
inline bool device_mesh_clean(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: mesh components (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vcomp = nullptr;
    const psgsdf_mesh_component* comps = nullptr; int64_t nv = 0, nf = 0, nc = 0;
    if (psgsdf_extract_mesh_components(ctx, &dump_options().mesh_filter, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc) != 0 || nc == 0) return false;
    std::string table; int64_t kept = 0;
    for (int64_t i = 0; i < nc; ++i) {
        const psgsdf_mesh_component& k = comps[i];
        char line[400];
        snprintf(line, sizeof line, "%lld %lld %lld %lld %lld %lld %.17g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", (long long)k.first_vertex, (long long)k.n_vertices, (long long)k.n_faces,
                 (long long)k.n_edges, (long long)k.n_boundary_edges, (long long)k.n_nonmanifold_edges, k.area, (double)k.lo[0], (double)k.lo[1], (double)k.lo[2],
                 (double)k.hi[0], (double)k.hi[1], (double)k.hi[2], (int)k.kept);
        table += line; kept += k.kept;
    }
    const std::string extra = "comment components kept " + std::to_string(kept) + " of " + std::to_string(nc) + "\n";
    auto mesh = std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf);
    queue_dump("the cleaned mesh", base, [=] { const bool ok = mesh->write(base + "_mesh_clean.ply", extra); return save_text(base + "_mesh_components.txt", table) && ok; });
    return true;
}
// <name>_mesh_lod.ply (one more comment line): cell = S voxels of the state's voxel size; with --mesh-bake the textured mesh and its maps in a second job
inline bool device_mesh_lod(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: level-of-detail mesh (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const DumpOptions& opt = dump_options();
    psgsdf_info info{}; psgsdf_get_info(ctx, &info);
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vmap = nullptr;
    int64_t nv = 0, nf = 0, nv_in = 0, nf_in = 0;
    const double cell = opt.lod_voxels * (double)info.voxel_size;
    psgsdf_bake bk{};      // --mesh-bake: the same level-of-detail arrays (bit for bit) and the atlas, in one call
    psgsdf_bake_ao ao{};   // --mesh-bake-ao: the same bake (bit for bit) and the occlusion map
    psgsdf_bake_photo ph{};   // --mesh-bake-photo: the same bake (bit for bit) and the albedo solved from the keyframes
    psgsdf_bake_curvature cv{};   // --mesh-bake-curvature: the same bake (bit for bit) and the mean curvature of the hit voxels
    if (opt.bake_res > 0) {
        bool baked = false;
        if (opt.bake_ao_dirs > 0) {
            const psgsdf_ao_params ap{opt.bake_ao_dirs, 0, 8.0 * (double)info.voxel_size, (double)info.voxel_size};
            if (psgsdf_bake_lod_ao(ctx, opt.filter(), cell, opt.bake_res, cell, &ap, &ao) != 0) return false;
            bk = ao.bake; baked = true;
        }
        if (opt.bake_photo) {      // (behind the occlusion: its map has slots of its own, the bake's are filled again with the same bits)
            const psgsdf_photo_params pp{(double)info.voxel_size, 0.2, 0.05, 0, 0};
            const int rc = psgsdf_bake_lod_photo(ctx, opt.filter(), cell, opt.bake_res, cell, &pp, &ph);
            if (rc == 0) { bk = ph.bake; baked = true; }
            else if (rc != PSGSDF_ERR_STATE) return false;      // (before psgsdf_init: no keyframes yet)
        }
        if (opt.bake_curvature_scale > 0) {      // (likewise: the map in slots of its own, the bake's filled again with the same bits)
            if (psgsdf_bake_lod_curvature(ctx, opt.filter(), cell, opt.bake_res, cell, &cv) != 0) return false;
            bk = cv.bake; baked = true;
        }
        if (!baked && psgsdf_bake_lod(ctx, opt.filter(), cell, opt.bake_res, cell, &bk) != 0) return false;
        if (bk.n_faces_in == 0) return false;
        xyz = bk.xyz; nrm = bk.normals; rgb = bk.rgb; faces = bk.faces; nv = bk.n_vertices; nf = bk.n_faces; nv_in = bk.n_vertices_in; nf_in = bk.n_faces_in;
    } else if (psgsdf_extract_mesh_lod(ctx, opt.filter(), cell, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vmap, &nv_in, &nf_in) != 0
        || nf_in == 0) return false;
    char line[200];
    snprintf(line, sizeof line, "comment lod cell %.9g voxels from %lld vertices %lld faces\n", opt.lod_voxels, (long long)nv_in, (long long)nf_in);
    auto mesh = std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf);
    queue_welded_ply(base + "_mesh_lod.ply", mesh, line, "the level-of-detail mesh", base);
    if (opt.bake_res > 0 && bk.width > 0) {
        const int W = bk.width, H = bk.height; const size_t px = (size_t)W * H;
        auto uv = std::make_shared<std::vector<float>>(bk.uv, bk.uv + 6 * nf);
        struct Map { const char* suffix; int channels; std::vector<uint8_t> px; };      // the maps, in the order they are written
        auto maps = std::make_shared<std::vector<Map>>();
        maps->push_back({"_albedo.png", 3, std::vector<uint8_t>(bk.albedo, bk.albedo + 3 * px)});
        maps->push_back({"_normal.png", 3, std::vector<uint8_t>(3 * px)});
        for (size_t q = 0; q < 3 * px; ++q) maps->back().px[q] = normal_to_u8(bk.normal[q]);
        std::cout << "baked " << bk.n_texels << " texels onto " << nf << " faces (" << W << " x " << H << "): " << bk.n_hits << " hits (" << bk.n_hits_off_band << " off the band), "
                  << bk.n_buried << " buried, " << bk.n_misses << " misses" << std::endl;
        const bool with_ao = opt.bake_ao_dirs > 0 && ao.occlusion, with_photo = ph.photo_rgb != nullptr;
        if (with_ao) {
            maps->push_back({"_ao.png", 1, std::vector<uint8_t>(ao.occlusion, ao.occlusion + px)});
            std::cout << "ambient occlusion: " << ao.counts.n_rays << " rays (" << ao.n_dirs << " per texel), " << ao.counts.n_occluded << " occluded, " << ao.counts.n_buried << " of them buried" << std::endl;
        }
        if (with_photo) {
            maps->push_back({"_photo.png", 3, std::vector<uint8_t>(ph.photo_rgb, ph.photo_rgb + 3 * px)});
            std::cout << "photo albedo: " << ph.counts.n_texels_solved << " of " << ph.counts.n_samples << " texels solved from " << ph.counts.n_used << " of " << ph.counts.n_pairs
                      << " views (" << ph.counts.n_outside << " outside, " << ph.counts.n_grazing << " grazing, " << ph.counts.n_occluded << " occluded, " << ph.counts.n_dark << " dark)" << std::endl;
        }
        if (cv.mean != nullptr) {
            maps->push_back({"_curvature.png", 1, std::vector<uint8_t>(px)});
            for (size_t q = 0; q < px; ++q) maps->back().px[q] = curvature_to_u8(cv.mean[q], cv.valid[q], (double)info.voxel_size, opt.bake_curvature_scale);
            std::cout << "curvature: " << cv.n_valid << " of " << bk.n_hits << " hit texels evaluated" << std::endl;
        }
        queue_dump("the baked level-of-detail mesh", base, [=] {
            const std::string lod = base + "_mesh_lod";
            bool ok = write_obj_bake(lod + ".obj", lod + ".mtl", lod + (with_photo ? "_photo.png" : "_albedo.png"), lod + "_normal.png", mesh->xyz.data(), mesh->normals.data(), mesh->nv(), mesh->faces.data(),
                                     uv->data(), mesh->nf(), with_ao ? lod + "_ao.png" : std::string());
            for (const Map& m : *maps) ok = write_png(lod + m.suffix, W, H, m.channels, m.px.data()) && ok;
            return ok;
        });
    }
    return true;
}
// <name>_mesh_fit.ply.  Before psgsdf_init there is no band: the mesh of psgsdf_extract_mesh_indexed with zeros
inline bool device_mesh_fit(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: welded mesh with vertex fit (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr;
    const int32_t* vn_obs = nullptr; const float* vrms = nullptr; const float* vloss = nullptr; int64_t nv = 0, nf = 0, first = 0;
    const int rc = psgsdf_extract_mesh_fit(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vn_obs, &vrms, &vloss);
    if (rc == PSGSDF_ERR_STATE) { if (psgsdf_extract_mesh_indexed(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &first) != 0) return false; vn_obs = nullptr; vrms = vloss = nullptr; }
    else if (rc != 0) return false;
    if (nf == 0) return false;
    auto mesh = std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf);
    const float* rms = mesh->add("quality", vrms); mesh->add("loss", vloss); const int32_t* n_obs = mesh->add("n_obs", vn_obs);
    queue_welded_ply(base + "_mesh_fit.ply", mesh, mesh_fit_comment(rms, n_obs, (size_t)nv), "the mesh with its fit", base);
    return true;
}
// <name>_mesh_curvature.ply
inline bool device_mesh_curvature(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: welded mesh with vertex curvature (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr;
    const uint8_t* valid = nullptr; const float *mean = nullptr, *gauss = nullptr, *k1 = nullptr, *k2 = nullptr; int64_t nv = 0, nf = 0;
    if (psgsdf_extract_mesh_curvature(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &valid, &mean, &gauss, &k1, &k2) != 0 || nf == 0) return false;
    auto mesh = std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf);
    mesh->add("quality", mean); mesh->add("gauss", gauss); mesh->add("k1", k1); mesh->add("k2", k2); mesh->add("curvature_valid", valid);
    queue_welded_ply(base + "_mesh_curvature.ply", mesh, mesh_curvature_comment(mean, valid, (size_t)nv), "the mesh with its curvature", base);
    return true;
}
// <name>_mesh_filled.ply: three calls -- the components of the state as it is (for the boundary edges the filling starts from), the filled voxels
// (for their number), the mesh of the filled state
inline bool device_mesh_filled(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: welded mesh of the filled state (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const int R = dump_options().fill_rounds, K = dump_options().fill_sweeps;
    const psgsdf_mesh_filter* flt = dump_options().filter();
    const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vcomp = nullptr;
    const psgsdf_mesh_component* comps = nullptr; const uint8_t* filled = nullptr; int64_t nv = 0, nf = 0, nc = 0;
    auto boundary = [&] { long long b = 0; for (int64_t i = 0; i < nc; ++i) if (comps[i].kept) b += comps[i].n_boundary_edges; return b; };
    if (psgsdf_extract_mesh_components(ctx, flt, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc) != 0) return false;
    const long long before = boundary();
    const int64_t* lin = nullptr; const float *fd = nullptr, *fg = nullptr, *fc = nullptr; const uint8_t* fr = nullptr; int64_t n_filled = 0;
    if (psgsdf_fill_voxels(ctx, R, K, &lin, &fd, &fg, &fc, &fr, &n_filled) != 0) return false;
    if (psgsdf_extract_mesh_filled(ctx, R, K, flt, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc, &filled) != 0 || nf == 0) return false;
    auto mesh = std::make_shared<MeshSnapshot>(ctx, xyz, nrm, rgb, nv, faces, nf);
    mesh->add("filled", filled);
    queue_welded_ply(base + "_mesh_filled.ply", mesh, mesh_filled_comment(R, K, (long long)n_filled, before, boundary()), "the filled mesh", base);
    return true;
}
// <name>_compare.txt + <name>_mesh_compare.ply: the welded mesh (with a filter flag: its kept components) against the reference of --compare-ply.  The
// text file, one record per line, every length in voxels and in metres:
//   reference FILE points N faces F / voxel_size VS max_dist_voxels D tau_voxels T
//   per direction (to_reference, to_reconstruction) three lines: the counts; mean, rms, max and signed mean; the histogram's 16 bins
//   precision P recall R fscore F
inline bool device_mesh_compare(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: comparison with the reference (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const CompareRef& ref = dump_options().compare;
    psgsdf_info info{}; psgsdf_get_info(ctx, &info);
    const double vsd = (double)info.voxel_size;
    psgsdf_compare_params p{}; p.max_dist = ref.max_voxels * vsd; p.tau = ref.tau_voxels * vsd;
    psgsdf_compare r{};
    const int64_t n_ref = (int64_t)(ref.xyz.size() / 3), n_ref_faces = (int64_t)(ref.faces.size() / 3);
    const float* ref_xyz = ref.xyz.data();
    std::vector<float> aligned;      // --compare-align: the reference under the transform found for THIS dump (a copy: the engine's array lives until the next extraction call)
    if (ref.align) {
        auto al = std::make_unique<psgsdf_align>();
        psgsdf_align_params ap{};
        for (int i = 0; i < 4; ++i) ap.init[5 * i] = 1.0;
        ap.max_dist = p.max_dist; ap.min_dist = std::min(vsd, p.max_dist); ap.shrink = 1.0; ap.eps_rot = 1e-5; ap.eps_trans = 1e-3 * vsd; ap.directions = 3; ap.max_iters = ref.align_iters;
        if (psgsdf_align_reference(ctx, dump_options().filter(), ref.xyz.data(), n_ref, ref.faces.data(), n_ref_faces, &ap, al.get()) != 0) return false;
        aligned.assign(al->aligned_xyz, al->aligned_xyz + 3 * n_ref);
        ref_xyz = aligned.data();
        static const char* const words[4] = {"converged", "max_iters", "degenerate", "too_few"};
        char ln[1200]; std::string at;
        snprintf(ln, sizeof ln, "status %s iterations %d\nreference %s points %lld faces %lld\nvoxel_size %.9g max_dist_voxels %.17g max_iters %d\n", words[al->status & 3], (int)al->n_iters, ref.file.c_str(),
                 (long long)n_ref, (long long)n_ref_faces, vsd, ref.max_voxels, ref.align_iters);
        at += ln;
        for (int k = 0; k < al->n_iters; ++k) {
            const psgsdf_align_iter& it = al->iters[k];
            snprintf(ln, sizeof ln, "iter %d radius_voxels %.17g rms_voxels %.17g pairs %lld %lld min_pivot %.17g step %.17g %.17g %.17g %.17g %.17g %.17g\n", k, it.radius / vsd, it.rms / vsd, (long long)it.n_pairs[0],
                     (long long)it.n_pairs[1], it.min_pivot, it.step[0], it.step[1], it.step[2], it.step[3], it.step[4], it.step[5]);
            at += ln;
        }
        snprintf(ln, sizeof ln, "final radius_voxels %.17g rms_voxels %.17g pairs %lld %lld\ntransform\n", al->final.radius / vsd, al->final.rms / vsd, (long long)al->final.n_pairs[0], (long long)al->final.n_pairs[1]);
        at += ln;
        for (int i = 0; i < 4; ++i) { snprintf(ln, sizeof ln, "%.17g %.17g %.17g %.17g\n", al->transform[4 * i], al->transform[4 * i + 1], al->transform[4 * i + 2], al->transform[4 * i + 3]); at += ln; }
        queue_text(base + "_align.txt", at, "the alignment", base);
    }
    if (psgsdf_compare_reference(ctx, dump_options().filter(), ref_xyz, n_ref, ref.faces.data(), n_ref_faces, &p, &r) != 0) return false;
    char line[1200]; std::string txt;
    snprintf(line, sizeof line, "reference %s points %lld faces %lld\nvoxel_size %.9g max_dist_voxels %.17g tau_voxels %.17g\n", ref.file.c_str(), (long long)n_ref, (long long)n_ref_faces, vsd, ref.max_voxels, ref.tau_voxels);
    txt += line;
    const psgsdf_compare_side* sides[2] = {&r.to_reference, &r.to_reconstruction};
    for (int d = 0; d < 2; ++d) {
        const psgsdf_compare_side& s = *sides[d]; const char* name = d ? "to_reconstruction" : "to_reference";
        snprintf(line, sizeof line, "%s n %lld n_valid %lld n_matched %lld n_within_tau %lld\n"
                 "%s mean_voxels %.17g mean %.17g rms_voxels %.17g rms %.17g max_voxels %.17g max %.17g mean_signed_voxels %.17g mean_signed %.17g\n%s hist", name, (long long)s.n, (long long)s.n_valid,
                 (long long)s.n_matched, (long long)s.n_within_tau, name, s.mean / vsd, s.mean, s.rms / vsd, s.rms, s.max / vsd, s.max, s.mean_signed / vsd, s.mean_signed, name);
        txt += line;
        for (int b = 0; b < 16; ++b) txt += " " + std::to_string((long long)s.hist[b]);
        txt += "\n";
    }
    snprintf(line, sizeof line, "precision %.17g recall %.17g fscore %.17g\n", r.precision, r.recall, r.fscore);
    txt += line;
    snprintf(line, sizeof line, "comment compare precision %.9g recall %.9g fscore %.9g tau %.9g max_dist %.9g\n", r.precision, r.recall, r.fscore, p.tau, p.max_dist);
    const std::string extra = line;
    auto mesh = std::make_shared<MeshSnapshot>(ctx, r.xyz, r.normals, r.rgb, r.n_vertices, r.faces, r.n_faces);
    mesh->add("distance", r.vertex_dist); mesh->add("side", r.vertex_side);
    queue_dump("the comparison", base, [=] {
        bool ok = save_text(base + "_compare.txt", txt);
        if (mesh->nf() > 0) ok = mesh->write(base + "_mesh_compare.ply", extra) && ok;
        return ok;
    });
    return true;
}
// <name>_query.ply: the points of --query-ply with the field there, or projected onto the surface (the columns: ply_io.hpp)
inline bool device_query(psgsdf_ctx* ctx, const std::string& mesh_file) {
    PSG_STAGE("dump: field queries (device) + binary PLY");
    const std::string base = dump_base(mesh_file);
    const QueryRef& q = dump_options().query;
    psgsdf_info info{}; psgsdf_get_info(ctx, &info);
    const int64_t n = (int64_t)(q.xyz.size() / 3);
    const size_t N = (size_t)n;
    struct Cloud { std::vector<float> xyz; std::vector<std::vector<float>> f; std::vector<std::vector<uint8_t>> b; std::vector<PlyColumn> columns; std::array<float, 3> origin; float vs; };
    auto cloud = std::make_shared<Cloud>();
    cloud->origin = {info.origin[0], info.origin[1], info.origin[2]}; cloud->vs = info.voxel_size;
    // one float column of an [n][stride] array / one byte column; the float columns go first in the file, in the order they are added
    std::vector<const char*> fnames, bnames;
    auto column_f = [&](const char* name, const float* src, size_t stride) {
        fnames.push_back(name); cloud->f.emplace_back(N);
        for (size_t i = 0; i < N; ++i) cloud->f.back()[i] = src[i * stride];
    };
    auto column_b = [&](const char* name, const uint8_t* src) { bnames.push_back(name); cloud->b.emplace_back(src, src + N); };
    const char* model = q.model == PSGSDF_Q_CELL ? "cell" : "trilinear";
    char line[300];
    if (q.project) {
        psgsdf_project_params p{}; p.model = q.model; p.max_iters = 16; p.tol = 1e-3 * (double)info.voxel_size;
        const uint8_t *st = nullptr, *it = nullptr; const float *xyz = nullptr, *res = nullptr, *nrm = nullptr, *moved = nullptr; const int64_t* vox = nullptr; psgsdf_project_counts c{};
        if (psgsdf_project_points(ctx, q.xyz.data(), n, &p, &st, &xyz, &res, &nrm, &vox, &it, &moved, &c) != 0) return false;
        if (n > 0) cloud->xyz.assign(xyz, xyz + 3 * N);
        column_f("distance", moved, 1); column_f("residual", res, 1); column_b("iterations", it); column_b("status", st);
        snprintf(line, sizeof line, "comment query project model %s points %lld converged %lld left %lld not_converged %lld invalid %lld\n", model, (long long)c.n, (long long)c.n_converged,
                 (long long)c.n_left, (long long)c.n_not_converged, (long long)c.n_invalid);
    } else {
        const uint8_t* st = nullptr; const float *d = nullptr, *nrm = nullptr, *rgb = nullptr, *w = nullptr; const int64_t* vox = nullptr; psgsdf_query_counts c{};
        if (psgsdf_query_points(ctx, q.xyz.data(), n, q.model, &st, &d, &nrm, &rgb, &w, &vox, &c) != 0) return false;
        cloud->xyz = q.xyz;
        static const char* const nn[3] = {"nx", "ny", "nz"}; static const char* const cc[3] = {"red", "green", "blue"};
        column_f("distance", d, 1);
        for (int k = 0; k < 3; ++k) column_f(nn[k], nrm + k, 3);
        for (int k = 0; k < 3; ++k) column_f(cc[k], rgb + k, 3);
        column_f("weight", w, 1); column_b("status", st);
        snprintf(line, sizeof line, "comment query points model %s points %lld ok %lld outside %lld unobserved %lld invalid %lld\n", model, (long long)c.n, (long long)c.n_ok, (long long)c.n_outside,
                 (long long)c.n_unobserved, (long long)c.n_invalid);
    }
    for (size_t k = 0; k < fnames.size(); ++k) cloud->columns.push_back(ply_column(fnames[k], cloud->f[k].data()));
    for (size_t k = 0; k < bnames.size(); ++k) cloud->columns.push_back(ply_column(bnames[k], cloud->b[k].data()));
    const std::string comment = line;
    queue_dump("the queries", base, [=] { return write_points_ply(base + "_query.ply", cloud->xyz.data(), N, cloud->origin.data(), cloud->vs, comment, cloud->columns); });
    return true;
}
// every dump that goes with a <name>_mesh.ply, in the order the engine is to be called in (its results are valid until the next extraction); one that
// queued nothing: `couldn't save <what> <label>`
inline void device_mesh_extras(psgsdf_ctx* ctx, const std::string& mesh_file, const std::string& label) {
    const DumpOptions& o = dump_options();
    const struct { bool on; bool (*dump)(psgsdf_ctx*, const std::string&); const char* what; } extras[] = {
        {o.indexed_mesh, device_mesh_indexed, "the indexed mesh"}, {o.clean_mesh, device_mesh_clean, "the cleaned mesh"}, {o.lod_voxels > 0, device_mesh_lod, "the level-of-detail mesh"},
        {o.fit, device_mesh_fit, "the mesh with its fit"}, {o.curvature, device_mesh_curvature, "the mesh with its curvature"}, {o.fill_rounds >= 0, device_mesh_filled, "the filled mesh"},
        {o.compare.on, device_mesh_compare, "the comparison"}, {o.query.on, device_query, "the queries"}};
    for (const auto& e : extras) if (e.on && !e.dump(ctx, mesh_file)) std::cout << "couldn't save " << e.what << " " << label << std::endl;
}
// the reference's own dumps from the device: <name>_mesh.ply (MarchingCubes::savePly's text), the point clouds, the SDF block
inline bool device_mesh(psgsdf_ctx* ctx, const std::string& file) {
    const float* xyz = nullptr; const uint8_t* rgb = nullptr; int64_t nv = 0;
    const bool ok = psgsdf_extract_mesh(ctx, &xyz, &rgb, &nv) == 0;
    if (!ok) nv = 0;
    if (multi_rank()) {
        std::vector<double> before, total;
        if (!scan_over_ranks(ctx, {(double)nv}, before, total, ok) || total[0] == 0) return false;
        auto V = std::make_shared<std::vector<TextOut>>(format_lines((size_t)nv, 40, [&](TextOut& o, size_t i) { mesh_vertex_line(o, xyz, rgb, i); }));
        const size_t face0 = (size_t)before[0] / 3;      // (faces are numbered through the whole file)
        auto F = std::make_shared<std::vector<TextOut>>(format_lines((size_t)nv / 3, 24, [&](TextOut& o, size_t q) { mesh_face_line(o, face0 + q); }));
        const std::string h = mesh_header((size_t)total[0]);
        std::vector<double> bb, bt;
        if (!scan_over_ranks(ctx, {(double)bytes_of(*V), (double)bytes_of(*F)}, bb, bt)) return false;
        write_shared_file(file, h, (long long)(h.size() + bt[0] + bt[1]), {{(long long)(h.size() + bb[0]), V}, {(long long)(h.size() + bt[0] + bb[1]), F}});
        return true;
    }
    if (!ok || nv == 0) return false;
    auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv); auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv);
    push_dump([=] { if (!write_mesh_ply(file, vx->data(), vc->data(), (size_t)nv)) std::cout << "couldn't save mesh " << file << std::endl; });
    return true;
}
inline bool device_pointcloud(psgsdf_ctx* ctx, int which, const std::string& file) {
    const float* pn = nullptr; const int32_t* col = nullptr; int64_t n = 0;
    const bool ok = psgsdf_extract_pointcloud(ctx, which, &pn, &col, &n) == 0;
    if (!ok) n = 0;
    if (multi_rank()) {
        auto L = std::make_shared<std::vector<TextOut>>(format_lines((size_t)n, 80, [&](TextOut& o, size_t i) { pointcloud_line(o, pn, col, i); }));
        std::vector<double> before, total;
        if (!scan_over_ranks(ctx, {(double)n, (double)bytes_of(*L)}, before, total, ok)) return false;
        const std::string h = pointcloud_header((size_t)total[0]);
        write_shared_file(file, h, (long long)(h.size() + total[1]), {{(long long)(h.size() + before[1]), L}});
        return true;
    }
    if (!ok) return false;
    auto vp = std::make_shared<std::vector<float>>(pn, pn + 6 * n); auto vc = std::make_shared<std::vector<int32_t>>(col, col + 3 * n);
    push_dump([=] { if (!write_pointcloud_ply(file, vp->data(), vc->data(), (size_t)n)) std::cout << " can't save point cloud!" << std::endl; });
    return true;
}
inline bool device_sdf(psgsdf_ctx* ctx, const std::string& file, float vs) {
    int32_t lo[3], dim[3]; const float* v = nullptr;
    bool ok = psgsdf_extract_sdf(ctx, lo, dim, &v) == 0;
    if (multi_rank()) {
        int32_t mi[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (ok && psgsdf_mg_info(ctx, mi)) ok = false;
        if (!ok) dim[0] = dim[1] = dim[2] = lo[0] = lo[1] = lo[2] = 0;
        const size_t cnt = (size_t)dim[0] * dim[1] * (size_t)std::max(0, std::min(lo[2] + dim[2], mi[11]) - std::max(lo[2], mi[10]));      // the planes of the box this rank owns
        auto L = std::make_shared<std::vector<TextOut>>(format_lines(cnt, 12, [&](TextOut& o, size_t i) { o.f(v[i]); o.c('\n'); }));
        std::vector<double> before, total;
        if (!scan_over_ranks(ctx, {(double)bytes_of(*L)}, before, total, ok)) return false;
        if (dim[0] == 0) return false;      // (the crop box is the whole volume's: empty on every rank alike)
        const int l3[3] = {lo[0], lo[1], lo[2]}, d3[3] = {dim[0], dim[1], dim[2]};
        const std::string h = sdf_header(l3, d3, vs);
        write_shared_file(file, h, (long long)(h.size() + total[0]), {{(long long)(h.size() + before[0]), L}});
        return true;
    }
    if (!ok || !v) return false;
    auto vv = std::make_shared<std::vector<float>>(v, v + (size_t)dim[0] * dim[1] * dim[2]);
    const std::array<int, 3> l{lo[0], lo[1], lo[2]}, d{dim[0], dim[1], dim[2]};
    push_dump([=] { write_sdf_block(file, l.data(), d.data(), vs, vv->data()); });
    return true;
}

}  // namespace psgsdf_host
