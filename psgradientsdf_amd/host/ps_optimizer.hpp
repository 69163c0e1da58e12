// ps_optimizer.hpp — C++ mirror of the reference's optimiser interface over the C ABI (include/psgsdf.h).
//
// Same class / member names, argument meaning and return conventions as
//   ps_optimizer/Optimizer.h:24-182, PsOptimizer.h, LedOptimizer.h, OptimizerSettings.h:24-51
// so that main_ps.cpp:193-202,323-330 reads the same against this header.  The reference's Eigen / OpenCV
// types are replaced by plain structs (none of those libraries is a dependency of this project):
//   Eigen::Matrix4f  -> Mat4f   (row-major 16 floats)        cv::Mat (CV_32FC3, BGR) -> ImageRGB (float RGB)
//   VolumetricGradSdf -> VolumetricGradSdf below: the SoA form of its private tsdf_/vis_ arrays, which the
//   reference's optimisers reach through `friend` access (VolumetricGradSdf.h:25-42).
// All numerical work happens in libpsgsdf.so on the GPU; this header only marshals and writes the text files
// the reference writes from inside alternatingOptimize (optimizer_doc.txt, after_poses_opt_<k>.txt,
// *_pointcloud.ply).  Mesh extraction (marching cubes) is a SURVEY §8f "next" row and not part of it.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <atomic>
#include <thread>
#include <cstdint>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/psgsdf.h"
#include "../../include/psgsdf_render.h"
#include "../../include/psgsdf_relight.h"
#include "../../include/psgsdf_mesh.h"
#include "../../include/psgsdf_fit.h"
#include "../../include/psgsdf_bake.h"
#include "../../include/psgsdf_occlusion.h"
#include "../../include/psgsdf_photo.h"
#include "../../include/psgsdf_compare.h"
#include "../../include/psgsdf_align.h"
#include "../../include/psgsdf_curvature.h"
#include "../../include/psgsdf_fill.h"
#include "marching_cubes.hpp"
#include "png_writer.hpp"
#include "obj_writer.hpp"

namespace psgsdf_host {

// Wall-clock per stage of a voxelPS run (`voxelPS --timing <file.json>`: VERDICT r04 item 4 -- the Gauss-Newton iterations are milliseconds, the
// decode / fusion / dump stages around them are what a user waits for).  Scopes nest: a stage's time includes the stages opened inside it.
struct StageClock {
    std::vector<std::pair<std::string, double>> acc; std::vector<long long> calls; std::mutex mu;      // (the background writer thread books its stages too)
    size_t slot(const std::string& n) { std::lock_guard<std::mutex> g(mu); for (size_t i = 0; i < acc.size(); ++i) if (acc[i].first == n) return i; acc.emplace_back(n, 0.0); calls.push_back(0); return acc.size() - 1; }
    struct Scope {
        StageClock& c; size_t i; std::chrono::steady_clock::time_point t0;
        Scope(StageClock& c_, const std::string& n) : c(c_), i(c_.slot(n)), t0(std::chrono::steady_clock::now()) {}
        ~Scope() { const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); std::lock_guard<std::mutex> g(c.mu); c.acc[i].second += dt; c.calls[i] += 1; }
    };
    static StageClock& get() { static StageClock c; return c; }
    double of(const std::string& n) { return acc[slot(n)].second; }
    bool write_json(const std::string& path, const std::string& extra = "") {
        std::ofstream f(path.c_str()); if (!f.is_open()) return false;
        f << "{\"stages_s\": {";
        for (size_t i = 0; i < acc.size(); ++i) f << (i ? ", " : "") << "\"" << acc[i].first << "\": " << acc[i].second;
        f << "}, \"calls\": {";
        for (size_t i = 0; i < acc.size(); ++i) f << (i ? ", " : "") << "\"" << acc[i].first << "\": " << calls[i];
        f << "}" << extra << "}\n";
        return true;
    }
};
#define PSG_STAGE_CAT2(a, b) a##b
#define PSG_STAGE_CAT(a, b) PSG_STAGE_CAT2(a, b)
#define PSG_STAGE(name) ::psgsdf_host::StageClock::Scope PSG_STAGE_CAT(psg_stage_, __LINE__)(::psgsdf_host::StageClock::get(), name)

using Mat4f = std::array<float, 16>;                 // row-major camera->world
struct Mat3f { float v[9]; };                        // row-major intrinsics
struct ImageRGB { int rows = 0, cols = 0; std::vector<float> data; };   // rows*cols*3, RGB in [0,1]

enum LossFunction { L2 = 0, CAUCHY = 1, HUBER = 2, TUKEY = 3, TRUNC_L2 = 4 };   // OptimizerSettings.h:9-16
enum ModelType { SH1, SH2, LED };                                               // OptimizerSettings.h:18-22

struct OptimizerSettings {                           // OptimizerSettings.h:24-51 (same defaults)
    int max_it = 100;
    float conv_threshold = 1e-4f;
    float damping = 1.0f;
    float lambda = 0.5f;
    float lambda_sq = 0.25f;
    float reg_weight_rho = 0.0f, reg_weight_n = 0.0f, reg_weight_l = 0.0f;
    int order = 1;
    bool upsample = false;
    ModelType model = SH1;
    LossFunction loss = CAUCHY;
};

// ---- the ASCII writers -----------------------------------------------------------------------------------------------------------------
// The reference prints every number through `ostream << float`, i.e. printf's %g with six significant digits, one std::endl (= a flush) per line;
// its files are tens of MB of that.  Same characters here, from snprintf into per-thread buffers (the lines of a file are formatted in parallel
// chunks and written in order), on a background thread, so that the optimisation goes on while a dump is being formatted.
inline bool& host_writers() { static bool v = false; return v; }
inline bool& indexed_mesh() { static bool v = false; return v; }      // voxelPS --indexed-mesh: a <name>_mesh_indexed.ply (psgsdf_extract_mesh_indexed) next to every <name>_mesh.ply
// voxelPS --mesh-min-faces N / --mesh-keep-largest K: next to every <name>_mesh.ply a <name>_mesh_clean.ply (the welded mesh without the connected components
// the filter drops, psgsdf_extract_mesh_components) and a <name>_mesh_components.txt (every component, one per line); single process only
inline bool& clean_mesh() { static bool v = false; return v; }
inline psgsdf_mesh_filter& mesh_filter() { static psgsdf_mesh_filter f{0, 0.0, 0}; return f; }
// voxelPS --mesh-lod S: next to every <name>_mesh.ply a <name>_mesh_lod.ply, the welded mesh (the filtered one, if a filter flag is given) with the vertices
// of every cube of S voxels merged into one (psgsdf_extract_mesh_lod); 0: off; single process only
inline double& mesh_lod_voxels() { static double v = 0.0; return v; }
// voxelPS --mesh-bake R (with --mesh-lod S): next to every <name>_mesh_lod.ply the same mesh as <name>_mesh_lod.obj / .mtl with the reconstruction's detail
// baked into <name>_mesh_lod_albedo.png and <name>_mesh_lod_normal.png (object space), R texels along a triangle's edge, rays from one cell outside
// (psgsdf_bake_lod); 0: off; single process only
inline int& mesh_bake_res() { static int v = 0; return v; }
// voxelPS --mesh-bake-ao K (with --mesh-bake): <name>_mesh_lod_ao.png next to the other maps (grey, 255 = open) and one `map_Ka` line in the .mtl: the
// ambient occlusion of the reconstructed surface from K rays per texel, radius 8 voxels, origins 1 voxel off the surface (psgsdf_bake_lod_ao); 0: off
inline int& mesh_bake_ao_dirs() { static int v = 0; return v; }
// voxelPS --mesh-bake-photo (with --mesh-bake): <name>_mesh_lod_photo.png next to the other maps, the albedo of every texel solved from the keyframes that
// see it (psgsdf_bake_lod_photo: rays lifted 1 voxel, cos_min 0.2, shade_min 0.05), and `map_Kd` in the .mtl names it; _albedo.png is still written.  A
// dump taken before psgsdf_init (the fused volume's) has no keyframes to solve from and is baked as without the flag
inline bool& mesh_bake_photo() { static bool v = false; return v; }
// voxelPS --mesh-fit: next to every <name>_mesh.ply a <name>_mesh_fit.ply, the welded mesh with the photometric fit of every vertex (psgsdf_extract_mesh_fit): how many
// keyframes saw it, the rms residual and the mean robust loss; single process only
inline bool& mesh_fit() { static bool v = false; return v; }
// voxelPS --mesh-curvature: next to every <name>_mesh.ply a <name>_mesh_curvature.ply, the welded mesh with the curvature of every vertex
// (psgsdf_extract_mesh_curvature): mean, Gaussian and the two principal curvatures, and how many of its end voxels could be evaluated; single process only
inline bool& mesh_curvature() { static bool v = false; return v; }
// voxelPS --mesh-bake-curvature S (with --mesh-bake): <name>_mesh_lod_curvature.png next to the other maps, 8-bit grey: the mean curvature of every hit
// texel's voxel (psgsdf_bake_lod_curvature), mean * vs = S white, -S black, flat and every texel without a value 128; convex is bright; 0: off
inline double& mesh_bake_curvature_scale() { static double v = 0.0; return v; }
inline uint8_t curvature_to_u8(float mean, uint8_t valid, double vs, double S) {
    if (!valid) return 128;
    const double x = 0.5 + 0.5 * (double)mean * vs / S;
    return (uint8_t)std::floor(255.0 * (!(x > 0.0) ? 0.0 : x > 1.0 ? 1.0 : x) + 0.5);
}
// voxelPS --mesh-fill R [--mesh-fill-sweeps K]: next to every <name>_mesh.ply a <name>_mesh_filled.ply, the welded mesh of the state with its unobserved
// voxels filled over R rounds and K relaxation sweeps (psgsdf_extract_mesh_filled; the filter flags apply to it) and how many of every vertex's end
// voxels are filled; -1: off; single process only
inline int& mesh_fill_rounds() { static int v = -1; return v; }
inline int& mesh_fill_sweeps() { static int v = 4; return v; }
// voxelPS --compare-ply FILE [--compare-tau T] [--compare-max D]: next to every <name>_mesh.ply a <name>_compare.txt (both directions' counts, mean / rms /
// max / signed mean, histogram, precision / recall / F) and a <name>_mesh_compare.ply (the welded mesh -- the filtered one, if a filter flag is given --
// with every vertex's distance to the reference and the side it lies on): psgsdf_compare_reference against the mesh or cloud read from FILE, whose
// coordinates are those of <name>_mesh_indexed.ply (the mesh's units: that writer adds no offset); T and D in voxels; single process only
// --compare-align [--compare-align-iters K]: before each comparison the reference is aligned to that dump's mesh from the identity (psgsdf_align_reference:
// both directions, the filter flags applied, the radius of --compare-max, at most K = 30 steps), the comparison runs on the aligned points, and a
// <name>_align.txt is written next to <name>_compare.txt: the status word, one line per iteration, the final evaluation, the 4x4 transform with %.17g
struct CompareRef { bool on = false; std::string file; std::vector<float> xyz; std::vector<int32_t> faces; double tau_voxels = 1.0, max_voxels = 8.0; bool align = false; int align_iters = 30; };
inline CompareRef& compare_ref() { static CompareRef r; return r; }
// `voxelPS --relight FILE`: the lights of the file (include/psgsdf_relight.h), bias and reach in voxels
struct RelightSpec { bool on = false; double bias_voxels = 1.0, reach_voxels = 0.0; std::vector<psgsdf_light> lights; };
inline RelightSpec& relight_spec() { static RelightSpec r; return r; }
// voxelPS reads nothing of the refined volume after alternatingOptimize (main_ps.cpp:330-343 ends there): the executable skips the whole-volume download
// that mirrors the reference's in-place mutation of tSDF_ (a host that goes on using tSDF_ keeps it: the default)
inline bool& skip_sync_back() { static bool v = false; return v; }      // voxelPS --host-writers: round 4's path (dense download, host marching cubes, iostream): the cross-check
// printf's "%g" (six significant digits, trailing zeros stripped, scientific below 1e-4 and from 1e6) without printf: a dump is 3-5 million numbers and
// snprintf takes ~150 ns for each.  The float is exact in a double; scaled by an EXACT power of ten (10^0 .. 10^22) the product is off by at most one
// rounding (1.1e-16 relative, < 2e-10 at six digits), so the six digits are decided unless the value sits within 1e-6 of a rounding tie -- those, the
// non-finite values and the exponents outside the exact powers' reach go to snprintf.  `voxelPS --selftest-fmt N` compares with `ostream << float`.
inline int format_g6(float v, char* out) {
    static const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    char* o = out;
    if (v == 0.0f) { if (std::signbit(v)) *o++ = '-'; *o++ = '0'; return (int)(o - out); }
    if (!std::isfinite(v)) return -1;
    const double a = std::fabs((double)v);
    int e2; std::frexp(a, &e2);
    int X = (int)std::floor((e2 - 1) * 0.30102999566398120);      // floor(log10(a)) or one less
    double x;
    for (int tries = 0;; ++tries) {
        const int sh = 5 - X;                                       // a * 10^sh in [1e5, 1e6)
        if (sh < -22 || sh > 22 || tries > 3) return -1;
        x = sh >= 0 ? a * p10[sh] : a / p10[-sh];
        if (x < 1e5) { --X; continue; }
        if (x >= 1e6) { ++X; continue; }
        break;
    }
    const double fl = std::floor(x), fr = x - fl;
    if (std::fabs(fr - 0.5) < 1e-6) return -1;                    // too close to a tie for this arithmetic to call
    long D = (long)fl + (fr > 0.5 ? 1 : 0);
    if (D >= 1000000) { D = 100000; ++X; }
    char d[6]; for (int k = 5; k >= 0; --k) { d[k] = (char)('0' + D % 10); D /= 10; }
    int nd = 6; while (nd > 1 && d[nd - 1] == '0') --nd;
    if (std::signbit(v)) *o++ = '-';
    if (X < -4 || X >= 6) {
        *o++ = d[0];
        if (nd > 1) { *o++ = '.'; for (int k = 1; k < nd; ++k) *o++ = d[k]; }
        *o++ = 'e'; *o++ = X < 0 ? '-' : '+';
        const int ax = X < 0 ? -X : X;
        if (ax >= 100) *o++ = (char)('0' + ax / 100);
        *o++ = (char)('0' + (ax / 10) % 10); *o++ = (char)('0' + ax % 10);
    } else if (X >= 0) {
        for (int k = 0; k <= X; ++k) *o++ = k < nd ? d[k] : '0';
        if (nd > X + 1) { *o++ = '.'; for (int k = X + 1; k < nd; ++k) *o++ = d[k]; }
    } else {
        *o++ = '0'; *o++ = '.';
        for (int k = 0; k < -X - 1; ++k) *o++ = '0';
        for (int k = 0; k < nd; ++k) *o++ = d[k];
    }
    return (int)(o - out);
}
struct TextOut {
    std::string s;
    void f(float v) { char t[40]; int n = format_g6(v, t); if (n < 0) n = snprintf(t, sizeof t, "%g", (double)v); s.append(t, (size_t)n); }
    void i(long long v) {
        char t[24]; int n = 24; unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { t[--n] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) t[--n] = '-';
        s.append(t + n, (size_t)(24 - n));
    }
    void c(char ch) { s.push_back(ch); }
};
// n lines, line(out, i) appends line i; formatted on up to 16 threads, in order
template <class Fn>
inline std::vector<TextOut> format_lines(size_t n, size_t approx_line_bytes, Fn line) {
    unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < 50000) T = 1;
    std::vector<TextOut> parts(T);
    auto work = [&](unsigned t) { const size_t a = n * t / T, b = n * (t + 1) / T; parts[t].s.reserve((b - a) * approx_line_bytes); for (size_t q = a; q < b; ++q) line(parts[t], q); };
    if (T == 1) work(0);
    else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(work, t); for (auto& x : th) x.join(); }
    return parts;
}
template <class Fn>
inline bool write_lines(FILE* f, size_t n, size_t approx_line_bytes, Fn line) {
    for (auto& p : format_lines(n, approx_line_bytes, line)) if (!p.s.empty() && fwrite(p.s.data(), 1, p.s.size(), f) != p.s.size()) return false;
    return true;
}
inline void mesh_vertex_line(TextOut& o, const float* xyz, const uint8_t* rgb, size_t i) { o.f(xyz[3 * i]); o.c(' '); o.f(xyz[3 * i + 1]); o.c(' '); o.f(xyz[3 * i + 2]); o.c(' '); o.i(rgb[3 * i]); o.c(' '); o.i(rgb[3 * i + 1]); o.c(' '); o.i(rgb[3 * i + 2]); o.c('\n'); }
inline void mesh_face_line(TextOut& o, size_t q) { o.c('3'); o.c(' '); o.i((long long)(3 * q)); o.c(' '); o.i((long long)(3 * q + 1)); o.c(' '); o.i((long long)(3 * q + 2)); o.c('\n'); }
inline void pointcloud_line(TextOut& o, const float* pn, const int32_t* col, size_t i) { for (int k = 0; k < 6; ++k) { o.f(pn[6 * i + k]); o.c(' '); } o.i(col[3 * i]); o.c(' '); o.i(col[3 * i + 1]); o.c(' '); o.i(col[3 * i + 2]); o.c('\n'); }
inline std::string mesh_header(size_t nv) {
    char h[400]; const int n = snprintf(h, sizeof h, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               "element face %d\nproperty list uchar int vertex_indices\nend_header\n", nv, (int)(nv / 3));
    return std::string(h, (size_t)n);
}
inline std::string pointcloud_header(size_t n) {
    char h[400]; const int k = snprintf(h, sizeof h, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", n);
    return std::string(h, (size_t)k);
}
inline std::string sdf_header(const int lo[3], const int dim[3], float vs) {
    TextOut h; h.i(dim[0]); h.c(' '); h.i(dim[1]); h.c(' '); h.i(dim[2]); h.c('\n'); h.f(lo[0] * vs); h.c(' '); h.f(lo[1] * vs); h.c(' '); h.f(lo[2] * vs); h.c('\n'); h.f(vs); h.c('\n');
    return h.s;
}
// MarchingCubes::savePly (third/mesh/MarchingCubes.cpp:659-699) from non-indexed vertices: 3 per face
inline bool write_mesh_ply(const std::string& file, const float* xyz, const uint8_t* rgb, size_t nv) {
    if (nv == 0) return false;
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_header(nv);
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size();
    ok = ok && write_lines(f, nv, 40, [&](TextOut& o, size_t i) { mesh_vertex_line(o, xyz, rgb, i); });
    ok = ok && write_lines(f, nv / 3, 24, [&](TextOut& o, size_t q) { mesh_face_line(o, q); });
    return fclose(f) == 0 && ok;
}
// the welded mesh (include/psgsdf_mesh.h) as a binary little-endian PLY: vertex records x y z nx ny nz (float) red green blue (uchar), 27 B;
// face records a uchar 3 and three int vertex indices, 13 B.  Coordinates are grid-local like every other writer's: the comment line holds the
// grid origin and the voxel size (world = origin + the position).  No reference counterpart: `voxelPS --indexed-mesh`.
constexpr size_t kPlyVertexBytes = 27, kPlyFaceBytes = 13;
inline std::string mesh_indexed_header(size_t nv, size_t nf, const float origin[3], float vs, const std::string& extra = std::string(),      // extra: further header lines (each ends in \n)
                                       const std::string& vertex_props = std::string()) {                                                     // vertex_props: further vertex property lines, behind the colours
    char c[160];
    snprintf(c, sizeof c, "comment grid origin %.9g %.9g %.9g voxel size %.9g\n", (double)origin[0], (double)origin[1], (double)origin[2], (double)vs);
    return std::string("ply\nformat binary_little_endian 1.0\n") + c + extra + "element vertex " + std::to_string(nv) + "\n"
           "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\n" + vertex_props +
           "element face " + std::to_string(nf) + "\nproperty list uchar int vertex_indices\nend_header\n";
}
inline std::string mesh_indexed_vertices(const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv) {
    std::string b(nv * kPlyVertexBytes, '\0'); char* p = &b[0];      // (the host is little-endian: the records are the arrays' bytes)
    for (size_t i = 0; i < nv; ++i, p += kPlyVertexBytes) { memcpy(p, xyz + 3 * i, 12); memcpy(p + 12, nrm + 3 * i, 12); memcpy(p + 24, rgb + 3 * i, 3); }
    return b;
}
inline std::string mesh_indexed_faces(const int32_t* faces, size_t nf) {
    std::string b(nf * kPlyFaceBytes, '\0'); char* p = &b[0];
    for (size_t q = 0; q < nf; ++q, p += kPlyFaceBytes) { p[0] = 3; memcpy(p + 1, faces + 3 * q, 12); }
    return b;
}
inline bool write_mesh_indexed_ply(const std::string& file, const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const int32_t* faces, size_t nf,
                                   const float origin[3], float vs, const std::string& extra = std::string()) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_indexed_header(nv, nf, origin, vs, extra), v = mesh_indexed_vertices(xyz, nrm, rgb, nv), q = mesh_indexed_faces(faces, nf);
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() && fwrite(v.data(), 1, v.size(), f) == v.size() && fwrite(q.data(), 1, q.size(), f) == q.size();
    return fclose(f) == 0 && ok;
}
// the welded mesh with the fit of its vertices (include/psgsdf_fit.h): the format above with three more vertex properties behind the colours -- float quality
// (the rms residual), float loss (the mean robust loss), int n_obs -- 39 B per vertex, and one more header line with the overall rms residual (the
// root of the n_obs-weighted mean of quality^2, in double from the columns as written) and the sum of n_obs.  `voxelPS --mesh-fit`.
constexpr size_t kPlyFitVertexBytes = kPlyVertexBytes + 12;
inline std::string mesh_fit_comment(const float* rms, const int32_t* n_obs, size_t nv) {
    double q = 0.0; long long n = 0;
    for (size_t i = 0; i < nv; ++i) { q += (double)n_obs[i] * ((double)rms[i] * (double)rms[i]); n += n_obs[i]; }
    char c[120];
    snprintf(c, sizeof c, "comment fit rms %.17g observations %lld\n", n ? std::sqrt(q / (double)n) : 0.0, n);
    return c;
}
inline bool write_mesh_fit_ply(const std::string& file, const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const int32_t* faces, size_t nf,
                               const float origin[3], float vs, const float* rms, const float* loss, const int32_t* n_obs) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_indexed_header(nv, nf, origin, vs, mesh_fit_comment(rms, n_obs, nv), "property float quality\nproperty float loss\nproperty int n_obs\n");
    const std::string base = mesh_indexed_vertices(xyz, nrm, rgb, nv), q = mesh_indexed_faces(faces, nf);
    std::string v(nv * kPlyFitVertexBytes, '\0'); char* p = &v[0];
    for (size_t i = 0; i < nv; ++i, p += kPlyFitVertexBytes) { memcpy(p, base.data() + i * kPlyVertexBytes, kPlyVertexBytes); memcpy(p + 27, rms + i, 4); memcpy(p + 31, loss + i, 4); memcpy(p + 35, n_obs + i, 4); }
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() && fwrite(v.data(), 1, v.size(), f) == v.size() && fwrite(q.data(), 1, q.size(), f) == q.size();
    return fclose(f) == 0 && ok;
}
// the welded mesh with the curvature of its vertices (include/psgsdf_curvature.h): the format of _mesh_indexed.ply with five more vertex properties behind
// the colours -- float quality (the mean curvature), float gauss, float k1, float k2, uchar curvature_valid (valid end voxels) -- 44 B per vertex, and one
// more header line with the mean of quality over the vertices with curvature_valid > 0 (in double, from the column as written) and their number.
// `voxelPS --mesh-curvature`.
constexpr size_t kPlyCurvatureVertexBytes = kPlyVertexBytes + 17;
inline std::string mesh_curvature_comment(const float* mean, const uint8_t* valid, size_t nv) {
    double q = 0.0; long long n = 0;
    for (size_t i = 0; i < nv; ++i) if (valid[i] > 0) { q += (double)mean[i]; n += 1; }
    char c[120];
    snprintf(c, sizeof c, "comment curvature mean %.17g valid %lld\n", n ? q / (double)n : 0.0, n);
    return c;
}
inline bool write_mesh_curvature_ply(const std::string& file, const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const int32_t* faces, size_t nf,
                                     const float origin[3], float vs, const float* mean, const float* gauss, const float* k1, const float* k2, const uint8_t* valid) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_indexed_header(nv, nf, origin, vs, mesh_curvature_comment(mean, valid, nv),
                                              "property float quality\nproperty float gauss\nproperty float k1\nproperty float k2\nproperty uchar curvature_valid\n");
    const std::string base = mesh_indexed_vertices(xyz, nrm, rgb, nv), q = mesh_indexed_faces(faces, nf);
    std::string v(nv * kPlyCurvatureVertexBytes, '\0'); char* p = &v[0];
    for (size_t i = 0; i < nv; ++i, p += kPlyCurvatureVertexBytes) {
        memcpy(p, base.data() + i * kPlyVertexBytes, kPlyVertexBytes);
        memcpy(p + 27, mean + i, 4); memcpy(p + 31, gauss + i, 4); memcpy(p + 35, k1 + i, 4); memcpy(p + 39, k2 + i, 4); memcpy(p + 43, valid + i, 1);
    }
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() && fwrite(v.data(), 1, v.size(), f) == v.size() && fwrite(q.data(), 1, q.size(), f) == q.size();
    return fclose(f) == 0 && ok;
}
// the welded mesh of the filled state (include/psgsdf_fill.h): the format of _mesh_indexed.ply with one more vertex property behind the colours -- uchar
// filled (filled end voxels: 0, 1 or 2) -- 28 B per vertex, and one more header line: the rounds, the sweeps, the voxels filled and the boundary edges of
// the kept components without and with the filling.  `voxelPS --mesh-fill`.
constexpr size_t kPlyFilledVertexBytes = kPlyVertexBytes + 1;
inline std::string mesh_filled_comment(int rounds, int sweeps, long long voxels, long long boundary_before, long long boundary_after) {
    char c[200];
    snprintf(c, sizeof c, "comment fill rounds %d sweeps %d voxels %lld boundary_edges %lld %lld\n", rounds, sweeps, voxels, boundary_before, boundary_after);
    return c;
}
inline bool write_mesh_filled_ply(const std::string& file, const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const int32_t* faces, size_t nf,
                                  const float origin[3], float vs, const uint8_t* filled, const std::string& comment) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_indexed_header(nv, nf, origin, vs, comment, "property uchar filled\n");
    const std::string base = mesh_indexed_vertices(xyz, nrm, rgb, nv), q = mesh_indexed_faces(faces, nf);
    std::string v(nv * kPlyFilledVertexBytes, '\0'); char* p = &v[0];
    for (size_t i = 0; i < nv; ++i, p += kPlyFilledVertexBytes) { memcpy(p, base.data() + i * kPlyVertexBytes, kPlyVertexBytes); memcpy(p + 27, filled + i, 1); }
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() && fwrite(v.data(), 1, v.size(), f) == v.size() && fwrite(q.data(), 1, q.size(), f) == q.size();
    return fclose(f) == 0 && ok;
}
// the welded mesh with its distance to a reference (include/psgsdf_compare.h): the format of _mesh_indexed.ply with two more vertex properties behind
// the colours -- float distance (inf: no match within max_dist), char side (-1 inside, +1 outside, 0 on the reference, a cloud, or no match) -- 32 B per
// vertex, and `extra` header lines.  `voxelPS --compare-ply`.
constexpr size_t kPlyCompareVertexBytes = kPlyVertexBytes + 5;
inline bool write_mesh_compare_ply(const std::string& file, const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const int32_t* faces, size_t nf,
                                   const float origin[3], float vs, const float* dist, const int8_t* side, const std::string& extra = std::string()) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = mesh_indexed_header(nv, nf, origin, vs, extra, "property float distance\nproperty char side\n");
    const std::string base = mesh_indexed_vertices(xyz, nrm, rgb, nv), q = mesh_indexed_faces(faces, nf);
    std::string v(nv * kPlyCompareVertexBytes, '\0'); char* p = &v[0];
    for (size_t i = 0; i < nv; ++i, p += kPlyCompareVertexBytes) { memcpy(p, base.data() + i * kPlyVertexBytes, kPlyVertexBytes); memcpy(p + 27, dist + i, 4); memcpy(p + 31, side + i, 1); }
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size() && fwrite(v.data(), 1, v.size(), f) == v.size() && fwrite(q.data(), 1, q.size(), f) == q.size();
    return fclose(f) == 0 && ok;
}
// A reference mesh or cloud from a PLY: `element vertex` with float x y z (other scalar properties are skipped by their declared sizes) and an optional
// `element face` with a `vertex_indices` (or `vertex_index`) list of three per face; binary little-endian, as this project's own writers produce, or
// ASCII.  Elements behind the faces are not read; an element in front of them must have scalar properties only.  false + why: anything else.
inline bool read_reference_ply(const std::string& file, std::vector<float>& xyz, std::vector<int32_t>& faces, std::string& why) {
    std::ifstream in(file, std::ios::binary);
    if (!in) { why = "cannot open " + file; return false; }
    auto type_size = [](const std::string& t) { return t == "char" || t == "uchar" || t == "int8" || t == "uint8" ? 1 : t == "short" || t == "ushort" || t == "int16" || t == "uint16" ? 2
                                                     : t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32" ? 4 : t == "double" || t == "float64" ? 8 : 0; };
    struct Prop { std::string name, type, count_type; bool list = false; };
    struct Elem { std::string name; long long n = 0; std::vector<Prop> props; };
    std::vector<Elem> elems;
    std::string line; int format = -1;      // 0 ascii, 1 binary little-endian
    if (!std::getline(in, line) || line.compare(0, 3, "ply") != 0) { why = file + " is not a PLY file"; return false; }
    bool ended = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::istringstream s(line); std::string w; s >> w;
        if (w == "end_header") { ended = true; break; }
        if (w == "format") { std::string f; s >> f; format = f == "ascii" ? 0 : f == "binary_little_endian" ? 1 : -1; }
        else if (w == "element") { Elem e; s >> e.name >> e.n; if (!s || e.n < 0) { why = file + ": bad element line"; return false; } elems.push_back(e); }
        else if (w == "property") {
            if (elems.empty()) { why = file + ": a property before any element"; return false; }
            Prop p; s >> p.type;
            if (p.type == "list") { p.list = true; s >> p.count_type >> p.type; }
            s >> p.name;
            if (!s || !type_size(p.type) || (p.list && !type_size(p.count_type))) { why = file + ": bad property line '" + line + "'"; return false; }
            elems.back().props.push_back(p);
        }
    }
    if (!ended || format < 0) { why = file + ": no end_header, or a format other than ascii and binary_little_endian"; return false; }
    auto is_float = [](const std::string& t) { return t == "float" || t == "float32"; };
    auto is_signed_int = [](const std::string& t) { return t == "char" || t == "short" || t == "int" || t == "int8" || t == "int16" || t == "int32"; };
    auto read_int = [&](const std::string& t, long long& v) -> bool {      // one integer of type t: binary, or the next ASCII token
        if (format == 0) { double d; if (!(in >> d)) return false; v = (long long)d; return true; }
        unsigned char b[8] = {}; const int n = type_size(t);
        if (!in.read((char*)b, n)) return false;
        unsigned long long u = 0; for (int k = n - 1; k >= 0; --k) u = (u << 8) | b[k];
        v = is_signed_int(t) && n < 8 && (u >> (8 * n - 1)) ? (long long)u - (1ll << (8 * n)) : (long long)u;
        return true;
    };
    bool got_vertices = false;
    xyz.clear(); faces.clear();
    for (const Elem& e : elems) {
        if (e.name == "vertex") {
            int off[3] = {-1, -1, -1}, col[3] = {-1, -1, -1}, stride = 0, k = 0;
            for (const Prop& p : e.props) {
                if (p.list) { why = file + ": a list property in the vertex element"; return false; }
                for (int a = 0; a < 3; ++a) if (p.name == std::string(1, "xyz"[a])) { if (!is_float(p.type)) { why = file + ": " + p.name + " is not a float"; return false; } off[a] = stride; col[a] = k; }
                stride += type_size(p.type); ++k;
            }
            if (off[0] < 0 || off[1] < 0 || off[2] < 0) { why = file + ": the vertex element has no float x y z"; return false; }
            if (e.n > (long long)INT32_MAX) { why = file + ": too many vertices"; return false; }
            xyz.resize(3 * (size_t)e.n);
            if (format == 1) {
                std::vector<char> rec((size_t)stride);
                for (long long i = 0; i < e.n; ++i) {
                    if (!in.read(rec.data(), stride)) { why = file + ": the vertex records end early"; return false; }
                    for (int a = 0; a < 3; ++a) memcpy(&xyz[3 * (size_t)i + a], rec.data() + off[a], 4);
                }
            } else {
                for (long long i = 0; i < e.n; ++i)
                    for (int c = 0; c < k; ++c) {
                        std::string tok;
                        if (!(in >> tok)) { why = file + ": the vertex lines end early"; return false; }
                        for (int a = 0; a < 3; ++a) if (col[a] == c) {
                            char* end = nullptr; const float v = strtof(tok.c_str(), &end);
                            if (end == tok.c_str() || *end) { why = file + ": '" + tok + "' is not a number"; return false; }
                            xyz[3 * (size_t)i + a] = v;
                        }
                    }
            }
            got_vertices = true;
        } else if (e.name == "face") {
            if (!got_vertices) { why = file + ": the face element comes before the vertices"; return false; }
            bool has = false;
            for (const Prop& p : e.props) has = has || (p.list && (p.name == "vertex_indices" || p.name == "vertex_index"));
            if (!has) { why = file + ": the face element has no vertex_indices list"; return false; }
            faces.reserve(3 * (size_t)e.n);
            for (long long q = 0; q < e.n; ++q)
                for (const Prop& p : e.props) {
                    long long cnt = 1, v = 0;
                    if (p.list && !read_int(p.count_type, cnt)) { why = file + ": the face records end early"; return false; }
                    const bool idx = p.list && (p.name == "vertex_indices" || p.name == "vertex_index");
                    if (idx && cnt != 3) { why = file + ": a face with " + std::to_string(cnt) + " corners (triangles only)"; return false; }
                    for (long long j = 0; j < cnt; ++j) {
                        if (is_float(p.type) || p.type == "double" || p.type == "float64") {      // (never an index: skipped)
                            if (format == 0) { double d; if (!(in >> d)) { why = file + ": the face records end early"; return false; } }
                            else { char b[8]; if (!in.read(b, type_size(p.type))) { why = file + ": the face records end early"; return false; } }
                            continue;
                        }
                        if (!read_int(p.type, v)) { why = file + ": the face records end early"; return false; }
                        if (idx) { if (v < 0 || v >= (long long)(xyz.size() / 3)) { why = file + ": a face index outside the vertices"; return false; } faces.push_back((int32_t)v); }
                    }
                }
            return true;      // (what follows the faces is not read)
        } else {      // another element in front: skipped by its declared sizes
            long long bytes = 0, cols = 0;
            for (const Prop& p : e.props) { if (p.list) { why = file + ": a list property in element " + e.name; return false; } bytes += type_size(p.type); ++cols; }
            if (format == 1) in.seekg(bytes * e.n, std::ios::cur);
            else for (long long i = 0; i < e.n * cols; ++i) { std::string tok; if (!(in >> tok)) { why = file + ": element " + e.name + " ends early"; return false; } }
        }
    }
    if (!got_vertices) { why = file + ": no vertex element"; return false; }
    return true;
}
// save_pointcloud / extract_pc (OptimizerAux.cpp:456-511, VolumetricGradSdf.cpp:320-376): x y z nx ny nz r g b
inline bool write_pointcloud_ply(const std::string& file, const float* pn, const int32_t* col, size_t n) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = pointcloud_header(n);
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size();
    ok = ok && write_lines(f, n, 80, [&](TextOut& o, size_t i) { pointcloud_line(o, pn, col, i); });
    return fclose(f) == 0 && ok;
}
// saveSDF (OptimizerAux.cpp:513-577): dims, the box's first voxel in metres, the voxel size, then -dist, x fastest
inline bool write_sdf_block(const std::string& file, const int lo[3], const int dim[3], float vs, const float* v) {
    FILE* f = fopen(file.c_str(), "wb"); if (!f) return false;
    const std::string h = sdf_header(lo, dim, vs);
    bool ok = fwrite(h.data(), 1, h.size(), f) == h.size();
    ok = ok && write_lines(f, (size_t)dim[0] * dim[1] * dim[2], 12, [&](TextOut& o, size_t i) { o.f(v[i]); o.c('\n'); });
    return fclose(f) == 0 && ok;
}
// One background thread that formats and writes the dumps in the order they were issued; drain() before anything that must see the files.
class DumpQueue {
    std::thread th_; std::mutex m_; std::condition_variable cv_, idle_; std::deque<std::function<void()>> q_; bool stop_ = false, busy_ = false;
    void run() {
        for (;;) {
            std::function<void()> job;
            { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return stop_ || !q_.empty(); }); if (q_.empty()) return; job = std::move(q_.front()); q_.pop_front(); busy_ = true; }
            { PSG_STAGE("background: format + write the dump files"); job(); }
            { std::lock_guard<std::mutex> l(m_); busy_ = false; }
            idle_.notify_all();
        }
    }
    std::atomic<int> failures_{0};
public:
    static DumpQueue& get() { static DumpQueue q; return q; }
    void report_failure() { failures_.fetch_add(1); }      // a job could not open / write its file: surfaced by failures() after drain() (voxelPS exits non-zero)
    int failures() const { return failures_.load(); }
    void push(std::function<void()> job) {
        if (host_writers()) { job(); return; }
        std::lock_guard<std::mutex> l(m_);
        if (!th_.joinable()) th_ = std::thread([this] { run(); });
        q_.push_back(std::move(job)); cv_.notify_one();
    }
    void drain() { PSG_STAGE("wait for the background writer"); std::unique_lock<std::mutex> l(m_); idle_.wait(l, [&] { return q_.empty() && !busy_; }); }
    ~DumpQueue() { { std::lock_guard<std::mutex> l(m_); stop_ = true; } cv_.notify_all(); if (th_.joinable()) th_.join(); }
};

// ---- one run on N devices (`voxelPS --gpus N`: one process per GPU, the volume cut into z-slabs; no reference counterpart) ---------------------------
// main() fills this in before anything else.  Every rank runs the same program on the same inputs (decodes the frames, selects the keyframes); the
// engine calls are collective.  Rank 0 narrates and writes the small text files; the big ones are written by ALL ranks: each formats the lines of
// its share (psgsdf_extract_* on a multi-rank context) and writes them into their place in the one file -- the places come from an exclusive scan of
// the byte counts over the ranks (psgsdf_comm_allreduce_host).  The files are the single-process files line for line, up to what the slabs'
// rank-order sums do to the last digit of a value.
struct RankInfo { int rank = 0, n = 1, device = 0; bool sockets = false; std::vector<int> fds; std::vector<uint8_t> id; };
inline RankInfo& rank_info() { static RankInfo r; return r; }
inline bool multi_rank() { return rank_info().n > 1; }
inline bool lead_rank() { return rank_info().rank == 0; }
// k numbers of every rank -> the sums over the ranks in front of this one, and over all
// `local_ok` = false: this rank failed in front of the collective.  It STILL enters it (a rank that returned early left the others blocked in the
// all-reduce: ADVICE r05) and its flag travels as one more summed element, so that every rank returns false together.
inline bool scan_over_ranks(psgsdf_ctx* ctx, const std::vector<double>& mine, std::vector<double>& before, std::vector<double>& total, bool local_ok = true) {
    const RankInfo& ri = rank_info(); const size_t k = mine.size(), k1 = k + 1;
    std::vector<double> all(k1 * (size_t)ri.n, 0.0);
    for (size_t i = 0; i < k; ++i) all[k1 * (size_t)ri.rank + i] = local_ok ? mine[i] : 0.0;
    all[k1 * (size_t)ri.rank + k] = local_ok ? 0.0 : 1.0;
    if (psgsdf_comm_allreduce_host(ctx, all.data(), (int)all.size())) return false;
    before.assign(k, 0.0); total.assign(k, 0.0);
    double failed = 0.0;
    for (int r = 0; r < ri.n; ++r) { for (size_t i = 0; i < k; ++i) { if (r < ri.rank) before[i] += all[k1 * (size_t)r + i]; total[i] += all[k1 * (size_t)r + i]; } failed += all[k1 * (size_t)r + k]; }
    return failed == 0.0;
}
inline size_t bytes_of(const std::vector<TextOut>& parts) { size_t b = 0; for (auto& p : parts) b += p.s.size(); return b; }
struct FilePiece { long long offset; std::shared_ptr<std::vector<TextOut>> parts; };
// this rank's pieces of a file all ranks write: rank 0 also owns the header and the file's final length
inline void write_shared_file(const std::string& file, const std::string& header, long long total_bytes, std::vector<FilePiece> pieces) {
    DumpQueue::get().push([=] {
        const int fd = open(file.c_str(), O_CREAT | O_WRONLY, 0644);      // (no O_TRUNC: the other ranks write their pieces into the same file at the same time; the lead rank sets the final length)
        if (fd < 0) { std::cerr << "couldn't open " << file << std::endl; DumpQueue::get().report_failure(); return; }
        auto put = [&](const char* p, size_t n, long long at) { while (n) { const ssize_t k = pwrite(fd, p, n, (off_t)at); if (k <= 0) { std::cerr << "couldn't write " << file << std::endl; return false; } p += k; n -= (size_t)k; at += k; } return true; };
        bool ok = true;
        if (lead_rank()) ok = put(header.data(), header.size(), 0) && ftruncate(fd, (off_t)total_bytes) == 0;
        for (auto& pc : pieces) { long long at = pc.offset; for (auto& t : *pc.parts) { if (ok && !t.s.empty()) ok = put(t.s.data(), t.s.size(), at); at += (long long)t.s.size(); } }
        if (close(fd) != 0) ok = false;
        if (!ok) DumpQueue::get().report_failure();      // (this rank's piece is missing from a file the other ranks completed: the run reports it, voxelps_main.cpp)
    });
}

struct DepthImage;
// writers shared by VolumetricGradSdf (init_* files) and Optimizer (refined files): cropped box of |d| <= sqrt(3) vs,
// -dist, grid-local coordinates (VolumetricGradSdf.cpp:234-318,379-442, OptimizerAux.cpp:278-363,513-577)
struct CropBox { int lo[3], hi[3]; bool any; };
inline CropBox crop_box(const int dim[3], const std::vector<float>& dist, float vs) {
    CropBox b{{1 << 30, 1 << 30, 1 << 30}, {-(1 << 30), -(1 << 30), -(1 << 30)}, false};
    size_t lin = 0;
    for (int k = 0; k < dim[2]; ++k) for (int j = 0; j < dim[1]; ++j) for (int i = 0; i < dim[0]; ++i, ++lin) {
        if (std::fabs(dist[lin]) > std::sqrt(3) * vs) continue;
        int idx[3] = {i, j, k};
        for (int a = 0; a < 3; ++a) { b.lo[a] = std::min(b.lo[a], idx[a]); b.hi[a] = std::max(b.hi[a], idx[a]); }
        b.any = true;
    }
    return b;
}
inline bool write_mesh(const std::string& file, const int dim[3], float vs, const std::vector<float>& dist, const std::vector<float>& weight, const std::vector<float>& rgb) {
    CropBox b = crop_box(dim, dist, vs); if (!b.any) return false;
    const size_t n = (size_t)dim[0] * dim[1] * dim[2];
    int d[3] = {b.hi[0] - b.lo[0] + 1, b.hi[1] - b.lo[1] + 1, b.hi[2] - b.lo[2] + 1};
    const size_t nv = (size_t)d[0] * d[1] * d[2];
    std::vector<float> t(nv), w(nv); std::vector<unsigned char> r(nv), g(nv), bl(nv);
    size_t pos = 0;
    for (int k = b.lo[2]; k <= b.hi[2]; ++k) for (int j = b.lo[1]; j <= b.hi[1]; ++j) for (int i = b.lo[0]; i <= b.hi[0]; ++i, ++pos) {
        size_t lin = (size_t)i + (size_t)j * dim[0] + (size_t)k * dim[0] * dim[1];
        t[pos] = -dist[lin]; w[pos] = weight[lin];
        r[pos] = (unsigned char)int(255 * rgb[lin]); g[pos] = (unsigned char)int(255 * rgb[n + lin]); bl[pos] = (unsigned char)int(255 * rgb[2 * n + lin]);
    }
    float size[3] = {vs * d[0], vs * d[1], vs * d[2]}, org[3] = {-vs * b.lo[0], -vs * b.lo[1], -vs * b.lo[2]};
    MarchingCubes mc(d, size, org);
    mc.computeIsoSurface(t.data(), w.data(), r.data(), g.data(), bl.data());
    return mc.savePly(file);
}
inline bool write_sdf(const std::string& file, const int dim[3], float vs, const std::vector<float>& dist) {
    CropBox b = crop_box(dim, dist, vs); if (!b.any) return false;
    std::ofstream f(file.c_str()); if (!f.is_open()) return false;
    f << b.hi[0] - b.lo[0] + 1 << " " << b.hi[1] - b.lo[1] + 1 << " " << b.hi[2] - b.lo[2] + 1 << "\n";
    f << b.lo[0] * vs << " " << b.lo[1] * vs << " " << b.lo[2] * vs << "\n" << vs << "\n";
    for (int k = b.lo[2]; k <= b.hi[2]; ++k) for (int j = b.lo[1]; j <= b.hi[1]; ++j) for (int i = b.lo[0]; i <= b.hi[0]; ++i)
        f << -dist[(size_t)i + (size_t)j * dim[0] + (size_t)k * dim[0] * dim[1]] << "\n";
    return true;
}

// SoA image of VolumetricGradSdf's state (x-fastest, VoxelGrid.h:79-82).  Two modes: host arrays handed to the optimiser
// (voxelps_scene), or -- when created with `attach` -- a volume that lives on the device from the first frame on
// (voxelPS: VolumetricGradSdf::update and the tracker run there too).
struct VolumetricGradSdf {
    int grid_dim_[3] = {0, 0, 0};
    float voxel_size_ = 0, T_ = 0;
    float shift_[3] = {0, 0, 0};
    float z_min_ = 0.5f, z_max_ = 10.0f;             // Sdf.h:40-41
    size_t counter_ = 0;
    std::vector<float> dist, grad, weight, rgb;      // N, 3N (x|y|z), N, 3N (r|g|b)
    std::vector<uint64_t> vis; int vis_words = 1;    // N*vis_words, bit c = seen by integrated frame c
    psgsdf_ctx* ctx = nullptr;                       // device-resident mode (owned)
    size_t num_voxels() const { return (size_t)grid_dim_[0] * grid_dim_[1] * grid_dim_[2]; }
    ~VolumetricGradSdf() { if (ctx) psgsdf_destroy(ctx); }

    // VolumetricGradSdf(grid_dim, voxel_size, shift, T) + init() on the device (main_ps.cpp:183)
    bool attach(const int dim[3], float voxel_size, const float shift[3], float T, const Mat3f& K, const psgsdf_settings& s, int max_frames) {
        for (int a = 0; a < 3; ++a) { grid_dim_[a] = dim[a]; shift_[a] = shift[a]; }
        voxel_size_ = voxel_size; T_ = T;
        psgsdf_grid_desc g{}; for (int a = 0; a < 3; ++a) { g.dim[a] = dim[a]; g.shift[a] = shift[a]; } g.voxel_size = voxel_size; g.truncation = T;
        const RankInfo& ri = rank_info();
        if (psgsdf_create(&g, K.v, &s, ri.device, &ctx)) { ctx = nullptr; return false; }
        if (ri.n > 1) {      // one process per GPU: RCCL over xGMI, or the node-local socket transport (ranks that share a device; no RCCL)
            const int rc = ri.sockets ? psgsdf_comm_init_sockets(ctx, ri.fds.data(), ri.rank, ri.n) : psgsdf_comm_init(ctx, ri.id.data(), ri.rank, ri.n);
            if (rc) { std::cerr << "rank " << ri.rank << ": no communicator: " << last_error() << std::endl; return false; }
        }
        std::cout << "Number of voxels: " << num_voxels() << std::endl;
        return psgsdf_volume_init(ctx, max_frames) == 0;
    }
    const char* last_error() const { const char* e = ctx ? psgsdf_last_error(ctx) : "no device volume"; return e ? e : ""; }
    void set_zmin(float z) { z_min_ = z; }
    void set_zmax(float z) { z_max_ = z; }
    void increase_counter() { ++counter_; }
    // VolumetricGradSdf::update (VolumetricGradSdf.cpp:51-138): FALS normals + fusion, both on the device
    bool update(const ImageRGB& color, const std::vector<float>& depth, const Mat4f& pose) {
        PSG_STAGE("fuse: FALS normals + integration (device, incl. transfers)");
        if (host_writers()) {      // (round 4's path: the normals come back to the host and go up again)
            std::vector<float> nrm((size_t)3 * color.rows * color.cols);
            if (psgsdf_estimate_normals(ctx, depth.data(), color.cols, color.rows, nrm.data())) return false;
            return psgsdf_integrate_frame(ctx, color.data.data(), depth.data(), nrm.data(), color.cols, color.rows, pose.data(), (int)counter_, z_min_, z_max_) == 0;
        }
        return psgsdf_integrate_frame(ctx, color.data.data(), depth.data(), nullptr, color.cols, color.rows, pose.data(), (int)counter_, z_min_, z_max_) == 0;      // NULL: FALS normals on the device
    }
    bool sync_host() {
        const size_t n = num_voxels();
        dist.resize(n); grad.resize(3 * n); weight.resize(n); rgb.resize(3 * n);
        return psgsdf_download_volume(ctx, dist.data(), grad.data(), weight.data(), rgb.data(), nullptr) == 0;
    }
    bool extract_mesh(const std::string& filename) {
        PSG_STAGE("dump: mesh (marching cubes + PLY)");
        if (ctx && indexed_mesh() && !device_mesh_indexed(ctx, filename)) std::cout << "couldn't save the indexed mesh of " << filename << std::endl;
        if (ctx && clean_mesh() && !device_mesh_clean(ctx, filename)) std::cout << "couldn't save the cleaned mesh of " << filename << std::endl;
        if (ctx && mesh_lod_voxels() > 0 && !device_mesh_lod(ctx, filename)) std::cout << "couldn't save the level-of-detail mesh of " << filename << std::endl;
        if (ctx && mesh_fit() && !device_mesh_fit(ctx, filename)) std::cout << "couldn't save the mesh with its fit of " << filename << std::endl;
        if (ctx && mesh_curvature() && !device_mesh_curvature(ctx, filename)) std::cout << "couldn't save the mesh with its curvature of " << filename << std::endl;
        if (ctx && mesh_fill_rounds() >= 0 && !device_mesh_filled(ctx, filename)) std::cout << "couldn't save the filled mesh of " << filename << std::endl;
        if (ctx && compare_ref().on && !device_mesh_compare(ctx, filename)) std::cout << "couldn't save the comparison of " << filename << std::endl;
        if (ctx && !host_writers()) return device_mesh(ctx, filename);
        return sync_host() && write_mesh(filename, grid_dim_, voxel_size_, dist, weight, rgb);
    }
    bool saveSDF(const std::string& filename) {
        PSG_STAGE("dump: sdf");
        if (ctx && !host_writers()) return device_sdf(ctx, filename, voxel_size_);
        return sync_host() && write_sdf(filename, grid_dim_, voxel_size_, dist);
    }
    // the device-side extraction (include/psgsdf.h psgsdf_extract_*): compact arrays come back, a copy of them goes to the background writer
    // <name>_mesh.ply -> <name>_mesh_indexed.ply: the welded mesh of the same state (include/psgsdf_mesh.h), binary.  A multi-rank run: every rank
    // writes its records at their place in the one file, which is byte for byte the single-process file.
    static bool device_mesh_indexed(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: welded mesh (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string file = (mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                  ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file) + "_mesh_indexed.ply";
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; int64_t nv = 0, nf = 0, first = 0;
        const bool ok = psgsdf_extract_mesh_indexed(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &first) == 0;
        if (!ok) { nv = 0; nf = 0; }
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        if (multi_rank()) {
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
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vn = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            if (!write_mesh_indexed_ply(file, vx->data(), vn->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs)) { std::cout << "couldn't save mesh " << file << std::endl; DumpQueue::get().report_failure(); }
        });
        return true;
    }
    // <name>_mesh.ply -> <name>_mesh_clean.ply (the binary format of _mesh_indexed.ply and one more comment line) + <name>_mesh_components.txt:
    // first_vertex n_vertices n_faces n_edges n_boundary_edges n_nonmanifold_edges area lo[3] hi[3] kept, one component per line
    static bool device_mesh_clean(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: mesh components (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vcomp = nullptr;
        const psgsdf_mesh_component* comps = nullptr; int64_t nv = 0, nf = 0, nc = 0;
        if (psgsdf_extract_mesh_components(ctx, &mesh_filter(), &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc) != 0 || nc == 0) return false;
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
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vn = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            bool ok = write_mesh_indexed_ply(base + "_mesh_clean.ply", vx->data(), vn->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs, extra);
            FILE* f = fopen((base + "_mesh_components.txt").c_str(), "wb");
            ok = f && fwrite(table.data(), 1, table.size(), f) == table.size() && ok;
            if (f && fclose(f) != 0) ok = false;
            if (!ok) { std::cout << "couldn't save the cleaned mesh " << base << std::endl; DumpQueue::get().report_failure(); }
        });
        return true;
    }
    // <name>_mesh.ply -> <name>_mesh_lod.ply (the binary format of _mesh_indexed.ply and one more comment line): cell = S voxels of the state's voxel size
    static bool device_mesh_lod(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: level-of-detail mesh (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vmap = nullptr;
        int64_t nv = 0, nf = 0, nv_in = 0, nf_in = 0;
        const double cell = mesh_lod_voxels() * (double)info.voxel_size;
        psgsdf_bake bk{};      // --mesh-bake: the same level-of-detail arrays (bit for bit) and the atlas, in one call
        psgsdf_bake_ao ao{};   // --mesh-bake-ao: the same bake (bit for bit) and the occlusion map
        psgsdf_bake_photo ph{};   // --mesh-bake-photo: the same bake (bit for bit) and the albedo solved from the keyframes
        psgsdf_bake_curvature cv{};   // --mesh-bake-curvature: the same bake (bit for bit) and the mean curvature of the hit voxels
        if (mesh_bake_res() > 0) {
            bool baked = false;
            if (mesh_bake_ao_dirs() > 0) {
                const psgsdf_ao_params ap{mesh_bake_ao_dirs(), 0, 8.0 * (double)info.voxel_size, (double)info.voxel_size};
                if (psgsdf_bake_lod_ao(ctx, clean_mesh() ? &mesh_filter() : nullptr, cell, mesh_bake_res(), cell, &ap, &ao) != 0) return false;
                bk = ao.bake; baked = true;
            }
            if (mesh_bake_photo()) {      // (behind the occlusion: its map has slots of its own, the bake's are filled again with the same bits)
                const psgsdf_photo_params pp{(double)info.voxel_size, 0.2, 0.05, 0, 0};
                const int rc = psgsdf_bake_lod_photo(ctx, clean_mesh() ? &mesh_filter() : nullptr, cell, mesh_bake_res(), cell, &pp, &ph);
                if (rc == 0) { bk = ph.bake; baked = true; }
                else if (rc != PSGSDF_ERR_STATE) return false;      // (before psgsdf_init: no keyframes yet)
            }
            if (mesh_bake_curvature_scale() > 0) {      // (likewise: the map in slots of its own, the bake's filled again with the same bits)
                if (psgsdf_bake_lod_curvature(ctx, clean_mesh() ? &mesh_filter() : nullptr, cell, mesh_bake_res(), cell, &cv) != 0) return false;
                bk = cv.bake; baked = true;
            }
            if (!baked && psgsdf_bake_lod(ctx, clean_mesh() ? &mesh_filter() : nullptr, cell, mesh_bake_res(), cell, &bk) != 0) return false;
            if (bk.n_faces_in == 0) return false;
            xyz = bk.xyz; nrm = bk.normals; rgb = bk.rgb; faces = bk.faces; nv = bk.n_vertices; nf = bk.n_faces; nv_in = bk.n_vertices_in; nf_in = bk.n_faces_in;
        } else if (psgsdf_extract_mesh_lod(ctx, clean_mesh() ? &mesh_filter() : nullptr, cell, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vmap, &nv_in, &nf_in) != 0
            || nf_in == 0) return false;
        char line[200];
        snprintf(line, sizeof line, "comment lod cell %.9g voxels from %lld vertices %lld faces\n", mesh_lod_voxels(), (long long)nv_in, (long long)nf_in);
        const std::string extra = line;
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vn = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            if (!write_mesh_indexed_ply(base + "_mesh_lod.ply", vx->data(), vn->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs, extra)) {
                std::cout << "couldn't save the level-of-detail mesh " << base << std::endl; DumpQueue::get().report_failure();
            }
        });
        if (mesh_bake_res() > 0 && bk.width > 0) {
            const int W = bk.width, H = bk.height; const size_t px = (size_t)W * H;
            auto uv = std::make_shared<std::vector<float>>(bk.uv, bk.uv + 6 * nf);
            auto alb = std::make_shared<std::vector<uint8_t>>(bk.albedo, bk.albedo + 3 * px);
            auto nmap = std::make_shared<std::vector<uint8_t>>(3 * px);
            for (size_t q = 0; q < 3 * px; ++q) (*nmap)[q] = normal_to_u8(bk.normal[q]);
            std::cout << "baked " << bk.n_texels << " texels onto " << nf << " faces (" << W << " x " << H << "): " << bk.n_hits << " hits (" << bk.n_hits_off_band << " off the band), "
                      << bk.n_buried << " buried, " << bk.n_misses << " misses" << std::endl;
            const bool with_ao = mesh_bake_ao_dirs() > 0 && ao.occlusion;
            auto occ = std::make_shared<std::vector<uint8_t>>();
            if (with_ao) {
                occ->assign(ao.occlusion, ao.occlusion + px);
                std::cout << "ambient occlusion: " << ao.counts.n_rays << " rays (" << ao.n_dirs << " per texel), " << ao.counts.n_occluded << " occluded, " << ao.counts.n_buried << " of them buried" << std::endl;
            }
            const bool with_photo = ph.photo_rgb != nullptr;
            auto pho = std::make_shared<std::vector<uint8_t>>();
            if (with_photo) {
                pho->assign(ph.photo_rgb, ph.photo_rgb + 3 * px);
                std::cout << "photo albedo: " << ph.counts.n_texels_solved << " of " << ph.counts.n_samples << " texels solved from " << ph.counts.n_used << " of " << ph.counts.n_pairs
                          << " views (" << ph.counts.n_outside << " outside, " << ph.counts.n_grazing << " grazing, " << ph.counts.n_occluded << " occluded, " << ph.counts.n_dark << " dark)" << std::endl;
            }
            const bool with_curv = cv.mean != nullptr;
            auto cur = std::make_shared<std::vector<uint8_t>>();
            if (with_curv) {
                cur->resize(px);
                for (size_t q = 0; q < px; ++q) (*cur)[q] = curvature_to_u8(cv.mean[q], cv.valid[q], (double)info.voxel_size, mesh_bake_curvature_scale());
                std::cout << "curvature: " << cv.n_valid << " of " << bk.n_hits << " hit texels evaluated" << std::endl;
            }
            DumpQueue::get().push([=] {
                const std::string lod = base + "_mesh_lod";
                bool ok = write_obj_bake(lod + ".obj", lod + ".mtl", lod + (with_photo ? "_photo.png" : "_albedo.png"), lod + "_normal.png", vx->data(), vn->data(), (size_t)nv, vf->data(), uv->data(), (size_t)nf,
                                         with_ao ? lod + "_ao.png" : std::string());
                ok = write_png(lod + "_albedo.png", W, H, 3, alb->data()) && ok;
                ok = write_png(lod + "_normal.png", W, H, 3, nmap->data()) && ok;
                if (with_ao) ok = write_png(lod + "_ao.png", W, H, 1, occ->data()) && ok;
                if (with_photo) ok = write_png(lod + "_photo.png", W, H, 3, pho->data()) && ok;
                if (with_curv) ok = write_png(lod + "_curvature.png", W, H, 1, cur->data()) && ok;
                if (!ok) { std::cout << "couldn't save the baked level-of-detail mesh " << base << std::endl; DumpQueue::get().report_failure(); }
            });
        }
        return true;
    }
    // <name>_mesh.ply -> <name>_mesh_fit.ply (write_mesh_fit_ply).  Before psgsdf_init there is no band: the mesh of psgsdf_extract_mesh_indexed with zeros
    static bool device_mesh_fit(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: welded mesh with vertex fit (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr;
        const int32_t* vn_obs = nullptr; const float* vrms = nullptr; const float* vloss = nullptr; int64_t nv = 0, nf = 0, first = 0;
        const int rc = psgsdf_extract_mesh_fit(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vn_obs, &vrms, &vloss);
        if (rc == PSGSDF_ERR_STATE) { if (psgsdf_extract_mesh_indexed(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &first) != 0) return false; }
        else if (rc != 0) return false;
        if (nf == 0) return false;
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vnr = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        auto fr = std::make_shared<std::vector<float>>((size_t)nv, 0.0f), fl = std::make_shared<std::vector<float>>((size_t)nv, 0.0f); auto fn = std::make_shared<std::vector<int32_t>>((size_t)nv, 0);
        if (rc == 0) { fr->assign(vrms, vrms + nv); fl->assign(vloss, vloss + nv); fn->assign(vn_obs, vn_obs + nv); }
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            if (!write_mesh_fit_ply(base + "_mesh_fit.ply", vx->data(), vnr->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs, fr->data(), fl->data(), fn->data())) {
                std::cout << "couldn't save the mesh with its fit " << base << std::endl; DumpQueue::get().report_failure();
            }
        });
        return true;
    }
    // <name>_mesh.ply -> <name>_mesh_curvature.ply (write_mesh_curvature_ply)
    static bool device_mesh_curvature(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: welded mesh with vertex curvature (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr;
        const uint8_t* valid = nullptr; const float *mean = nullptr, *gauss = nullptr, *k1 = nullptr, *k2 = nullptr; int64_t nv = 0, nf = 0;
        if (psgsdf_extract_mesh_curvature(ctx, &xyz, &nrm, &rgb, &nv, &faces, &nf, &valid, &mean, &gauss, &k1, &k2) != 0 || nf == 0) return false;
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vnr = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        auto cm = std::make_shared<std::vector<float>>(mean, mean + nv), cg = std::make_shared<std::vector<float>>(gauss, gauss + nv);
        auto c1 = std::make_shared<std::vector<float>>(k1, k1 + nv), c2 = std::make_shared<std::vector<float>>(k2, k2 + nv); auto cl = std::make_shared<std::vector<uint8_t>>(valid, valid + nv);
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            if (!write_mesh_curvature_ply(base + "_mesh_curvature.ply", vx->data(), vnr->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs,
                                          cm->data(), cg->data(), c1->data(), c2->data(), cl->data())) {
                std::cout << "couldn't save the mesh with its curvature " << base << std::endl; DumpQueue::get().report_failure();
            }
        });
        return true;
    }
    // <name>_mesh.ply -> <name>_mesh_filled.ply (write_mesh_filled_ply): three calls -- the components of the state as it is (for the boundary edges the
    // filling starts from), the filled voxels (for their number), the mesh of the filled state
    static bool device_mesh_filled(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: welded mesh of the filled state (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        const int R = mesh_fill_rounds(), K = mesh_fill_sweeps();
        const psgsdf_mesh_filter* flt = clean_mesh() ? &mesh_filter() : nullptr;
        const float* xyz = nullptr; const float* nrm = nullptr; const uint8_t* rgb = nullptr; const int32_t* faces = nullptr; const int32_t* vcomp = nullptr;
        const psgsdf_mesh_component* comps = nullptr; const uint8_t* filled = nullptr; int64_t nv = 0, nf = 0, nc = 0;
        auto boundary = [&] { long long b = 0; for (int64_t i = 0; i < nc; ++i) if (comps[i].kept) b += comps[i].n_boundary_edges; return b; };
        if (psgsdf_extract_mesh_components(ctx, flt, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc) != 0) return false;
        const long long before = boundary();
        const int64_t* lin = nullptr; const float *fd = nullptr, *fg = nullptr, *fc = nullptr; const uint8_t* fr = nullptr; int64_t n_filled = 0;
        if (psgsdf_fill_voxels(ctx, R, K, &lin, &fd, &fg, &fc, &fr, &n_filled) != 0) return false;
        if (psgsdf_extract_mesh_filled(ctx, R, K, flt, &xyz, &nrm, &rgb, &nv, &faces, &nf, &vcomp, &comps, &nc, &filled) != 0 || nf == 0) return false;
        const std::string comment = mesh_filled_comment(R, K, (long long)n_filled, before, boundary());
        auto vx = std::make_shared<std::vector<float>>(xyz, xyz + 3 * nv), vnr = std::make_shared<std::vector<float>>(nrm, nrm + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(rgb, rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(faces, faces + 3 * nf);
        auto fl = std::make_shared<std::vector<uint8_t>>(filled, filled + nv);
        psgsdf_info info{}; psgsdf_get_info(ctx, &info);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            if (!write_mesh_filled_ply(base + "_mesh_filled.ply", vx->data(), vnr->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs, fl->data(), comment)) {
                std::cout << "couldn't save the filled mesh " << base << std::endl; DumpQueue::get().report_failure();
            }
        });
        return true;
    }
    // <name>_mesh.ply -> <name>_compare.txt + <name>_mesh_compare.ply (write_mesh_compare_ply): the welded mesh (with a filter flag: its kept components)
    // against the reference of --compare-ply.  The text file, one record per line, every length in voxels and in metres:
    //   reference FILE points N faces F / voxel_size VS max_dist_voxels D tau_voxels T
    //   per direction (to_reference, to_reconstruction) three lines: the counts; mean, rms, max and signed mean; the histogram's 16 bins
    //   precision P recall R fscore F
    static bool device_mesh_compare(psgsdf_ctx* ctx, const std::string& mesh_file) {
        PSG_STAGE("dump: comparison with the reference (device) + binary PLY");
        const std::string tail = "_mesh.ply";
        const std::string base = mesh_file.size() >= tail.size() && mesh_file.compare(mesh_file.size() - tail.size(), tail.size(), tail) == 0
                                 ? mesh_file.substr(0, mesh_file.size() - tail.size()) : mesh_file;
        const CompareRef& ref = compare_ref();
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
            if (psgsdf_align_reference(ctx, clean_mesh() ? &mesh_filter() : nullptr, ref.xyz.data(), n_ref, ref.faces.data(), n_ref_faces, &ap, al.get()) != 0) return false;
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
            DumpQueue::get().push([=] {
                FILE* f = fopen((base + "_align.txt").c_str(), "wb");
                bool ok = f && fwrite(at.data(), 1, at.size(), f) == at.size();
                if (f && fclose(f) != 0) ok = false;
                if (!ok) { std::cout << "couldn't save the alignment " << base << std::endl; DumpQueue::get().report_failure(); }
            });
        }
        if (psgsdf_compare_reference(ctx, clean_mesh() ? &mesh_filter() : nullptr, ref_xyz, n_ref, ref.faces.data(), n_ref_faces, &p, &r) != 0) return false;
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
        const int64_t nv = r.n_vertices, nf = r.n_faces;
        auto vx = std::make_shared<std::vector<float>>(r.xyz, r.xyz + 3 * nv), vnr = std::make_shared<std::vector<float>>(r.normals, r.normals + 3 * nv);
        auto vc = std::make_shared<std::vector<uint8_t>>(r.rgb, r.rgb + 3 * nv); auto vf = std::make_shared<std::vector<int32_t>>(r.faces, r.faces + 3 * nf);
        auto vd = std::make_shared<std::vector<float>>(r.vertex_dist, r.vertex_dist + nv); auto vsd8 = std::make_shared<std::vector<int8_t>>(r.vertex_side, r.vertex_side + nv);
        const std::array<float, 3> org = {info.origin[0], info.origin[1], info.origin[2]}; const float vs = info.voxel_size;
        DumpQueue::get().push([=] {
            FILE* f = fopen((base + "_compare.txt").c_str(), "wb");
            bool ok = f && fwrite(txt.data(), 1, txt.size(), f) == txt.size();
            if (f && fclose(f) != 0) ok = false;
            if (nf > 0) ok = write_mesh_compare_ply(base + "_mesh_compare.ply", vx->data(), vnr->data(), vc->data(), (size_t)nv, vf->data(), (size_t)nf, org.data(), vs, vd->data(), vsd8->data(), extra) && ok;
            if (!ok) { std::cout << "couldn't save the comparison " << base << std::endl; DumpQueue::get().report_failure(); }
        });
        return true;
    }
    static bool device_mesh(psgsdf_ctx* ctx, const std::string& file) {
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
        DumpQueue::get().push([=] { if (!write_mesh_ply(file, vx->data(), vc->data(), (size_t)nv)) std::cout << "couldn't save mesh " << file << std::endl; });
        return true;
    }
    static bool device_pointcloud(psgsdf_ctx* ctx, int which, const std::string& file) {
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
        DumpQueue::get().push([=] { if (!write_pointcloud_ply(file, vp->data(), vc->data(), (size_t)n)) std::cout << " can't save point cloud!" << std::endl; });
        return true;
    }
    static bool device_sdf(psgsdf_ctx* ctx, const std::string& file, float vs) {
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
        DumpQueue::get().push([=] { write_sdf_block(file, l.data(), d.data(), vs, vv->data()); });
        return true;
    }
    // extract_pc, VolumetricGradSdf.cpp:320-376: x y z nx ny nz r g b of every voxel with |d| < sqrt(3) vs and weight > 0
    bool extract_pc(const std::string& filename) {
        PSG_STAGE("dump: point cloud");
        if (ctx && !host_writers()) return device_pointcloud(ctx, 1, filename);
        if (!sync_host()) return false;
        const size_t n = num_voxels(); std::vector<size_t> sel;
        for (size_t lin = 0; lin < n; ++lin) if (weight[lin] > 0 && std::fabs(dist[lin]) < std::sqrt(3) * voxel_size_) sel.push_back(lin);
        std::ofstream ply(filename.c_str()); if (!ply.is_open()) return false;
        ply << "ply\nformat ascii 1.0\nelement vertex " << sel.size() << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            << "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header" << std::endl;
        const int nx = grid_dim_[0], nxy = grid_dim_[0] * grid_dim_[1];
        for (size_t lin : sel) {
            int k = (int)(lin / nxy), rest = (int)(lin - (size_t)k * nxy), j = rest / nx, i = rest - j * nx;
            float g[3] = {grad[lin], grad[n + lin], grad[2 * n + lin]}; float z = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
            if (z > 0) { float s = std::sqrt(z); g[0] /= s; g[1] /= s; g[2] /= s; }
            ply << voxel_size_ * i - dist[lin] * g[0] << " " << voxel_size_ * j - dist[lin] * g[1] << " " << voxel_size_ * k - dist[lin] * g[2] << " " << g[0] << " " << g[1] << " " << g[2] << " "
                << int(255 * rgb[lin]) << " " << int(255 * rgb[n + lin]) << " " << int(255 * rgb[2 * n + lin]) << std::endl;
        }
        return true;
    }
};

// RigidPointOptimizer (sdf_tracker/RigidPointOptimizer.{h,cpp}, RigidOptimizer.h:41-47): frame-to-model tracking on the device volume
class RigidPointOptimizer {
    VolumetricGradSdf* tSDF_;
    int num_iterations_ = 50; float conv_threshold_ = 1e-3f, damping_ = 1.0f;
    Mat4f pose_ = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
public:
    explicit RigidPointOptimizer(VolumetricGradSdf* tSDF) : tSDF_(tSDF) {}
    void set_pose(const Mat4f& p) { pose_ = p; }
    Mat4f pose() const { return pose_; }
    bool optimize(const std::vector<float>& depth, int cols, int rows) {
        PSG_STAGE("track: frame-to-model (device)");
        int iters = 0, conv = 0;
        if (psgsdf_track(tSDF_->ctx, depth.data(), cols, rows, pose_.data(), tSDF_->z_min_, tSDF_->z_max_, num_iterations_, conv_threshold_, damping_, &iters, &conv)) return false;
        if (conv) std::cout << "... Convergence after " << iters << " iterations!" << std::endl;
        return conv != 0;
    }
};

class Optimizer {
protected:
    VolumetricGradSdf* tSDF_;
    float voxel_size_;
    Mat3f K_;
    std::string save_path_;
    OptimizerSettings* settings_;
    std::vector<int> frame_idx_;
    std::vector<std::shared_ptr<ImageRGB>> images_;
    std::vector<Mat4f> poses_;
    std::vector<std::string> key_stamps_;
    psgsdf_ctx* ctx_ = nullptr; bool borrowed_ = false;
    size_t num_frames_ = 0, num_voxels_ = 0;
    std::ofstream doc_;

    bool fail(const char* what, int rc) {
        std::cerr << what << " failed (" << rc << "): " << (ctx_ ? psgsdf_last_error(ctx_) : "") << std::endl;
        return false;
    }
    static int on_iter_trampoline(void* user, int iter_done, const psgsdf_iter_stats* rec) { return static_cast<Optimizer*>(user)->on_iter(iter_done, rec); }

    // getTotalEnergy's log line, OptimizerAux.cpp:259-269
    void log_energy(double E, const psgsdf_iter_stats* r, bool before_dist = false) {
        // (the blocks in front of the distance block are logged with the regulariser energies of the previous iteration: E_n / E_l only change at PsOptimizer.cpp:342-343)
        double en = r->reg_weight_n * (before_dist ? r->e_n_in : r->e_n), el = r->reg_weight_l * (before_dist ? r->e_l_in : r->e_l), er = settings_->reg_weight_rho * r->e_r;
        for (std::ostream* o : {static_cast<std::ostream*>(&std::cout), static_cast<std::ostream*>(&doc_)})
            if (o == &std::cout || doc_.is_open())
                *o << "PS energy: " << E << "\t normal reg energy: " << en << "\t laplacian reg energy: " << el << "\t rho reg energy: " << er
                   << "\t total energy: " << (float)(E + en + el + er) << std::endl;
    }
    // the per-iteration narration of PsOptimizer.cpp:304-366: needs the record only, so it runs as the engine's PASSIVE record observer
    // (psgsdf_set_record_observer) and the loop may already be working on the next iteration while it prints
    int narrate(int iter_done, const psgsdf_iter_stats* r) {
        const int iter = iter_done - 1;
        const bool led = settings_->model == LED;
        const char* names[4] = {"albedo", "light", "distance", "pose"};
        const int order_sh[4] = {0, 1, 2, 3}, order_led[4] = {1, 0, 2, 3};
        for (int q = 0; q < 4; ++q) {
            int s = led ? order_led[q] : order_sh[q];
            if (std::isnan(r->e_after[s])) continue;
            std::cout << "===> [" << iter << "]: after " << names[s] << " optimization: ";
            if (doc_.is_open()) doc_ << "===> [" << iter << "]: after " << names[s] << " optimization: \n";
            log_energy(r->e_after[s], r, s < 2);
        }
        std::cout << "===> [" << iter << "]: relative diff " << r->rel_diff << std::endl;
        if (doc_.is_open()) doc_ << "===> [" << iter << "]: relative diff " << r->rel_diff << "\n";
        return 0;
    }
    static int narrate_trampoline(void* user, int iter_done, const psgsdf_iter_stats* rec) { return static_cast<Optimizer*>(user)->narrate(iter_done, rec); }
    // the periodic dumps of PsOptimizer.cpp:397-398,419-423 read the STATE of the iteration: the exact-state callback, due every 3rd iteration
    // (psgsdf_set_on_iter_period(3)) and after the 2x refinement; in between the loop closes its iterations speculatively
    int on_iter(int iter_done, const psgsdf_iter_stats* r) {
        const int iter = iter_done - 1;
        if (r->upsampled) {   // PsOptimizer.cpp:397-405
            save_pointcloud("upsample_after_" + std::to_string(iter));
            extract_mesh("upsample_after_" + std::to_string(iter));
            // the log line behind the refinement: the iteration's last PS energy and Eikonal term with the Laplacian energy of the REFINED grid under
            // its re-normalised weight (PsOptimizer.cpp:400-405: E_l = getLaplacianEnergy(); reg_weight_l *= E / E_l; getTotalEnergy(...))
            double e4[4] = {0, 0, 0, 0}; psgsdf_info info{};
            if (!psgsdf_energy(ctx_, e4) && !psgsdf_get_info(ctx_, &info)) {
                double E = 0; for (int q = 0; q < 4; ++q) if (!std::isnan(r->e_after[q])) E = r->e_after[q];      // (slot order albedo, light, dist, pose: the last enabled block is the last one run)
                psgsdf_iter_stats t = *r; t.e_l = e4[2]; t.reg_weight_l = info.reg_weight_l;
                std::cout << "===> [" << iter << "]: after pose optimization: ";
                if (doc_.is_open()) doc_ << "===> [" << iter << "]: after pose optimization: \n";
                log_energy(E, &t);
            }
        }
        if (iter_done % 3 == 0) {
            savePoses("after_poses_opt_" + std::to_string(iter_done));
            save_pointcloud("after_iter_" + std::to_string(iter_done));
            extract_mesh("after_iter_" + std::to_string(iter_done));
        }
        return 0;
    }

public:
    Optimizer(VolumetricGradSdf* tSDF, const float voxel_size, const Mat3f& K, std::string save_path, OptimizerSettings* settings)
        : tSDF_(tSDF), voxel_size_(voxel_size), K_(K), save_path_(save_path), settings_(settings) {}
    virtual ~Optimizer() { if (ctx_ && !borrowed_) psgsdf_destroy(ctx_); }

    void setImages(std::vector<std::shared_ptr<ImageRGB>> images) { images_ = images; }          // Optimizer.h:137-140
    void setPoses(std::vector<Mat4f>& pose) { poses_ = pose; }                                    // Optimizer.h:142-145
    void setKeyframes(std::vector<int>& keyframes) { frame_idx_ = keyframes; }                    // Optimizer.h:147-150
    void setKeytimestamps(std::vector<std::string>& keystamps) { key_stamps_ = keystamps; }      // Optimizer.h:151-154

    // `voxelPS --render-keyframes` (no reference counterpart): every keyframe re-rendered from the final state (include/psgsdf_render.h) as
    // <prefix>render/<keyframe>_{rendered,albedo,shading,residual}.png and one row per keyframe in <prefix>render_report.txt.  Bytes: values clamped to
    // [0, 1], then round(255 v); the residual as 0.5 + r.  Multi-rank: the render calls are collective (every rank makes them and gets the whole
    // views), the lead rank writes the files.
    bool renderKeyframes(const std::string& prefix) {
        if (!ctx_) return false;
        const int F = (int)num_frames_;
        const bool lead = lead_rank();
        std::vector<psgsdf_render_stats> rows(F);
        if (int rc = psgsdf_render_report(ctx_, rows.data())) return fail("psgsdf_render_report", rc);
        const std::string dir = prefix + "render/";
        std::ofstream rep;
        if (lead) {
            ::mkdir(dir.c_str(), 0755);
            rep.open(prefix + "render_report.txt");
            rep << "# keyframe hits off_band_hits rmse psnr_db robust_energy  (residual = keyframe - albedo x shading over the hit pixels, RGB in [0, 1])\n";
        }
        psgsdf_view v0{}; int32_t W = 0, H = 0;
        if (int rc = psgsdf_render_size(ctx_, &v0, &W, &H)) return fail("psgsdf_render_size", rc);
        const size_t HW = (size_t)W * H;
        std::vector<float> planes(10 * HW);
        std::vector<uint8_t> px(3 * HW);
        bool ok = !lead || rep.is_open();
        for (int f = 0; f < F; ++f) {
            const std::string name = f < (int)key_stamps_.size() ? key_stamps_[f] : std::to_string(f);
            psgsdf_view v{}; v.frame = f;
            psgsdf_render_stats st{};
            if (int rc = psgsdf_render(ctx_, &v, PSGSDF_R_ALBEDO | PSGSDF_R_SHADING | PSGSDF_R_RENDERED | PSGSDF_R_RESIDUAL, planes.data(), &st)) return fail("psgsdf_render", rc);
            if (!lead) continue;
            // planes in bit order: albedo 3 | shading 1 | rendered 3 | residual 3
            auto rgb = [&](size_t plane0, float bias, const char* what) {
                for (size_t i = 0; i < HW; ++i) for (int c = 0; c < 3; ++c) px[3 * i + c] = psgsdf_host::unit_to_u8(bias + planes[(plane0 + c) * HW + i]);
                ok &= psgsdf_host::write_png(dir + name + "_" + what + ".png", W, H, 3, px.data());
            };
            rgb(4, 0.f, "rendered"); rgb(0, 0.f, "albedo"); rgb(7, 0.5f, "residual");
            for (size_t i = 0; i < HW; ++i) px[i] = psgsdf_host::unit_to_u8(planes[3 * HW + i]);
            ok &= psgsdf_host::write_png(dir + name + "_shading.png", W, H, 1, px.data());
            const double r2 = rows[f].sum_r2[0] + rows[f].sum_r2[1] + rows[f].sum_r2[2];
            const double mse = rows[f].n_hits ? r2 / (3.0 * rows[f].n_hits) : 0.0;
            char line[256];
            snprintf(line, sizeof(line), "%s %lld %lld %.6g %.4f %.6g\n", name.c_str(), (long long)rows[f].n_hits, (long long)rows[f].n_hits_off_band, std::sqrt(mse),
                     mse > 0 ? 10.0 * std::log10(1.0 / mse) : 0.0, rows[f].robust);
            rep << line;
        }
        return ok;
    }

    // `--relight FILE`: every keyframe's view under every light of the file, with cast shadows (psgsdf_relight): relight/<keyframe>_light<NN>.png
    // (the rendered plane through the 8-bit colour rule), relight/<keyframe>_light<NN>_visibility.png (grey) and one line of counts per keyframe
    // and light in relight_report.txt.  Single process only (refused while parsing otherwise).
    bool relightKeyframes(const std::string& prefix, const RelightSpec& spec) {
        if (!ctx_) return false;
        const int F = (int)num_frames_, L = (int)spec.lights.size();
        const std::string dir = prefix + "relight/";
        ::mkdir(dir.c_str(), 0755);
        std::ofstream rep(prefix + "relight_report.txt");
        rep << "# keyframe light kind samples hits lit rays occluded buried\n";
        psgsdf_view v0{}; int32_t W = 0, H = 0;
        if (int rc = psgsdf_render_size(ctx_, &v0, &W, &H)) return fail("psgsdf_render_size", rc);
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        psgsdf_relight_params par{};
        par.bias = spec.bias_voxels * (double)info.voxel_size; par.reach = spec.reach_voxels * (double)info.voxel_size; par.n_lights = L;
        const size_t HW = (size_t)W * H;
        std::vector<float> planes((size_t)L * 4 * HW);
        std::vector<psgsdf_relight_counts> counts(L);
        std::vector<uint8_t> px(3 * HW);
        bool ok = rep.is_open();
        static const char* kinds[3] = {"sh", "directional", "point"};
        for (int f = 0; f < F; ++f) {
            const std::string name = f < (int)key_stamps_.size() ? key_stamps_[f] : std::to_string(f);
            psgsdf_view v{}; v.frame = f;
            if (int rc = psgsdf_relight(ctx_, &v, spec.lights.data(), &par, planes.data(), nullptr, counts.data())) return fail("psgsdf_relight", rc);
            for (int l = 0; l < L; ++l) {
                const float* p = planes.data() + (size_t)l * 4 * HW;
                char tag[32]; snprintf(tag, sizeof(tag), "_light%02d", l);
                for (size_t i = 0; i < HW; ++i) for (int c = 0; c < 3; ++c) px[3 * i + c] = psgsdf_host::unit_to_u8(p[c * HW + i]);
                ok &= psgsdf_host::write_png(dir + name + tag + ".png", W, H, 3, px.data());
                for (size_t i = 0; i < HW; ++i) px[i] = psgsdf_host::unit_to_u8(p[3 * HW + i]);
                ok &= psgsdf_host::write_png(dir + name + tag + "_visibility.png", W, H, 1, px.data());
                const psgsdf_relight_counts& k = counts[l];
                char line[256];
                snprintf(line, sizeof(line), "%s %d %s %d %lld %lld %lld %lld %lld\n", name.c_str(), l, kinds[spec.lights[l].kind], (int)spec.lights[l].n_shadow, (long long)k.n_hits,
                         (long long)k.n_lit, (long long)k.n_rays, (long long)k.n_occluded, (long long)k.n_buried);
                rep << line;
            }
        }
        return ok;
    }

    // PsOptimizer::init / LedOptimizer::init (PsOptimizer.cpp:25-42): with zero keyframes (the constructor-time
    // call of the reference) this is a no-op; with keyframes it creates the device context and uploads everything.
    virtual void init() {
        PSG_STAGE("optimiser init: keyframe upload + band");
        num_frames_ = frame_idx_.size();
        num_voxels_ = tSDF_->num_voxels();
        if (num_frames_ == 0) return;
        if (tSDF_->ctx) {   // device-resident volume: the fused state is already there
            ctx_ = tSDF_->ctx; borrowed_ = true;
            if (multi_rank()) { const int rb = psgsdf_rebalance_slabs(ctx_); if (rb) { fail("psgsdf_rebalance_slabs", rb); return; } }      // fused in slabs of equal height, optimised in slabs of equal band count
            const int W = images_[0]->cols, H = images_[0]->rows;
            std::vector<float> P(num_frames_ * 16); std::vector<const float*> img(num_frames_);
            for (size_t f = 0; f < num_frames_; ++f) {
                if (images_[f]->cols != W || images_[f]->rows != H) { std::cerr << "keyframe " << f << " has another size" << std::endl; return; }
                img[f] = images_[f]->data.data();      // (one allocation per image, like the reference's std::vector<cv::Mat>: no gather)
                std::copy(poses_[f].begin(), poses_[f].end(), P.begin() + f * 16);
            }
            int rc = psgsdf_set_keyframes_frames(ctx_, (int)num_frames_, frame_idx_.data(), img.data(), W, H, P.data());
            if (rc) { fail("psgsdf_set_keyframes", rc); return; }
            rc = psgsdf_init(ctx_);
            if (rc) fail("psgsdf_init", rc);
            return;
        }
        if (ctx_) { psgsdf_destroy(ctx_); ctx_ = nullptr; }
        psgsdf_grid_desc g{};
        for (int a = 0; a < 3; ++a) { g.dim[a] = tSDF_->grid_dim_[a]; g.shift[a] = tSDF_->shift_[a]; }
        g.voxel_size = voxel_size_; g.truncation = tSDF_->T_;
        psgsdf_settings s{};
        s.model = settings_->model == LED ? PSGSDF_LED : (settings_->model == SH2 ? PSGSDF_SH2 : PSGSDF_SH1);
        s.loss = (int)settings_->loss; s.lambda = settings_->lambda; s.damping = settings_->damping;
        s.reg_weight_rho = settings_->reg_weight_rho; s.reg_weight_n = settings_->reg_weight_n; s.reg_weight_l = settings_->reg_weight_l;
        s.max_it = settings_->max_it; s.conv_threshold = settings_->conv_threshold; s.upsample = settings_->upsample ? 1 : 0;
        s.ref_quirks = 1; s.cg_max_it = 0;
        int rc = psgsdf_create(&g, K_.v, &s, 0, &ctx_);
        if (rc) { fail("psgsdf_create", rc); ctx_ = nullptr; return; }
        rc = psgsdf_upload_volume(ctx_, tSDF_->dist.data(), tSDF_->grad.data(), tSDF_->weight.data(), tSDF_->rgb.data(), tSDF_->vis.data(), tSDF_->vis_words);
        if (rc) { fail("psgsdf_upload_volume", rc); return; }
        const int W = images_[0]->cols, H = images_[0]->rows;
        std::vector<float> img((size_t)num_frames_ * W * H * 3), P(num_frames_ * 16);
        for (size_t f = 0; f < num_frames_; ++f) {
            std::copy(images_[f]->data.begin(), images_[f]->data.end(), img.begin() + f * (size_t)W * H * 3);
            std::copy(poses_[f].begin(), poses_[f].end(), P.begin() + f * 16);
        }
        rc = psgsdf_set_keyframes(ctx_, (int)num_frames_, frame_idx_.data(), img.data(), W, H, P.data());
        if (rc) { fail("psgsdf_set_keyframes", rc); return; }
        rc = psgsdf_init(ctx_);
        if (rc) fail("psgsdf_init", rc);
    }

    // alternatingOptimize (PsOptimizer.cpp:239-428 / LedOptimizer.cpp:279-478): true = converged
    virtual bool alternatingOptimize(bool light, bool albedo, bool distance, bool pose) {
        PSG_STAGE("alternatingOptimize: total (incl. its dumps)");
        if (!ctx_) return false;
        if (lead_rank()) doc_.open((save_path_ + "optimizer_doc.txt").c_str());
        std::cout << "albation study settings: \n" << "light: " << light << "\n" << "albedo: " << albedo << "\n" << "distance: " << distance << "\n" << "pose: " << pose << std::endl;
        if (doc_.is_open()) doc_ << "albation study settings: \t" << "light: " << light << "\t" << "albedo: " << albedo << "\t" << "distance: " << distance << "\t" << "pose: " << pose
             << "\n" << "num of key frame: " << num_frames_ << " \n total voxels: " << num_voxels_ << "\n";
        int flags = (albedo ? PSGSDF_ALBEDO : 0) | (light ? PSGSDF_LIGHT : 0) | (distance ? PSGSDF_DIST : 0) | (pose ? PSGSDF_POSE : 0);
        std::vector<psgsdf_iter_stats> recs(settings_->max_it + 1);
        int n_done = 0, result = 0;
        psgsdf_set_record_observer(ctx_, &Optimizer::narrate_trampoline, this);
        psgsdf_set_on_iter_period(ctx_, 3);
        int rc = psgsdf_optimize(ctx_, flags, recs.data(), (int)recs.size(), &n_done, &result, &Optimizer::on_iter_trampoline, this);
        psgsdf_set_record_observer(ctx_, nullptr, nullptr);
        if (rc) return fail("psgsdf_optimize", rc);
        if (n_done > 0 && (recs[n_done - 1].converged || recs[n_done - 1].diverged)) {
            const int iter = n_done - 1;
            narrate(n_done, &recs[n_done - 1]);   // (the observer is not invoked for the terminating iteration.  Narration only: the reference returns at PsOptimizer.cpp:368-384, before ++iter and the iter % 3 dumps of :419-423 -- no after_iter_<k> files for it)
            std::cout << "===> [" << iter << "]: " << (result ? "converged!" : "diverged!") << std::endl;
            if (doc_.is_open()) doc_ << "===> [" << iter << "]: " << (result ? "converged! \n" : "diverged!\n");
            save_pointcloud("final_refined");                      // PsOptimizer.cpp:372-373,379-380
            extract_mesh("final_refined");
            if (settings_->model == LED) saveSDF("refined_sdf.sdf");   // LedOptimizer.cpp:422,430
        }
        // the reference mutates the shared settings (B9): report the effective weights back the same way
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        settings_->reg_weight_n = info.reg_weight_n; settings_->reg_weight_l = info.reg_weight_l;
        sync_back();
        if (doc_.is_open()) doc_.close();
        DumpQueue::get().drain();      // the reference has written its files when alternatingOptimize returns
        if (multi_rank()) { double one = 1; psgsdf_comm_allreduce_host(ctx_, &one, 1); }      // ... on every rank
        return result != 0;
    }

    // copy the refined state back into tSDF_ / poses_ (the reference mutates them in place)
    bool sync_back() {
        PSG_STAGE("sync back: refined volume to host");
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        size_t n = (size_t)info.dim[0] * info.dim[1] * info.dim[2];
        for (int a = 0; a < 3; ++a) tSDF_->grid_dim_[a] = info.dim[a];
        tSDF_->voxel_size_ = info.voxel_size; voxel_size_ = info.voxel_size;
        const bool no_volume = multi_rank() || skip_sync_back();      // (a rank holds a slab: no whole-volume host copy; nothing in voxelPS reads one after the optimisation)
        if (no_volume) n = 0;
        tSDF_->dist.resize(n); tSDF_->grad.resize(3 * n); tSDF_->weight.resize(n); tSDF_->rgb.resize(3 * n);
        tSDF_->vis.resize(n * info.vis_words); tSDF_->vis_words = info.vis_words;
        int rc = no_volume ? 0 : psgsdf_download_volume(ctx_, tSDF_->dist.data(), tSDF_->grad.data(), tSDF_->weight.data(), tSDF_->rgb.data(), tSDF_->vis.data());
        if (rc) return fail("psgsdf_download_volume", rc);
        std::vector<float> P(num_frames_ * 16);
        rc = psgsdf_download_poses(ctx_, P.data());
        if (rc) return fail("psgsdf_download_poses", rc);
        for (size_t f = 0; f < num_frames_; ++f) std::copy(P.begin() + 16 * f, P.begin() + 16 * f + 16, poses_[f].begin());
        return true;
    }

    // savePoses, OptimizerAux.cpp:580-599: "stamp tx ty tz qx qy qz qw" with Eigen's matrix->quaternion conversion
    bool savePoses(std::string filename) {
        PSG_STAGE("dump: poses");
        std::vector<float> P(num_frames_ * 16);
        if (psgsdf_download_poses(ctx_, P.data())) return false;
        if (!lead_rank()) return true;
        std::ofstream posefile((save_path_ + filename + ".txt").c_str());
        if (!posefile.is_open()) { std::cout << "couldn't save optimized poses! " << std::endl; return false; }
        for (size_t i = 0; i < num_frames_; ++i) {
            const float* M = &P[16 * i];
            float q[4];   // x y z w, Eigen::QuaternionBase::operator=(Matrix3)
            float t = M[0] + M[5] + M[10];
            if (t > 0) { t = std::sqrt(t + 1.0f); q[3] = 0.5f * t; t = 0.5f / t; q[0] = (M[9] - M[6]) * t; q[1] = (M[2] - M[8]) * t; q[2] = (M[4] - M[1]) * t; }
            else {
                int a = 0; if (M[5] > M[0]) a = 1; if (M[10] > M[a * 5]) a = 2;
                int b = (a + 1) % 3, c = (b + 1) % 3;
                t = std::sqrt(M[a * 5] - M[b * 5] - M[c * 5] + 1.0f);
                q[a] = 0.5f * t; t = 0.5f / t;
                q[3] = (M[c * 4 + b] - M[b * 4 + c]) * t; q[b] = (M[b * 4 + a] + M[a * 4 + b]) * t; q[c] = (M[c * 4 + a] + M[a * 4 + c]) * t;
            }
            posefile << (i < key_stamps_.size() ? key_stamps_[i] : std::to_string(i)) << " " << M[3] << " " << M[7] << " " << M[11] << " "
                     << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << "\n";
        }
        return true;
    }

    // save_pointcloud, OptimizerAux.cpp:456-511 (grid-local coordinates: vox2float, origin not added)
    bool save_pointcloud(std::string filename) {
        PSG_STAGE("dump: point cloud");
        if (!host_writers()) return VolumetricGradSdf::device_pointcloud(ctx_, 0, save_path_ + filename + "_pointcloud.ply");
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        size_t n = (size_t)info.dim[0] * info.dim[1] * info.dim[2];
        std::vector<float> d(n), g(3 * n), rgb(3 * n); std::vector<int32_t> band(info.n_band);
        if (psgsdf_download_volume(ctx_, d.data(), g.data(), nullptr, rgb.data(), nullptr) || psgsdf_download_band(ctx_, band.data())) return false;
        std::ofstream ply((save_path_ + filename + "_pointcloud.ply").c_str());
        if (!ply.is_open()) { std::cout << " can't save point cloud!" << std::endl; return false; }
        size_t cnt = 0;
        for (int lin : band) if (std::abs(d[lin]) < std::sqrt(3.0) * info.voxel_size) ++cnt;
        ply << "ply\nformat ascii 1.0\nelement vertex " << cnt << "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            << "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header" << std::endl;
        const int nx = info.dim[0], nxy = info.dim[0] * info.dim[1];
        for (int lin : band) {
            if (!(std::abs(d[lin]) < std::sqrt(3.0) * info.voxel_size)) continue;
            int k = lin / nxy, rest = lin - k * nxy, j = rest / nx, i = rest - j * nx;
            float gv[3] = {g[lin], g[n + lin], g[2 * n + lin]};
            float z = gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2];
            if (z > 0) { float s = std::sqrt(z); gv[0] /= s; gv[1] /= s; gv[2] /= s; }
            float p[3] = {info.voxel_size * i - d[lin] * gv[0], info.voxel_size * j - d[lin] * gv[1], info.voxel_size * k - d[lin] * gv[2]};
            ply << p[0] << " " << p[1] << " " << p[2] << " " << gv[0] << " " << gv[1] << " " << gv[2] << " "
                << int(255 * rgb[lin]) << " " << int(255 * rgb[n + lin]) << " " << int(255 * rgb[2 * n + lin]) << std::endl;
        }
        return true;
    }

    // extract_mesh / saveSDF, OptimizerAux.cpp:278-363,513-577
    bool extract_mesh(std::string filename) {
        PSG_STAGE("dump: mesh (marching cubes + PLY)");
        if (indexed_mesh() && !VolumetricGradSdf::device_mesh_indexed(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the indexed mesh " << save_path_ << filename << std::endl;
        if (clean_mesh() && !VolumetricGradSdf::device_mesh_clean(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the cleaned mesh " << save_path_ << filename << std::endl;
        if (mesh_lod_voxels() > 0 && !VolumetricGradSdf::device_mesh_lod(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the level-of-detail mesh " << save_path_ << filename << std::endl;
        if (mesh_fit() && !VolumetricGradSdf::device_mesh_fit(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the mesh with its fit " << save_path_ << filename << std::endl;
        if (mesh_curvature() && !VolumetricGradSdf::device_mesh_curvature(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the mesh with its curvature " << save_path_ << filename << std::endl;
        if (mesh_fill_rounds() >= 0 && !VolumetricGradSdf::device_mesh_filled(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the filled mesh " << save_path_ << filename << std::endl;
        if (compare_ref().on && !VolumetricGradSdf::device_mesh_compare(ctx_, save_path_ + filename + "_mesh.ply")) std::cout << "couldn't save the comparison " << save_path_ << filename << std::endl;
        if (!host_writers()) {
            const bool ok = VolumetricGradSdf::device_mesh(ctx_, save_path_ + filename + "_mesh.ply");
            if (!ok) std::cout << "couldn't save mesh " << save_path_ << filename << std::endl;
            return ok;
        }
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        size_t n = (size_t)info.dim[0] * info.dim[1] * info.dim[2];
        std::vector<float> d(n), w(n), rgb(3 * n);
        if (psgsdf_download_volume(ctx_, d.data(), nullptr, w.data(), rgb.data(), nullptr)) return false;
        bool ok = write_mesh(save_path_ + filename + "_mesh.ply", info.dim, info.voxel_size, d, w, rgb);
        if (!ok) std::cout << "couldn't save mesh " << save_path_ << filename << std::endl;
        return ok;
    }
    bool saveSDF(std::string filename) {
        PSG_STAGE("dump: sdf");
        if (!host_writers()) { psgsdf_info i2{}; psgsdf_get_info(ctx_, &i2); return VolumetricGradSdf::device_sdf(ctx_, save_path_ + filename, i2.voxel_size); }
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        size_t n = (size_t)info.dim[0] * info.dim[1] * info.dim[2];
        std::vector<float> d(n);
        if (psgsdf_download_volume(ctx_, d.data(), nullptr, nullptr, nullptr, nullptr)) return false;
        return write_sdf(save_path_ + filename, info.dim, info.voxel_size, d);
    }
    psgsdf_ctx* context() { return ctx_; }
};

// PsOptimizer.h / LedOptimizer.h: the constructor runs init() like the reference (PsOptimizer.cpp:15-23)
class PsOptimizer : public Optimizer {
public:
    PsOptimizer(VolumetricGradSdf* tSDF, const float voxel_size, const Mat3f& K, std::string save_path, OptimizerSettings* settings)
        : Optimizer(tSDF, voxel_size, K, save_path, settings) { init(); }
};
class LedOptimizer : public Optimizer {
public:
    LedOptimizer(VolumetricGradSdf* tSDF, const float voxel_size, const Mat3f& K, std::string save_path, OptimizerSettings* settings)
        : Optimizer(tSDF, voxel_size, K, save_path, settings) { settings_->model = LED; init(); }
};

}  // namespace psgsdf_host
