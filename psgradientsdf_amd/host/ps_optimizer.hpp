// ps_optimizer.hpp — C++ mirror of the reference's optimiser interface over the C ABI (include/psgsdf.h).
//
// Same class / member names, argument meaning and return conventions as
//   ps_optimizer/Optimizer.h:24-182, PsOptimizer.h, LedOptimizer.h, OptimizerSettings.h:24-51
// so that main_ps.cpp:193-202,323-330 reads the same against this header.  The reference's Eigen / OpenCV
// types are replaced by plain structs (none of those libraries is a dependency of this project):
//   Eigen::Matrix4f  -> Mat4f   (row-major 16 floats)        cv::Mat (CV_32FC3, BGR) -> ImageRGB (float RGB)
//   VolumetricGradSdf -> VolumetricGradSdf below: the SoA form of its private tsdf_/vis_ arrays, which the
//   reference's optimisers reach through `friend` access (VolumetricGradSdf.h:25-42).
// All numerical work happens in libpsgsdf.so on the GPU; this header only marshals, narrates, and writes the small text files the reference
// writes from inside alternatingOptimize (optimizer_doc.txt, after_poses_opt_<k>.txt) plus the reference's own dense writers (write_mesh,
// write_sdf, write_pointcloud: the `--host-writers` cross-check).  Everything else a run dumps is issued through device_dumps.hpp (the options record,
// engine call -> owned copy -> queue), the only dump header the classes here need; behind it dump_queue.hpp, ply_io.hpp, text_format.hpp, stage_clock.hpp.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/psgsdf.h"
#include "../../include/psgsdf_render.h"
#include "../../include/psgsdf_relight.h"
#include "device_dumps.hpp"
#include "marching_cubes.hpp"

namespace psgsdf_host {

using Mat4f = std::array<float, 16>;                 // row-major camera->world
struct Mat3f { float v[9]; };                        // row-major intrinsics
struct ImageRGB { int rows = 0, cols = 0; std::vector<float> data; };   // rows*cols*3, RGB in [0,1]
inline void quat_of(const float* M, float q[4]) {   // the rotation of a row-major 4x4 as Eigen::Quaternionf(Matrix3f) gives it: x y z w
    float t = M[0] + M[5] + M[10];
    if (t > 0) { t = std::sqrt(t + 1.0f); q[3] = 0.5f * t; t = 0.5f / t; q[0] = (M[9] - M[6]) * t; q[1] = (M[2] - M[8]) * t; q[2] = (M[4] - M[1]) * t; }
    else { int a = 0; if (M[5] > M[0]) a = 1; if (M[10] > M[a * 5]) a = 2; int b = (a + 1) % 3, c = (b + 1) % 3;
        t = std::sqrt(M[a * 5] - M[b * 5] - M[c * 5] + 1.0f); q[a] = 0.5f * t; t = 0.5f / t;
        q[3] = (M[c * 4 + b] - M[b * 4 + c]) * t; q[b] = (M[b * 4 + a] + M[a * 4 + b]) * t; q[c] = (M[c * 4 + a] + M[a * 4 + c]) * t; }
}

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
// the reference's point-cloud loop (extract_pc VolumetricGradSdf.cpp:320-376, save_pointcloud OptimizerAux.cpp:456-511: grid-local coordinates, vox2float,
// origin not added) over the voxels `sel` of a dense volume: x y z nx ny nz r g b
inline bool write_pointcloud(const std::string& file, const std::vector<size_t>& sel, const int dim[3], float vs, const std::vector<float>& dist, const std::vector<float>& grad, const std::vector<float>& rgb) {
    std::ofstream ply(file.c_str()); if (!ply.is_open()) return false;
    ply << pointcloud_header(sel.size()) << std::flush;
    const size_t n = (size_t)dim[0] * dim[1] * dim[2]; const int nx = dim[0], nxy = dim[0] * dim[1];
    for (size_t lin : sel) {
        int k = (int)(lin / nxy), rest = (int)(lin - (size_t)k * nxy), j = rest / nx, i = rest - j * nx;
        float g[3] = {grad[lin], grad[n + lin], grad[2 * n + lin]}; float z = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
        if (z > 0) { float s = std::sqrt(z); g[0] /= s; g[1] /= s; g[2] /= s; }
        ply << vs * i - dist[lin] * g[0] << " " << vs * j - dist[lin] * g[1] << " " << vs * k - dist[lin] * g[2] << " " << g[0] << " " << g[1] << " " << g[2] << " "
            << int(255 * rgb[lin]) << " " << int(255 * rgb[n + lin]) << " " << int(255 * rgb[2 * n + lin]) << std::endl;
    }
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
        if (dump_options().host_writers) {      // (round 4's path: the normals come back to the host and go up again)
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
        if (ctx) device_mesh_extras(ctx, filename, "of " + filename);
        if (ctx && !dump_options().host_writers) return device_mesh(ctx, filename);
        return sync_host() && write_mesh(filename, grid_dim_, voxel_size_, dist, weight, rgb);
    }
    bool saveSDF(const std::string& filename) {
        PSG_STAGE("dump: sdf");
        if (ctx && !dump_options().host_writers) return device_sdf(ctx, filename, voxel_size_);
        return sync_host() && write_sdf(filename, grid_dim_, voxel_size_, dist);
    }
    // extract_pc, VolumetricGradSdf.cpp:320-376: x y z nx ny nz r g b of every voxel with |d| < sqrt(3) vs and weight > 0
    bool extract_pc(const std::string& filename) {
        PSG_STAGE("dump: point cloud");
        if (ctx && !dump_options().host_writers) return device_pointcloud(ctx, 1, filename);
        if (!sync_host()) return false;
        const size_t n = num_voxels(); std::vector<size_t> sel;
        for (size_t lin = 0; lin < n; ++lin) if (weight[lin] > 0 && std::fabs(dist[lin]) < std::sqrt(3) * voxel_size_) sel.push_back(lin);
        return write_pointcloud(filename, sel, grid_dim_, voxel_size_, dist, grad, rgb);
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
        const bool no_volume = multi_rank() || dump_options().skip_sync_back;      // (a rank holds a slab: no whole-volume host copy; nothing in voxelPS reads one after the optimisation)
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
            float q[4]; quat_of(M, q);
            posefile << (i < key_stamps_.size() ? key_stamps_[i] : std::to_string(i)) << " " << M[3] << " " << M[7] << " " << M[11] << " "
                     << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << "\n";
        }
        return true;
    }

    // save_pointcloud, OptimizerAux.cpp:456-511 (grid-local coordinates: vox2float, origin not added)
    bool save_pointcloud(std::string filename) {
        PSG_STAGE("dump: point cloud");
        if (!dump_options().host_writers) return device_pointcloud(ctx_, 0, save_path_ + filename + "_pointcloud.ply");
        psgsdf_info info{}; psgsdf_get_info(ctx_, &info);
        size_t n = (size_t)info.dim[0] * info.dim[1] * info.dim[2];
        std::vector<float> d(n), g(3 * n), rgb(3 * n); std::vector<int32_t> band(info.n_band);
        if (psgsdf_download_volume(ctx_, d.data(), g.data(), nullptr, rgb.data(), nullptr) || psgsdf_download_band(ctx_, band.data())) return false;
        std::vector<size_t> sel;
        for (int lin : band) if (std::abs(d[lin]) < std::sqrt(3.0) * info.voxel_size) sel.push_back((size_t)lin);
        if (!write_pointcloud(save_path_ + filename + "_pointcloud.ply", sel, info.dim, info.voxel_size, d, g, rgb)) { std::cout << " can't save point cloud!" << std::endl; return false; }
        return true;
    }

    // extract_mesh / saveSDF, OptimizerAux.cpp:278-363,513-577
    bool extract_mesh(std::string filename) {
        PSG_STAGE("dump: mesh (marching cubes + PLY)");
        device_mesh_extras(ctx_, save_path_ + filename + "_mesh.ply", save_path_ + filename);
        if (!dump_options().host_writers) {
            const bool ok = device_mesh(ctx_, save_path_ + filename + "_mesh.ply");
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
        if (!dump_options().host_writers) { psgsdf_info i2{}; psgsdf_get_info(ctx_, &i2); return device_sdf(ctx_, save_path_ + filename, i2.voxel_size); }
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
