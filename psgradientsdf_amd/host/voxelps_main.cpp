// voxelPS — drop-in for the reference executable: `voxelPS --config_file <config.json>` (cpp/voxel_ps/src/main_ps.cpp:41-343),
// same JSON keys (ConfigLoader.h:16-170), same exit codes, same output files under the "output" prefix.  Every numerical
// stage runs on the GPU through libpsgsdf.so: FALS normals, depth tracking, fusion, the photometric-stereo optimisation.
// Extra optional keys: "grid dim" (default 128, main_ps.cpp:123), "max keyframes" (default 40, :312).
#include "image_loader.hpp"
#include "mini_json.hpp"
#include <signal.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/wait.h>

using namespace psgsdf_host;

// compute_centroid, main_ps.cpp:346-375.  A float running sum over ~1e6 pixels, in the reference's order of operations (R * p, + t, += into the
// float accumulator; / float(counter)): the grid origin must be the reference's to the bit, not a better-rounded one.
static void compute_centroid(const Mat3f& K, const DepthImage& depth, const Mat4f& T, float out[3]) {
    float c[3] = {0.f, 0.f, 0.f}; int counter = 0;
    const float fx_inv = 1.f / K.v[0], fy_inv = 1.f / K.v[4], cx = K.v[2], cy = K.v[5];
    for (int y = 0; y < depth.rows; ++y) for (int x = 0; x < depth.cols; ++x) {
        float z = depth.data[(size_t)y * depth.cols + x];
        if (z > 0.0) {
            const float x0 = (float(x) - cx) * fx_inv, y0 = (float(y) - cy) * fy_inv;
            const float p[3] = {x0 * z, y0 * z, z};
            for (int a = 0; a < 3; ++a) { const float rp = (T[a * 4] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]; c[a] += rp + T[a * 4 + 3]; }
            ++counter;
        }
    }
    for (int a = 0; a < 3; ++a) out[a] = c[a] / float(counter);
}
// sampleKeyFrame, main_ps.cpp:392-421
template <class A, class B, class C_, class D>
static void sampleKeyFrame(A& frames, B& stamps, C_& images, D& poses, int max_num) {
    if ((int)frames.size() < max_num) return;
    max_num -= 1;
    float step = static_cast<float>(frames.size()) / static_cast<float>(max_num), idx = 0;
    A f2; B s2; C_ i2; D p2;
    for (int count = 0; count < max_num; ++count) { int i = static_cast<int>(idx); f2.push_back(frames[i]); s2.push_back(stamps[i]); i2.push_back(images[i]); p2.push_back(poses[i]); idx += step; }
    f2.push_back(frames.back()); s2.push_back(stamps.back()); i2.push_back(images.back()); p2.push_back(poses.back());
    frames = f2; stamps = s2; images = i2; poses = p2;
}

// host-side self tests that need no GPU (tests/test_host_tools.py): PNG decoding and the generated marching-cubes table
static int selftest_png(const char* path) {
    PngImage p; if (!read_png(path, p)) { std::cout << "FAIL" << std::endl; return 1; }
    unsigned long long sum = 0; for (uint16_t v : p.px) sum += v;
    std::cout << p.width << " " << p.height << " " << p.channels << " " << p.bit_depth << " " << sum << std::endl; return 0;
}
// `--selftest-png-write out.png`: a 37 x 23 RGB pattern through the PNG writer (tests/test_render_cpu.py decodes it with PIL)
static int selftest_png_write(const char* path) {
    const int W = 37, H = 23;
    std::vector<uint8_t> px(3 * W * H);
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) { uint8_t* p = &px[3 * (y * W + x)]; p[0] = (uint8_t)(7 * x); p[1] = (uint8_t)(11 * y); p[2] = (uint8_t)(x * y); }
    return psgsdf_host::write_png(path, W, H, 3, px.data()) ? 0 : 1;
}
static int selftest_mc() {
    int dim[3] = {24, 24, 24}; float size[3] = {24, 24, 24}, org[3] = {0, 0, 0};
    MarchingCubes mc(dim, size, org);
    int ntri = 0; for (int c = 0; c < 256; ++c) ntri += (int)mc.table(c).size() / 3;
    std::vector<float> t(24 * 24 * 24), w(t.size(), 1.f); std::vector<unsigned char> col(t.size() + 2, 128);
    for (int k = 0; k < 24; ++k) for (int j = 0; j < 24; ++j) for (int i = 0; i < 24; ++i) { float dx = i - 11.3f, dy = j - 11.7f, dz = k - 11.1f; t[(k * 24 + j) * 24 + i] = 7.2f - std::sqrt(dx * dx + dy * dy + dz * dz); }
    mc.computeIsoSurface(t.data(), w.data(), col.data(), col.data(), col.data());
    // closedness by the divergence theorem: the signed volume must not depend on the origin it is taken from, and the area vectors sum to 0
    double vol = 0, vol2 = 0, area = 0, asum[3] = {0, 0, 0}, maxr = 0, minr = 1e9; auto& v = mc.vertices();
    const double o2[3] = {40.5, -17.25, 3.125};
    for (size_t f = 0; f + 2 < v.size(); f += 3) {
        double a[3], b[3], c[3], a2[3], b2[3], c2[3];
        for (int q = 0; q < 3; ++q) { a[q] = v[f][q]; b[q] = v[f + 1][q]; c[q] = v[f + 2][q]; a2[q] = a[q] - o2[q]; b2[q] = b[q] - o2[q]; c2[q] = c[q] - o2[q]; }
        vol += (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0])) / 6.0;
        vol2 += (a2[0] * (b2[1] * c2[2] - b2[2] * c2[1]) - a2[1] * (b2[0] * c2[2] - b2[2] * c2[0]) + a2[2] * (b2[0] * c2[1] - b2[1] * c2[0])) / 6.0;
        double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        double n[3] = {u[1] * w2[2] - u[2] * w2[1], u[2] * w2[0] - u[0] * w2[2], u[0] * w2[1] - u[1] * w2[0]};
        area += 0.5 * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]); for (int q = 0; q < 3; ++q) asum[q] += 0.5 * n[q];
        for (int q = 0; q < 3; ++q) { double r = std::sqrt(std::pow(v[f + q][0] - 11.3, 2) + std::pow(v[f + q][1] - 11.7, 2) + std::pow(v[f + q][2] - 11.1, 2)); maxr = std::max(maxr, r); minr = std::min(minr, r); } }
    std::cout.precision(12);
    std::cout << ntri << " " << mc.num_faces() << " " << vol << " " << minr << " " << maxr << " " << vol2 << " " << area << " " << std::sqrt(asum[0] * asum[0] + asum[1] * asum[1] + asum[2] * asum[2]) << std::endl; return 0;
}
// the 256-case triangle table in use, one line per case: `case n_triangles e0 e1 e2 ...` (edge ids of the reference's numbering);
// generated = true: the first-principles table of round 1 (cross-check)
static int selftest_mc_table(bool generated) {
    int dim[3] = {4, 4, 4}; float size[3] = {4, 4, 4}, org[3] = {0, 0, 0};
    MarchingCubes mc(dim, size, org);
    for (int c = 0; c < 256; ++c) { const std::vector<int>& t = generated ? mc.generated_table(c) : mc.table(c); std::cout << c << " " << t.size() / 3; for (int e : t) std::cout << " " << e; std::cout << "\n"; }
    return 0;
}
// a mesh of a small analytic volume, written the way the product writes it: `--selftest-mc-ply N out.ply` (an off-centre bumpy sphere in an N^3 grid
// with a weight-0 corner region and varying colours): tests/test_host_tools.py re-derives it face by face
static int selftest_mc_ply(int n, const char* path) {
    int dim[3] = {n, n, n}; float size[3] = {0.5f * n, 0.5f * n, 0.5f * n}, org[3] = {0.1f, -0.2f, 0.3f};
    MarchingCubes mc(dim, size, org);
    std::vector<float> t((size_t)n * n * n), w(t.size(), 1.f); std::vector<unsigned char> r(t.size() + 2), g(t.size() + 2), b(t.size() + 2);
    for (int k = 0; k < n; ++k) for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) {
        const size_t l = ((size_t)k * n + j) * n + i;
        const float dx = i - 0.47f * n, dy = j - 0.52f * n, dz = k - 0.45f * n;
        t[l] = 0.31f * n + 0.6f * std::sin(0.9f * i) * std::cos(0.7f * j + 0.3f * k) - std::sqrt(dx * dx + dy * dy + dz * dz);
        if (i + j + k < n / 2) w[l] = 0.f;
        r[l] = (unsigned char)((37 * i + 11 * j) & 255); g[l] = (unsigned char)((5 * j + 91 * k) & 255); b[l] = (unsigned char)((17 * k + 3 * i) & 255);
    }
    mc.computeIsoSurface(t.data(), w.data(), r.data(), g.data(), b.data());
    return mc.savePly(path) ? 0 : 1;
}

// the fixture of the writers' self tests: a fixed octahedron (6 vertices, 8 outward-wound faces, unit normals), its grid origin and voxel size
namespace octa {
const float xyz[6][3] = {{1.5f, 0, 0}, {-1.5f, 0, 0}, {0, 2.25f, 0}, {0, -2.25f, 0}, {0, 0, 0.75f}, {0, 0, -0.75f}};
const float nrm[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
const uint8_t rgb[6][3] = {{255, 0, 0}, {0, 255, 0}, {0, 0, 255}, {1, 2, 3}, {128, 64, 32}, {7, 77, 177}};
const int32_t faces[8][3] = {{0, 2, 4}, {2, 1, 4}, {1, 3, 4}, {3, 0, 4}, {2, 0, 5}, {1, 2, 5}, {3, 1, 5}, {0, 3, 5}};
const float origin[3] = {-0.25f, 0.5f, 1.0f}, vs = 0.004f;
const MeshView mesh{&xyz[0][0], &nrm[0][0], &rgb[0][0], 6, &faces[0][0], 8};
}
// `--selftest-ply-indexed out.ply`: the octahedron through the binary writer of the welded mesh (tests/test_mesh_indexed_cpu.py parses it back)
static int selftest_ply_indexed(const char* path) { return write_mesh_indexed_ply(path, octa::mesh, octa::origin, octa::vs) ? 0 : 1; }

// `--selftest-ply-fit out.ply`: the octahedron with the columns and the header line of `--mesh-fit` (tests/test_fit_cpu.py parses it back)
static int selftest_ply_fit(const char* path) {
    const float rms[6] = {0.125f, 0.03125f, 0.0f, 0.25f, 0.0625f, 0.5f}, loss[6] = {0.75f, 0.01f, 0.0f, 1.5f, 0.02f, 2.25f};
    const int32_t n_obs[6] = {3, 8, 0, 1, 16, 2};
    return write_mesh_indexed_ply(path, octa::mesh, octa::origin, octa::vs, mesh_fit_comment(rms, n_obs, 6), {ply_column("quality", rms), ply_column("loss", loss), ply_column("n_obs", n_obs)}) ? 0 : 1;
}

// `--selftest-ply-curvature out.ply`: the octahedron with the columns and the header line of `--mesh-curvature` (tests/test_curvature_cpu.py parses it back)
static int selftest_ply_curvature(const char* path) {
    const float mean[6] = {0.5f, -0.25f, 0.0f, 8.0f, 0.125f, -3.0f}, gauss[6] = {0.25f, 0.0625f, 0.0f, -4.0f, 0.01f, 9.0f};
    const float k1[6] = {0.75f, -0.125f, 0.0f, 16.0f, 0.25f, -3.0f}, k2[6] = {0.25f, -0.375f, 0.0f, -0.25f, 0.04f, -3.0f};
    const uint8_t valid[6] = {2, 1, 0, 2, 1, 2};
    return write_mesh_indexed_ply(path, octa::mesh, octa::origin, octa::vs, mesh_curvature_comment(mean, valid, 6),
                                  {ply_column("quality", mean), ply_column("gauss", gauss), ply_column("k1", k1), ply_column("k2", k2), ply_column("curvature_valid", valid)}) ? 0 : 1;
}

// `--selftest-ply-filled out.ply`: the octahedron with the column and the header line of `--mesh-fill` (tests/test_fill_cpu.py parses it back)
static int selftest_ply_filled(const char* path) {
    const uint8_t filled[6] = {0, 1, 2, 0, 2, 1};
    return write_mesh_indexed_ply(path, octa::mesh, octa::origin, octa::vs, mesh_filled_comment(3, 4, 17, 12, 0), {ply_column("filled", filled)}) ? 0 : 1;
}

// `--selftest-ply-compare out.ply`: the octahedron with the columns of `--compare-ply` and one more header line (tests/test_compare_cpu.py parses it
// back) and back through the reader of `--compare-ply`, which has to skip what it does not want by the declared sizes: 0 iff the positions and faces
// it returns are the ones written
static int selftest_ply_compare(const char* path) {
    const float dist[6] = {0.125f, 0.03125f, 0.0f, INFINITY, 0.0625f, 0.5f};
    const int8_t side[6] = {1, -1, 0, 0, -1, 1};
    if (!write_mesh_indexed_ply(path, octa::mesh, octa::origin, octa::vs, "comment compare selftest\n", {ply_column("distance", dist), ply_column("side", side)})) return 1;
    std::vector<float> rx; std::vector<int32_t> rf; std::string why;
    if (!read_reference_ply(path, rx, rf, why)) { std::cerr << why << std::endl; return 1; }
    return rx.size() == 18 && rf.size() == 24 && memcmp(rx.data(), octa::xyz, sizeof octa::xyz) == 0 && memcmp(rf.data(), octa::faces, sizeof octa::faces) == 0 ? 0 : 1;
}

// `--selftest-obj-bake out.obj`: the octahedron with made-up texture coordinates (dyadic, so that 1 - v is exact) through the writer of
// `--mesh-bake` -- out.obj, out.mtl -- and three normals through the normal map's byte rule into out_normal.png (tests/test_bake_cpu.py parses them back)
static int selftest_obj_bake(const char* path) {
    float uv[8][3][2];
    for (int f = 0; f < 8; ++f) for (int k = 0; k < 3; ++k) { uv[f][k][0] = (3 * f + k) / 32.0f; uv[f][k][1] = (f + k) / 16.0f; }
    std::string base = path;
    if (base.size() > 4 && base.compare(base.size() - 4, 4, ".obj") == 0) base.resize(base.size() - 4);
    const float nm[3][3] = {{1.0f, 0.0f, -1.0f}, {0.0f, 0.0f, 0.0f}, {0.5f, -0.5f, 0.25f}};
    uint8_t px[9];
    for (int q = 0; q < 9; ++q) px[q] = normal_to_u8((&nm[0][0])[q]);
    const bool ok = write_obj_bake(path, base + ".mtl", base + "_albedo.png", base + "_normal.png", octa::mesh.xyz, octa::mesh.normals, octa::mesh.nv, octa::mesh.faces, &uv[0][0][0], octa::mesh.nf);
    return ok && write_png(base + "_normal.png", 3, 1, 3, px) ? 0 : 1;
}

// the focus measure of one colour PNG as the keyframe selector computes it (SharpDetector.h:22-37), and the keyframe sub-sampling of
// main_ps.cpp:392-421 on the index list 0..n-1: tests/test_host_tools.py compares both with numpy / scipy restatements (no GPU needed)
static int selftest_lapm(const char* path) {
    ImageLoader* l = new MultiviewLoader("");
    ImageRGB c; if (!l->load_color(path, c)) { std::cout << "FAIL" << std::endl; return 1; }
    std::cout.precision(9); std::cout << modifiedLaplacian(c) << std::endl; delete l; return 0;
}
static int selftest_sample(int n, int max_num) {
    std::vector<int> frames(n), poses(n), images(n); std::vector<std::string> stamps(n);
    for (int i = 0; i < n; ++i) { frames[i] = 3 * i + 1; poses[i] = i; images[i] = -i; stamps[i] = std::to_string(i); }
    if ((int)frames.size() > max_num) sampleKeyFrame(frames, stamps, images, poses, max_num);      // (the call site's guard, main_ps.cpp:312)
    for (size_t i = 0; i < frames.size(); ++i) std::cout << frames[i] << ":" << stamps[i] << ":" << images[i] << ":" << poses[i] << (i + 1 < frames.size() ? " " : "\n");
    return 0;
}

// the threaded writers print floats with snprintf("%g"), the reference with `ostream << float`: the same characters for EVERY float?  `--selftest-fmt N` formats N
// pseudo-random bit patterns (all exponents, denormals, +-0, inf, nan) and a ladder of round-number cases both ways and counts the differences
static int selftest_fmt(long n) {
    unsigned long long x = 0x9e3779b97f4a7c15ull; long bad = 0, done = 0;
    auto check = [&](float v) {
        TextOut t; t.f(v);
        std::ostringstream o; o << v;
        if (o.str() != t.s) { if (bad < 5) std::cout << "MISMATCH " << o.str() << " vs " << t.s << std::endl; ++bad; }
        ++done;
    };
    auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (long i = 0; i < n; ++i) { uint32_t u = (uint32_t)(rnd() >> 16); float v; memcpy(&v, &u, 4); check(v); }
    // the ranges the dumps live in (the fast path of format_g6): uniform in (-2, 2), log-uniform over 1e-7 .. 1e7, and decimals of seven digits ending in 5
    // -- the floats nearest to a rounding tie of the sixth digit
    for (long i = 0; i < n; ++i) check((float)((double)(rnd() >> 11) * (4.0 / 9007199254740992.0) - 2.0));
    for (long i = 0; i < n; ++i) { const double u = (double)(rnd() >> 11) / 9007199254740992.0; check((float)std::pow(10.0, 14.0 * u - 7.0)); }
    for (long i = 0; i < n; ++i) { const long k = (long)(rnd() % 900000) + 100000; const int e = (int)(rnd() % 16) - 9; const double t = ((double)k * 10.0 + 5.0) * std::pow(10.0, (double)e - 6.0); check((float)t); check(std::nextafter((float)t, 0.0f)); check(std::nextafter((float)t, 1e30f)); }
    for (int e = -45; e <= 38; ++e) for (float m : {1.0f, 9.999995f, 9.9999995f, 1.234565f, 1.2345649f, 0.5f, 2.5f}) { check(m * std::pow(10.0f, (float)e)); check(-m * std::pow(10.0f, (float)e)); }
    for (int i = 0; i <= 255; ++i) check((float)i * (1.0f / 255.0f));
    std::cout << done << " " << bad << std::endl;
    return bad ? 1 : 0;
}

// `--relight FILE`: {"bias_voxels": 1, "reach_voxels": 0, "lights": [{"kind": "sh" | "directional" | "point", "sh": [..], "vec": [..], "colour": [..],
// "ambient": [..], "spread": s, "samples": K}, ...]} into the lights of include/psgsdf_relight.h (defaults: colour 1, ambient 0, spread 0, one
// shadow ray).  false: why says what is wrong with the file.
static bool read_relight_file(const std::string& path, RelightSpec& spec, std::string& why) {
    JsonNode root;
    { std::ifstream f(path); if (!f.is_open()) { why = "cannot read " + path; return false; } }
    if (!root.load(path) || root.kind != JsonNode::OBJECT) { why = path + " is not a JSON object"; return false; }
    auto number = [&](const JsonNode* n, double& out) { if (!n) return true; if (n->kind != JsonNode::NUMBER || !std::isfinite(n->n)) return false; out = n->n; return true; };
    if (!number(root.get("bias_voxels"), spec.bias_voxels) || !(spec.bias_voxels > 0)) { why = "bias_voxels: a number > 0"; return false; }
    if (!number(root.get("reach_voxels"), spec.reach_voxels) || !(spec.reach_voxels >= 0)) { why = "reach_voxels: a number >= 0 (0: no limit)"; return false; }
    const JsonNode* lights = root.get("lights");
    if (!lights || lights->kind != JsonNode::ARRAY || lights->items.empty()) { why = "lights: a list of at least one light"; return false; }
    if (lights->items.size() > PSGSDF_RELIGHT_MAX_LIGHTS) { why = "lights: " + std::to_string(lights->items.size()) + " lights, at most 64"; return false; }
    for (size_t l = 0; l < lights->items.size(); ++l) {
        const JsonNode& n = lights->items[l];
        const std::string at = "light " + std::to_string(l) + ": ";
        if (n.kind != JsonNode::OBJECT) { why = at + "not an object"; return false; }
        psgsdf_light L{};
        const JsonNode* kind = n.get("kind");
        const std::string k = kind && kind->kind == JsonNode::STRING ? kind->s : "";
        if (k == "sh") L.kind = PSGSDF_LIGHT_SH; else if (k == "directional") L.kind = PSGSDF_LIGHT_DIRECTIONAL; else if (k == "point") L.kind = PSGSDF_LIGHT_POINT;
        else { why = at + "kind: sh, directional or point"; return false; }
        // a list of `lo` to `hi` finite numbers into out; its length (0: the key is missing and `need` is false), -1: malformed
        auto floats = [&](const char* key, float* out, int lo, int hi, bool need) {
            const JsonNode* a = n.get(key);
            if (!a) return need ? -1 : 0;
            if (a->kind != JsonNode::ARRAY || (int)a->items.size() < lo || (int)a->items.size() > hi) return -1;
            for (size_t i = 0; i < a->items.size(); ++i) { if (a->items[i].kind != JsonNode::NUMBER || !std::isfinite(a->items[i].n)) return -1; out[i] = (float)a->items[i].n; }
            return (int)a->items.size();
        };
        L.colour[0] = L.colour[1] = L.colour[2] = 1.f;
        if (floats("colour", L.colour, 3, 3, false) < 0 || floats("ambient", L.ambient, 3, 3, false) < 0) { why = at + "colour / ambient: three numbers"; return false; }
        for (int c = 0; c < 3; ++c) if (L.colour[c] < 0.f || L.ambient[c] < 0.f) { why = at + "colour / ambient: >= 0"; return false; }
        double spread = 0.0, samples = L.kind == PSGSDF_LIGHT_SH ? 0.0 : 1.0;
        if (!number(n.get("spread"), spread) || spread < 0) { why = at + "spread: a number >= 0"; return false; }
        if (!number(n.get("samples"), samples)) { why = at + "samples: a number"; return false; }
        L.spread = (float)spread;
        if (L.kind == PSGSDF_LIGHT_SH) {
            const int ns = floats("sh", L.sh, 4, 9, true);
            if (ns != 4 && ns != 9) { why = at + "sh: 4 or 9 coefficients"; return false; }
            L.n_sh = ns;
            if (samples != 0.0 || spread != 0.0) { why = at + "an sh light has no samples and no spread"; return false; }
        } else {
            if (floats("vec", L.vec, 3, 3, true) < 0) { why = at + "vec: three numbers"; return false; }
            if (L.kind == PSGSDF_LIGHT_DIRECTIONAL && L.vec[0] == 0.f && L.vec[1] == 0.f && L.vec[2] == 0.f) { why = at + "vec: a direction of length zero"; return false; }
            if (samples != 1 && samples != 8 && samples != 16 && samples != 32 && samples != 64) { why = at + "samples: 1, 8, 16, 32 or 64"; return false; }
            if (spread > 0 && samples < 8) { why = at + "a spread > 0 needs at least 8 samples"; return false; }
            L.n_shadow = (int)samples;
        }
        spec.lights.push_back(L);
    }
    return true;
}

// `voxelPS --config_file <cfg> --gpus N [--transport rccl|sockets]`: this process only starts the N ranks (itself, once per GPU) and waits for them.
// rccl (default): rank r runs on device r, the ranks meet in ncclCommInitRank over the id made here.  sockets: the engine's node-local transport over one
// socket pair per pair of ranks (psgsdf_comm_init_sockets) -- a node without a working RCCL, or ranks that share a device: VOXELPS_SHARE_GPU=1 puts
// all of them on device 0, VOXELPS_CU_MASKS="0:128,128:256" confines rank r to the r-th CU range (the one-GPU rehearsal, tests/test_voxelps_ranks_gpu.py).
// A rank that fails ends the run: the others are terminated (exactly the processes started here) and its exit code is returned.
static int launch_ranks(int n, bool sockets, int argc, char* argv[]) {
    if (n < 2 || n > 32) { std::cerr << "--gpus " << n << ": 2 .. 32 ranks" << std::endl; return 1; }
    std::vector<std::vector<int>> mesh(n, std::vector<int>(n, -1));
    std::string id_hex;
    if (sockets) {
        for (int r = 0; r < n; ++r) for (int q = r + 1; q < n; ++q) { int sv[2]; if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv)) { perror("socketpair"); return 1; } mesh[r][q] = sv[0]; mesh[q][r] = sv[1]; }
    } else {
        uint8_t id[128];
        if (psgsdf_comm_unique_id(id)) { std::cerr << "no RCCL on this node (psgsdf_comm_unique_id failed): --transport sockets runs without it" << std::endl; return 1; }
        static const char* hx = "0123456789abcdef";
        for (int i = 0; i < 128; ++i) { id_hex.push_back(hx[id[i] >> 4]); id_hex.push_back(hx[id[i] & 15]); }
    }
    std::vector<std::string> masks;
    if (const char* e = getenv("VOXELPS_CU_MASKS")) { std::string m = e; size_t a = 0; while (a <= m.size()) { size_t b = m.find(',', a); if (b == std::string::npos) b = m.size(); masks.push_back(m.substr(a, b - a)); a = b + 1; } }
    std::vector<pid_t> pids;
    for (int r = 0; r < n; ++r) {
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); for (pid_t p : pids) kill(p, SIGTERM); return 1; }
        if (pid == 0) {
            prctl(PR_SET_PDEATHSIG, SIGTERM);      // a launcher that is killed takes its ranks with it
            for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) if (a != r && mesh[a][b] >= 0) close(mesh[a][b]);      // the other ranks' ends
            if ((int)masks.size() == n) setenv("PSGSDF_CU_MASK", masks[r].c_str(), 1);
            setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
            std::vector<std::string> av(argv, argv + argc);
            av.push_back("--rank"); av.push_back(std::to_string(r)); av.push_back("--nranks"); av.push_back(std::to_string(n));
            if (sockets) { std::string f; for (int q = 0; q < n; ++q) f += (q ? "," : "") + std::to_string(mesh[r][q]); av.push_back("--fds"); av.push_back(f); }
            else { av.push_back("--comm-id"); av.push_back(id_hex); }
            std::vector<char*> cv; for (auto& a : av) cv.push_back(const_cast<char*>(a.c_str())); cv.push_back(nullptr);
            execv("/proc/self/exe", cv.data());
            perror("execv"); _exit(127);
        }
        pids.push_back(pid);
    }
    for (auto& row : mesh) for (int f : row) if (f >= 0) close(f);
    int rc = 0, left = n;
    while (left > 0) {
        int st = 0; const pid_t p = waitpid(-1, &st, 0);
        if (p < 0) break;
        auto it = std::find(pids.begin(), pids.end(), p); if (it == pids.end()) continue;
        --left; *it = -1;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        if (code != 0 && rc == 0) {
            rc = code;
            std::cerr << "rank " << (it - pids.begin()) << " ended with " << code << ": stopping the other ranks" << std::endl;
            for (pid_t q : pids) if (q > 0) kill(q, SIGTERM);
        }
    }
    return rc;
}

int main(int argc, char* argv[]) {
    if (argc >= 3 && std::string(argv[1]) == "--selftest-fmt") return selftest_fmt(atol(argv[2]));
    if (argc >= 3 && std::string(argv[1]) == "--selftest-lapm") return selftest_lapm(argv[2]);
    if (argc >= 4 && std::string(argv[1]) == "--selftest-sample") return selftest_sample(atoi(argv[2]), atoi(argv[3]));
    if (argc >= 3 && std::string(argv[1]) == "--selftest-png") return selftest_png(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-png-write") return selftest_png_write(argv[2]);
    if (argc >= 2 && std::string(argv[1]) == "--selftest-mc") return selftest_mc();
    if (argc >= 2 && std::string(argv[1]) == "--selftest-mc-table") return selftest_mc_table(false);
    if (argc >= 2 && std::string(argv[1]) == "--selftest-mc-generated") return selftest_mc_table(true);
    if (argc >= 4 && std::string(argv[1]) == "--selftest-mc-ply") return selftest_mc_ply(atoi(argv[2]), argv[3]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-ply-indexed") return selftest_ply_indexed(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-ply-fit") return selftest_ply_fit(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-ply-curvature") return selftest_ply_curvature(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-ply-filled") return selftest_ply_filled(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-obj-bake") return selftest_obj_bake(argv[2]);
    if (argc >= 3 && std::string(argv[1]) == "--selftest-ply-compare") return selftest_ply_compare(argv[2]);
    int want_ranks = 1; std::string transport = "rccl";
    std::string configfile, timing_file;      // --timing <file.json>: wall-clock per stage (no reference counterpart; the reference's outputs are unchanged)
    std::string filter_flag;                  // the last of --mesh-min-faces / --mesh-keep-largest given
    bool lod_flag = false, lod_ok = true;     // --mesh-lod S given / S is a number > 0
    bool bake_flag = false, bake_ok = true;   // --mesh-bake R given / R is a whole number >= 1
    bool ao_flag = false, ao_ok = true;       // --mesh-bake-ao K given / K is 8, 16, 32 or 64
    bool curv_flag = false, curv_ok = true;   // --mesh-bake-curvature S given / S is a finite number > 0
    bool fill_flag = false, fill_ok = true, fillk_flag = false, fillk_ok = true;   // --mesh-fill R given / R is a whole number in 0 .. 255; --mesh-fill-sweeps K given / K is a whole number in 0 .. 4096
    std::string cmp_file, cmp_bad;            // --compare-ply FILE given / the --compare-* flag whose number is bad
    bool cmp_tau_flag = false, cmp_max_flag = false, cmp_iters_flag = false, cmp_bad_iters = false;
    std::string query_file, query_model = "trilinear"; bool query_model_flag = false;   // --query-ply FILE given / --query-model M given
    std::string relight_file;                 // --relight FILE: every keyframe under the lights of FILE (relight/*.png, relight_report.txt; include/psgsdf_relight.h)
    bool render_keyframes = false;            // --render-keyframes: re-render every keyframe from the final state (render/*.png, render_report.txt)
    DumpOptions& opt = dump_options();      // (every dump flag is documented at its member, device_dumps.hpp)
    for (int i = 1; i < argc; ++i) { std::string a = argv[i]; if (a == "--config_file" && i + 1 < argc) configfile = argv[++i]; else if (a.rfind("--config_file=", 0) == 0) configfile = a.substr(14);
        else if (a == "--timing" && i + 1 < argc) timing_file = argv[++i];
        else if (a == "--host-writers") opt.host_writers = true;
        else if (a == "--render-keyframes") render_keyframes = true;
        else if (a == "--relight" && i + 1 < argc) relight_file = argv[++i];
        else if (a == "--indexed-mesh") opt.indexed_mesh = true;
        else if (a == "--mesh-min-faces" && i + 1 < argc) { opt.mesh_filter.min_faces = atoll(argv[++i]); opt.clean_mesh = true; filter_flag = a; }
        else if (a == "--mesh-keep-largest" && i + 1 < argc) { opt.mesh_filter.keep_largest = atoi(argv[++i]); opt.clean_mesh = true; filter_flag = a; }
        else if (a == "--mesh-lod" && i + 1 < argc) { char* end = nullptr; const double v = strtod(argv[++i], &end); lod_ok = end != argv[i] && *end == 0 && std::isfinite(v) && v > 0; opt.lod_voxels = lod_ok ? v : 0.0; lod_flag = true; }
        else if (a == "--mesh-bake" && i + 1 < argc) { char* end = nullptr; const long v = strtol(argv[++i], &end, 10); bake_ok = end != argv[i] && *end == 0 && v >= 1 && v <= 16383; opt.bake_res = bake_ok ? (int)v : 0; bake_flag = true; }
        else if (a == "--mesh-bake-ao" && i + 1 < argc) { char* end = nullptr; const long v = strtol(argv[++i], &end, 10); ao_ok = end != argv[i] && *end == 0 && (v == 8 || v == 16 || v == 32 || v == 64); opt.bake_ao_dirs = ao_ok ? (int)v : 0; ao_flag = true; }
        else if (a == "--mesh-bake-photo") opt.bake_photo = true;
        else if (a == "--mesh-fit") opt.fit = true;
        else if (a == "--mesh-curvature") opt.curvature = true;
        else if (a == "--mesh-bake-curvature" && i + 1 < argc) { char* end = nullptr; const double v = strtod(argv[++i], &end); curv_ok = end != argv[i] && *end == 0 && std::isfinite(v) && v > 0; opt.bake_curvature_scale = curv_ok ? v : 0.0; curv_flag = true; }
        else if (a == "--mesh-fill" && i + 1 < argc) { char* end = nullptr; const long v = strtol(argv[++i], &end, 10); fill_ok = end != argv[i] && *end == 0 && v >= 0 && v <= PSGSDF_FILL_MAX_ROUNDS; opt.fill_rounds = fill_ok ? (int)v : -1; fill_flag = true; }
        else if (a == "--mesh-fill-sweeps" && i + 1 < argc) { char* end = nullptr; const long v = strtol(argv[++i], &end, 10); fillk_ok = end != argv[i] && *end == 0 && v >= 0 && v <= PSGSDF_FILL_MAX_SWEEPS; if (fillk_ok) opt.fill_sweeps = (int)v; fillk_flag = true; }
        else if (a == "--compare-ply" && i + 1 < argc) cmp_file = argv[++i];
        else if ((a == "--compare-tau" || a == "--compare-max") && i + 1 < argc) {
            char* end = nullptr; const double v = strtod(argv[++i], &end);
            if (end == argv[i] || *end || !std::isfinite(v) || !(v > 0) || v > 64) cmp_bad = a;
            (a == "--compare-tau" ? opt.compare.tau_voxels : opt.compare.max_voxels) = v; (a == "--compare-tau" ? cmp_tau_flag : cmp_max_flag) = true; }
        else if (a == "--query-ply" && i + 1 < argc) query_file = argv[++i];
        else if (a == "--query-model" && i + 1 < argc) { query_model = argv[++i]; query_model_flag = true; }
        else if (a == "--query-project") opt.query.project = true;
        else if (a == "--compare-align") opt.compare.align = true;
        else if (a == "--compare-align-iters" && i + 1 < argc) { char* end = nullptr; const long v = strtol(argv[++i], &end, 10); if (end == argv[i] || *end || v < 0 || v > 64) cmp_bad_iters = true; opt.compare.align_iters = (int)v; cmp_iters_flag = true; }
        else if (a == "--frame-solver" && i + 1 < argc) { setenv("PSGSDF_FRAME_SOLVE", argv[++i], 1); std::cout << "frame solver: " << argv[i] << std::endl; }      // eigen = the reference's own solver of the light / pose blocks (include/psgsdf.h psgsdf_set_frame_solver); default ldlt.  The ranks of --gpus N inherit the environment.
        else if (a == "--gpus" && i + 1 < argc) want_ranks = atoi(argv[++i]);
        else if (a == "--transport" && i + 1 < argc) transport = argv[++i];
        else if (a == "--rank" && i + 1 < argc) rank_info().rank = atoi(argv[++i]);
        else if (a == "--nranks" && i + 1 < argc) rank_info().n = atoi(argv[++i]);
        else if (a == "--fds" && i + 1 < argc) { std::string f = argv[++i]; size_t p0 = 0; while (p0 <= f.size()) { size_t p1 = f.find(',', p0); if (p1 == std::string::npos) p1 = f.size(); rank_info().fds.push_back(atoi(f.substr(p0, p1 - p0).c_str())); p0 = p1 + 1; } }
        else if (a == "--comm-id" && i + 1 < argc) { std::string h = argv[++i]; for (size_t q = 0; q + 1 < h.size(); q += 2) rank_info().id.push_back((uint8_t)strtol(h.substr(q, 2).c_str(), nullptr, 16)); } }
    if (transport != "rccl" && transport != "sockets") { std::cerr << "--transport: rccl or sockets" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && opt.host_writers) { std::cerr << "--host-writers is the single-process cross-check" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && opt.clean_mesh) { std::cerr << filter_flag << " needs a single process: mesh components are not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << " yet" << std::endl; return 1; }
    if (ao_flag && !ao_ok) { std::cerr << "--mesh-bake-ao: rays per texel, 8, 16, 32 or 64" << std::endl; return 1; }
    if (ao_flag && !bake_flag) { std::cerr << "--mesh-bake-ao needs --mesh-bake R: the occlusion is one more map of the bake" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && ao_flag) { std::cerr << "--mesh-bake-ao needs a single process: the level-of-detail mesh it bakes onto is not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if (opt.bake_photo && !bake_flag) { std::cerr << "--mesh-bake-photo needs --mesh-bake R: the photo map is one more map of the bake" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && opt.bake_photo) { std::cerr << "--mesh-bake-photo needs a single process: the level-of-detail mesh it bakes onto is not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if (curv_flag && !curv_ok) { std::cerr << "--mesh-bake-curvature: the mean curvature times the voxel size that maps to white, a finite number > 0" << std::endl; return 1; }
    if (curv_flag && !bake_flag) { std::cerr << "--mesh-bake-curvature needs --mesh-bake R: the curvature is one more map of the bake" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && curv_flag) { std::cerr << "--mesh-bake-curvature needs a single process: the level-of-detail mesh it bakes onto is not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && opt.curvature) { std::cerr << "--mesh-curvature needs a single process: a slab holds only its own planes of the volume (--gpus " << std::max(want_ranks, rank_info().n) << ")" << std::endl; return 1; }
    if (fill_flag && !fill_ok) { std::cerr << "--mesh-fill: the front rounds, a whole number in 0 .. " << PSGSDF_FILL_MAX_ROUNDS << std::endl; return 1; }
    if (fillk_flag && !fillk_ok) { std::cerr << "--mesh-fill-sweeps: the relaxation sweeps, a whole number in 0 .. " << PSGSDF_FILL_MAX_SWEEPS << std::endl; return 1; }
    if (fillk_flag && !fill_flag) { std::cerr << "--mesh-fill-sweeps needs --mesh-fill R: the sweeps relax the voxels it fills" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && fill_flag) { std::cerr << "--mesh-fill needs a single process: a slab holds only its own planes of the volume (--gpus " << std::max(want_ranks, rank_info().n) << ")" << std::endl; return 1; }
    if (bake_flag && !bake_ok) { std::cerr << "--mesh-bake: texels along a triangle's edge, a whole number >= 1" << std::endl; return 1; }
    if (bake_flag && !lod_flag) { std::cerr << "--mesh-bake needs --mesh-lod S: the maps are baked onto the level-of-detail mesh" << std::endl; return 1; }
    if (lod_flag && !lod_ok) { std::cerr << "--mesh-lod: a cell size > 0, in voxels" << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && bake_flag) { std::cerr << "--mesh-bake needs a single process: the level-of-detail mesh it bakes onto is not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && lod_flag) { std::cerr << "--mesh-lod needs a single process: clusters are not merged across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if ((want_ranks > 1 || multi_rank()) && opt.fit) { std::cerr << "--mesh-fit needs a single process: the fit is not gathered across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if (!cmp_bad.empty()) { std::cerr << cmp_bad << ": a number of voxels, 0 < tau <= max <= 64" << std::endl; return 1; }
    if ((cmp_tau_flag || cmp_max_flag) && cmp_file.empty()) { std::cerr << "--compare-tau / --compare-max need --compare-ply FILE: the reference to compare with" << std::endl; return 1; }
    if (cmp_bad_iters) { std::cerr << "--compare-align-iters: a whole number of steps, 0 .. 64" << std::endl; return 1; }
    if (cmp_iters_flag && !opt.compare.align) { std::cerr << "--compare-align-iters needs --compare-align" << std::endl; return 1; }
    if (opt.compare.align && cmp_file.empty()) { std::cerr << "--compare-align needs --compare-ply FILE: the reference to align" << std::endl; return 1; }
    if (opt.compare.align && (want_ranks > 1 || multi_rank())) { std::cerr << "--compare-align needs a single process: the welded mesh is not gathered across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
    if (!cmp_file.empty()) {
        if (want_ranks > 1 || multi_rank()) { std::cerr << "--compare-ply needs a single process: the welded mesh is not gathered across the slabs of --gpus " << std::max(want_ranks, rank_info().n) << std::endl; return 1; }
        if (opt.compare.tau_voxels > opt.compare.max_voxels) { std::cerr << (cmp_tau_flag ? "--compare-tau" : "--compare-max") << ": tau " << opt.compare.tau_voxels << " is more than the matching radius " << opt.compare.max_voxels << std::endl; return 1; }
        std::string why;
        if (!read_reference_ply(cmp_file, opt.compare.xyz, opt.compare.faces, why)) { std::cerr << "--compare-ply: " << why << std::endl; return 1; }
        opt.compare.file = cmp_file; opt.compare.on = true;
    }
    if (query_model_flag && query_file.empty()) { std::cerr << "--query-model needs --query-ply FILE: the points to ask the field at" << std::endl; return 1; }
    if (opt.query.project && query_file.empty()) { std::cerr << "--query-project needs --query-ply FILE: the points to project" << std::endl; return 1; }
    if (!query_file.empty()) {
        if (query_model != "cell" && query_model != "trilinear") { std::cerr << "--query-model: cell or trilinear, not " << query_model << std::endl; return 1; }
        if (want_ranks > 1 || multi_rank()) { std::cerr << "--query-ply needs a single process: a slab holds only its own planes of the volume (--gpus " << std::max(want_ranks, rank_info().n) << ")" << std::endl; return 1; }
        std::string why; std::vector<int32_t> faces_unused;
        if (!read_reference_ply(query_file, opt.query.xyz, faces_unused, why)) { std::cerr << "--query-ply: " << why << std::endl; return 1; }
        opt.query.file = query_file; opt.query.model = query_model == "cell" ? PSGSDF_Q_CELL : PSGSDF_Q_TRILINEAR; opt.query.on = true;
    }
    if (!relight_file.empty()) {
        if (want_ranks > 1 || multi_rank()) { std::cerr << "--relight needs a single process: a slab holds only its own planes of the volume the shadow rays cross (--gpus " << std::max(want_ranks, rank_info().n) << ")" << std::endl; return 1; }
        std::string why;
        if (!read_relight_file(relight_file, opt.relight, why)) { std::cerr << "--relight: " << why << std::endl; return 1; }
        opt.relight.on = true;
    }
    if (opt.mesh_filter.keep_largest < 0) { std::cerr << "--mesh-keep-largest: a count >= 0" << std::endl; return 1; }
    if (want_ranks > 1 && !multi_rank()) return launch_ranks(want_ranks, transport == "sockets", argc, argv);
    static std::ofstream null_out;
    if (multi_rank()) {
        RankInfo& ri = rank_info();
        ri.sockets = transport == "sockets";
        ri.device = getenv("VOXELPS_SHARE_GPU") && atoi(getenv("VOXELPS_SHARE_GPU")) ? 0 : ri.rank;
        if (ri.rank < 0 || ri.rank >= ri.n || (ri.sockets ? (int)ri.fds.size() != ri.n : ri.id.size() != 128)) { std::cerr << "--rank / --nranks / --fds / --comm-id are set by `voxelPS --gpus N`" << std::endl; return 1; }
        if (!lead_rank()) { null_out.open("/dev/null"); std::cout.rdbuf(null_out.rdbuf()); }      // rank 0 narrates
    }
    const auto t_main0 = std::chrono::steady_clock::now();
    std::cout << "load the config file from: " << configfile << std::endl;
    JsonObject config;
    if (!config.load(configfile)) { std::cout << "can't load config file!" << std::endl << "fail to load the config file!" << std::endl; return 1; }
    if (!config.contains("input") || !config.contains("output") || !config.contains("datatype")) {
        std::cout << "missing necessary input arguments (input/out folder/datatype) in config file!" << std::endl << "fail to load the config file!" << std::endl; return 1; }
    const std::string input = config.str("input"), output = config.str("output"), datatype = config.str("datatype");
    ImageLoader* loader;
    if (datatype == "tum") loader = new TumrgbdLoader(input);
    else if (datatype == "led" || datatype == "synth") loader = new SynthLoader(input);
    else if (datatype == "intrinsic3d" || datatype == "multiview") loader = new MultiviewLoader(input);
    else { std::cerr << "Your specified dataset type is not supported (yet)." << std::endl; return 1; }
    // TrackingSettings.h:26-38 defaults
    std::string pose_file = "pose.txt"; size_t first = 0, last = (size_t)-1; float voxel_size = 0.02f, truncation_factor = 5, zmin = 0.5f, zmax = 3.5f, sharp_thr = 0.5f;
    if (config.contains("pose filename")) pose_file = config.str("pose filename");
    if (config.contains("first")) first = (size_t)config.num("first");
    if (config.contains("last")) last = (size_t)config.num("last");
    if (config.contains("voxel size")) voxel_size = (float)config.num("voxel size");
    if (config.contains("truncation factor")) truncation_factor = (float)config.num("truncation factor");
    if (config.contains("sharpness threshold")) sharp_thr = (float)config.num("sharpness threshold");
    if (config.contains("zmin")) zmin = (float)config.num("zmin");
    if (config.contains("zmax")) zmax = (float)config.num("zmax");
    OptimizerSettings* opt_set_ = new OptimizerSettings();
    if (config.contains("model type")) {
        std::string m = config.str("model type");
        if (m == "SH1") { opt_set_->model = SH1; opt_set_->order = 1; } else if (m == "SH2") { opt_set_->model = SH2; opt_set_->order = 2; } else if (m == "LED") opt_set_->model = LED;
        else { std::cerr << "Your specified model type is not supported (yet)." << std::endl; return 1; }
    }
    if (config.contains("loss function")) {
        std::string l = config.str("loss function");
        if (l == "cauchy") opt_set_->loss = CAUCHY; else if (l == "l2") opt_set_->loss = L2; else if (l == "huber") opt_set_->loss = HUBER;
        else if (l == "trunc_l2") opt_set_->loss = TRUNC_L2;   // the reference leaves the loss uninitialised here (ConfigLoader.h:126, B7); we honour the key
        else if (l == "tukey") opt_set_->loss = TUKEY;
        else { std::cerr << "Your specified loss function type is not supported (yet)." << std::endl; return 1; }
    }
    if (config.contains("reg albedo")) opt_set_->reg_weight_rho = (float)config.num("reg albedo");
    if (config.contains("reg norm")) opt_set_->reg_weight_n = (float)config.num("reg norm");
    if (config.contains("reg laplacian")) opt_set_->reg_weight_l = (float)config.num("reg laplacian");
    if (config.contains("max iter")) opt_set_->max_it = (int)config.num("max iter");
    if (config.contains("damping")) opt_set_->damping = (float)config.num("damping");
    if (config.contains("converge threshold")) opt_set_->conv_threshold = (float)config.num("converge threshold");
    if (config.contains("upsample")) opt_set_->upsample = config.boolean("upsample");
    if (config.contains("lambda")) { opt_set_->lambda = (float)config.num("lambda"); opt_set_->lambda_sq = opt_set_->lambda * opt_set_->lambda; }
    if (lead_rank()) { std::ofstream save_conf(output + "saved_config.json"); if (!save_conf.is_open()) std::cout << "could not save config file." << std::endl; config.dump(save_conf); }
    bool light = false, albedo = false, distance = false, pose = false;
    if (config.contains("--light")) light = config.boolean("--light");
    if (config.contains("--albedo")) albedo = config.boolean("--albedo");
    if (config.contains("--distance")) distance = config.boolean("--distance");
    if (config.contains("--pose")) pose = config.boolean("--pose");
    const int grid = config.contains("grid dim") ? (int)config.num("grid dim") : 128;
    const int max_key = config.contains("max keyframes") ? (int)config.num("max keyframes") : 40;
    const float truncation = truncation_factor * voxel_size;

    if (!loader->load_intrinsics("intrinsics.txt")) { std::cerr << "No intrinsics file found in " << input << "!" << std::endl; return 1; }
    const Mat3f K = loader->K();
    ImageRGB color; DepthImage depth;
    if (!loader->load_next(color, depth)) { std::cerr << " -> Frame could not be loaded!" << std::endl; return 1; }
    if (color.rows != depth.rows || color.cols != depth.cols) { std::cerr << "-> depth image and color image sizes don't match." << std::endl; return 1; }
    loader->reset_counter();

    int grid_dim[3] = {grid, grid, grid};
    VolumetricGradSdf* tSDF = new VolumetricGradSdf();
    RigidPointOptimizer* pOpt = nullptr; Optimizer* vOpt = nullptr;
    std::ofstream pose_out; if (lead_rank()) pose_out.open(output + "tracking_poses.txt");
    std::vector<Mat4f> poses; std::vector<int> keyframes{0}; std::vector<std::string> key_stamps; std::vector<std::shared_ptr<ImageRGB>> key_images;
    const Mat4f I4 = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<Mat4f> key_poses{I4};   // key_poses[0] is Identity even with GT poses (main_ps.cpp:139, B1)
    int dist_to_last_keyframe = 0; bool GT_pose = false;
    if (!loader->load_pose(pose_file, poses)) { std::cout << "GT poses is not avalible!" << std::endl; poses.push_back(I4); }
    else { std::cout << poses.size() << " GT poses are loaded." << std::endl; GT_pose = true; }
    { std::string d, r; for (size_t i = 0; i < first; ++i) if (opt.host_writers) loader->load_next(color, depth); else loader->next_names(d, r); }      // (frames in front of "first" are skipped; the reference decodes them, nothing reads them)
    Mat4f cur_pose = I4;
    size_t window = opt.host_writers ? 1 : std::min<size_t>(4, std::max(2u, std::thread::hardware_concurrency() / 2));
    if (const char* e = getenv("VOXELPS_PREFETCH")) window = (size_t)std::max(1, atoi(e));      // (frames decoded ahead of the fusion)
    FramePrefetcher prefetch(loader, window);
    std::string stamp_rgb, stamp_depth;
    for (size_t i = first; i <= last; ++i) {
        std::cout << "Working on frame: " << i << std::endl;
        {
            PSG_STAGE("decode: PNG colour + depth (host; wait for the prefetched frame)");
            if (opt.host_writers) { if (!loader->load_next(color, depth)) { std::cerr << " -> Frame " << i << " could not be loaded!" << std::endl; break; } stamp_rgb = loader->rgb_timestamp(); stamp_depth = loader->depth_timestamp(); }
            else {
                auto fr = prefetch.next();
                if (!fr) { std::cerr << " -> Frame " << i << " could not be loaded!" << std::endl; break; }
                color = std::move(fr->color); depth = std::move(fr->depth); stamp_rgb = fr->rgb_stamp; stamp_depth = fr->depth_stamp;
            }
        }
        if (GT_pose && i >= poses.size()) break;
        if (i == first) {
            float centroid[3]; compute_centroid(K, depth, poses[0], centroid);
            psgsdf_settings s{};
            s.model = opt_set_->model == LED ? PSGSDF_LED : (opt_set_->model == SH2 ? PSGSDF_SH2 : PSGSDF_SH1); s.loss = (int)opt_set_->loss; s.lambda = opt_set_->lambda; s.damping = opt_set_->damping;
            s.reg_weight_rho = opt_set_->reg_weight_rho; s.reg_weight_n = opt_set_->reg_weight_n; s.reg_weight_l = opt_set_->reg_weight_l; s.max_it = opt_set_->max_it;
            s.conv_threshold = opt_set_->conv_threshold; s.upsample = opt_set_->upsample ? 1 : 0; s.ref_quirks = 1;
            // frames to expect: the config's range when it has a "last", else unknown (the reference runs until the loader is exhausted,
            // main_ps.cpp:222-258) -- the device volume widens its per-voxel visibility words when the sequence outgrows this
            const int max_frames = last == (size_t)-1 ? 256 : (int)std::min<size_t>(last - first + 1, (size_t)1 << 20);
            if (!tSDF->attach(grid_dim, voxel_size, centroid, truncation, K, s, max_frames)) { std::cerr << "could not create the device volume" << std::endl; return 1; }
            tSDF->set_zmin(zmin); tSDF->set_zmax(zmax);
            pOpt = new RigidPointOptimizer(tSDF);
            if (opt_set_->model == LED) vOpt = new LedOptimizer(tSDF, voxel_size, K, output, opt_set_); else vOpt = new PsOptimizer(tSDF, voxel_size, K, output, opt_set_);
            if (!tSDF->update(color, depth.data, poses[0])) { std::cerr << " -> Frame " << i << " could not be fused: " << tSDF->last_error() << std::endl; return 1; }
            cur_pose = poses[0];
            key_stamps.push_back(stamp_rgb);
            key_images.push_back(std::make_shared<ImageRGB>(color));
        } else {
            tSDF->increase_counter();
            bool integrated = false;
            if (GT_pose) { cur_pose = poses[i]; integrated = tSDF->update(color, depth.data, poses[i]); }
            else { bool conv = pOpt->optimize(depth.data, depth.cols, depth.rows); cur_pose = pOpt->pose(); if (conv) integrated = tSDF->update(color, depth.data, cur_pose); }
            if (!integrated && tSDF->last_error()[0]) { std::cerr << " -> Frame " << i << " could not be fused: " << tSDF->last_error() << std::endl; return 1; }   // a frame that is not in the volume must not become a keyframe
            if (integrated) {
                bool sharp; { PSG_STAGE("keyframe selection: focus measure (host)"); sharp = sharpDetector(color, sharp_thr); }
                if (sharp || dist_to_last_keyframe > 5) {
                    dist_to_last_keyframe = 0;
                    keyframes.push_back((int)(i - first)); key_stamps.push_back(stamp_rgb); key_poses.push_back(cur_pose);
                    key_images.push_back(std::make_shared<ImageRGB>(color));
                } else ++dist_to_last_keyframe;
            }
        }
        float q[4]; quat_of(cur_pose.data(), q);
        pose_out << stamp_depth << " " << cur_pose[3] << " " << cur_pose[7] << " " << cur_pose[11] << " " << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << "\n";
    }
    pose_out.close();
    if (!vOpt) { std::cerr << "no frame was processed" << std::endl; return 1; }
    if (!tSDF->extract_mesh(output + "init_mesh.ply")) std::cerr << "Could not save mesh to " << output + "init_mesh.ply" << "!" << std::endl;
    if (!tSDF->extract_pc(output + "init_pointcloud.ply")) std::cerr << "Could not save point cloud to " << output + "init_pointcloud.ply" << "!" << std::endl;
    if (!tSDF->saveSDF(output + "init_sdf.sdf")) std::cerr << "Could not save sdf to " << output + "init_sdf.sdf" << "!" << std::endl;
    std::cout << " selected key frame: " << std::endl; for (int k : keyframes) std::cout << k << " "; std::cout << std::endl;
    if ((int)keyframes.size() > max_key) sampleKeyFrame(keyframes, key_stamps, key_images, key_poses, max_key);
    std::cout << " selected key frame after sampling: " << std::endl; for (int k : keyframes) std::cout << k << " "; std::cout << std::endl;
    opt.skip_sync_back = !opt.host_writers;
    vOpt->setImages(key_images); vOpt->setKeyframes(keyframes); vOpt->setKeytimestamps(key_stamps); vOpt->setPoses(key_poses);
    vOpt->init();
    vOpt->alternatingOptimize(light, albedo, distance, pose);
    if (render_keyframes && !vOpt->renderKeyframes(output)) { std::cerr << "--render-keyframes: rendering failed" << std::endl; return 1; }   // (collective on a multi-rank run)
    if (opt.relight.on && !vOpt->relightKeyframes(output, opt.relight)) { std::cerr << "--relight: relighting failed" << std::endl; return 1; }
    DumpQueue::get().drain();
    const int write_failures = DumpQueue::get().failures();      // (a rank whose piece of a shared output file could not be written: the file has a hole where it belongs)
    if (write_failures) std::cerr << "rank " << rank_info().rank << ": " << write_failures << " output file piece(s) could not be written" << std::endl;
    delete vOpt; delete pOpt; delete tSDF; delete loader; delete opt_set_;
    if (!timing_file.empty() && lead_rank()) {
        char extra[256];
        snprintf(extra, sizeof(extra), ", \"total_s\": %.6f, \"frames\": %zu, \"keyframes\": %zu", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main0).count(),
                 (size_t)(last == (size_t)-1 ? 0 : last - first + 1), keyframes.size());
        StageClock::get().write_json(timing_file, extra);
    }
    return write_failures ? 1 : 0;
}
