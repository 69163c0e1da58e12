// ply_io.hpp — the dump files' formats: the reference's ASCII mesh / point cloud / SDF files (threaded, text_format.hpp), the binary PLY of the
// welded mesh with any number of further vertex columns, and the reader of `--compare-ply`.  No engine call and no queue in here: arrays in, a file out.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "text_format.hpp"

namespace psgsdf_host {

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
    return OutFile(file).put(mesh_header(nv)).lines(nv, 40, [&](TextOut& o, size_t i) { mesh_vertex_line(o, xyz, rgb, i); })
                        .lines(nv / 3, 24, [&](TextOut& o, size_t q) { mesh_face_line(o, q); }).close();
}
// save_pointcloud / extract_pc (OptimizerAux.cpp:456-511, VolumetricGradSdf.cpp:320-376): x y z nx ny nz r g b
inline bool write_pointcloud_ply(const std::string& file, const float* pn, const int32_t* col, size_t n) {
    return OutFile(file).put(pointcloud_header(n)).lines(n, 80, [&](TextOut& o, size_t i) { pointcloud_line(o, pn, col, i); }).close();
}
// saveSDF (OptimizerAux.cpp:513-577): dims, the box's first voxel in metres, the voxel size, then -dist, x fastest
inline bool write_sdf_block(const std::string& file, const int lo[3], const int dim[3], float vs, const float* v) {
    return OutFile(file).put(sdf_header(lo, dim, vs)).lines((size_t)dim[0] * dim[1] * dim[2], 12, [&](TextOut& o, size_t i) { o.f(v[i]); o.c('\n'); }).close();
}

// ---- the welded mesh (include/psgsdf_mesh.h) as a binary little-endian PLY ---------------------------------------------------------------------------
// Vertex records x y z nx ny nz (float) red green blue (uchar), 27 B, then one value of every further column; face records a uchar 3 and three
// int vertex indices, 13 B.  Coordinates are grid-local like every other writer's: the first comment line holds the grid origin and the voxel size
// (world = origin + the position).  No reference counterpart: `voxelPS --indexed-mesh` and the dumps that attach something to its vertices.
constexpr size_t kPlyVertexBytes = 27, kPlyFaceBytes = 13;
struct MeshView { const float* xyz; const float* normals; const uint8_t* rgb; size_t nv; const int32_t* faces; size_t nf; };      // (borrowed arrays)
// one further vertex column behind the colours: `bytes` per vertex of PLY type `type`, vertex i's at data + i * bytes (the host is little-endian:
// the records are the arrays' bytes).  ply_column() takes type and width from the array it is given.
struct PlyColumn { const char* type; const char* name; const void* data; size_t bytes; };
inline PlyColumn ply_column(const char* name, const float* d) { return {"float", name, d, 4}; }
inline PlyColumn ply_column(const char* name, const int32_t* d) { return {"int", name, d, 4}; }
inline PlyColumn ply_column(const char* name, const uint8_t* d) { return {"uchar", name, d, 1}; }
inline PlyColumn ply_column(const char* name, const int8_t* d) { return {"char", name, d, 1}; }
inline std::string mesh_indexed_header(size_t nv, size_t nf, const float origin[3], float vs, const std::string& extra = std::string(),      // extra: further header lines (each ends in \n)
                                       const std::string& vertex_props = std::string()) {                                                     // vertex_props: further vertex property lines, behind the colours
    char c[160];
    snprintf(c, sizeof c, "comment grid origin %.9g %.9g %.9g voxel size %.9g\n", (double)origin[0], (double)origin[1], (double)origin[2], (double)vs);
    return std::string("ply\nformat binary_little_endian 1.0\n") + c + extra + "element vertex " + std::to_string(nv) + "\n"
           "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\n" + vertex_props +
           "element face " + std::to_string(nf) + "\nproperty list uchar int vertex_indices\nend_header\n";
}
inline std::string mesh_indexed_vertices(const float* xyz, const float* nrm, const uint8_t* rgb, size_t nv, const std::vector<PlyColumn>& columns = {}) {
    size_t rec = kPlyVertexBytes; for (const PlyColumn& c : columns) rec += c.bytes;
    std::string b(nv * rec, '\0'); char* p = &b[0];
    for (size_t i = 0; i < nv; ++i) {
        memcpy(p, xyz + 3 * i, 12); memcpy(p + 12, nrm + 3 * i, 12); memcpy(p + 24, rgb + 3 * i, 3); p += kPlyVertexBytes;
        for (const PlyColumn& c : columns) { memcpy(p, (const char*)c.data + i * c.bytes, c.bytes); p += c.bytes; }
    }
    return b;
}
inline std::string mesh_indexed_faces(const int32_t* faces, size_t nf) {
    std::string b(nf * kPlyFaceBytes, '\0'); char* p = &b[0];
    for (size_t q = 0; q < nf; ++q, p += kPlyFaceBytes) { p[0] = 3; memcpy(p + 1, faces + 3 * q, 12); }
    return b;
}
// the one writer: `comments` are further header lines (each ends in \n), the property lines and the record width follow from `columns`
inline bool write_mesh_indexed_ply(const std::string& file, const MeshView& m, const float origin[3], float vs, const std::string& comments = std::string(),
                                   const std::vector<PlyColumn>& columns = {}) {
    std::string props; for (const PlyColumn& c : columns) props += std::string("property ") + c.type + " " + c.name + "\n";
    return OutFile(file).put(mesh_indexed_header(m.nv, m.nf, origin, vs, comments, props)).put(mesh_indexed_vertices(m.xyz, m.normals, m.rgb, m.nv, columns)).put(mesh_indexed_faces(m.faces, m.nf)).close();
}
// What the dumps attach (the columns in file order) and the header line that goes with them:
//   `--mesh-fit` (include/psgsdf_fit.h): float quality (the rms residual), float loss (the mean robust loss), int n_obs; the line holds the overall rms
//     residual (the root of the n_obs-weighted mean of quality^2, in double from the columns as written) and the sum of n_obs
//   `--mesh-curvature` (include/psgsdf_curvature.h): float quality (the mean curvature), float gauss, float k1, float k2, uchar curvature_valid (valid end
//     voxels); the line holds the mean of quality over the vertices with curvature_valid > 0 (in double, from the column as written) and their number
//   `--mesh-fill` (include/psgsdf_fill.h): uchar filled (filled end voxels: 0, 1 or 2); the line holds the rounds, the sweeps, the voxels filled and the
//     boundary edges of the kept components without and with the filling
//   `--compare-ply` (include/psgsdf_compare.h): float distance (inf: no match within max_dist), char side (-1 inside, +1 outside, 0 on the reference, a
//     cloud, or no match); the line is the caller's
//   `--query-ply` (include/psgsdf_query.h; write_points_ply below, a cloud: no normals or colours of its own, no faces): float distance nx ny nz red
//     green blue weight and uchar status (the field at the points), or with --query-project float distance residual, uchar iterations status (the
//     projected points); the line names the model and holds the call's counts
// A cloud as a binary little-endian PLY: x y z (float) and one value of every column per vertex; the comment line of the welded mesh's writer first.
inline bool write_points_ply(const std::string& file, const float* xyz, size_t n, const float origin[3], float vs, const std::string& comments, const std::vector<PlyColumn>& columns) {
    char c[160];
    snprintf(c, sizeof c, "comment grid origin %.9g %.9g %.9g voxel size %.9g\n", (double)origin[0], (double)origin[1], (double)origin[2], (double)vs);
    std::string h = std::string("ply\nformat binary_little_endian 1.0\n") + c + comments + "element vertex " + std::to_string(n) + "\nproperty float x\nproperty float y\nproperty float z\n";
    size_t rec = 12;
    for (const PlyColumn& k : columns) { h += std::string("property ") + k.type + " " + k.name + "\n"; rec += k.bytes; }
    h += "end_header\n";
    std::string b(n * rec, '\0'); char* p = &b[0];
    for (size_t i = 0; i < n; ++i) {
        memcpy(p, xyz + 3 * i, 12); p += 12;
        for (const PlyColumn& k : columns) { memcpy(p, (const char*)k.data + i * k.bytes, k.bytes); p += k.bytes; }
    }
    return OutFile(file).put(h).put(b).close();
}
inline std::string mesh_fit_comment(const float* rms, const int32_t* n_obs, size_t nv) {
    double q = 0.0; long long n = 0;
    for (size_t i = 0; i < nv; ++i) { q += (double)n_obs[i] * ((double)rms[i] * (double)rms[i]); n += n_obs[i]; }
    char c[120];
    snprintf(c, sizeof c, "comment fit rms %.17g observations %lld\n", n ? std::sqrt(q / (double)n) : 0.0, n);
    return c;
}
inline std::string mesh_curvature_comment(const float* mean, const uint8_t* valid, size_t nv) {
    double q = 0.0; long long n = 0;
    for (size_t i = 0; i < nv; ++i) if (valid[i] > 0) { q += (double)mean[i]; n += 1; }
    char c[120];
    snprintf(c, sizeof c, "comment curvature mean %.17g valid %lld\n", n ? q / (double)n : 0.0, n);
    return c;
}
inline std::string mesh_filled_comment(int rounds, int sweeps, long long voxels, long long boundary_before, long long boundary_after) {
    char c[200];
    snprintf(c, sizeof c, "comment fill rounds %d sweeps %d voxels %lld boundary_edges %lld %lld\n", rounds, sweeps, voxels, boundary_before, boundary_after);
    return c;
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

}  // namespace psgsdf_host
