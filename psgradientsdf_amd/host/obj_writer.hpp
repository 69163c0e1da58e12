// obj_writer.hpp -- the textured mesh of `voxelPS --mesh-bake R` (include/psgsdf_bake.h): a Wavefront OBJ with positions, vertex normals and one
// texture coordinate per face corner, its material file, and the object-space normal map's bytes.  Floats are written with %.9g: a float32 reads
// back as the same float32.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "text_format.hpp"

namespace psgsdf_host {

inline std::string path_basename(const std::string& p) { const size_t s = p.find_last_of('/'); return s == std::string::npos ? p : p.substr(s + 1); }

// a unit normal's component as a byte of an object-space normal map: floor(127.5 (n + 1) + 0.5), clamped to [0, 255]
inline uint8_t normal_to_u8(float n) {
    const float v = std::floor(127.5f * (n + 1.0f) + 0.5f);
    return (uint8_t)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);      // (NaN -> 0)
}

// xyz, nrm: [nv][3]; faces: [nf][3] (0-based); uv: [nf][3][2] with v pointing DOWN (row 0 of the image on top): OBJ's v points up, so 1 - v is written.
// ao_png (if given): one more line `map_Ka <file>` in the material.
// `f a/t/n`: position and normal share the vertex number, the texture coordinate of corner k of face f is number 3 f + k (all 1-based in the file)
inline bool write_obj_bake(const std::string& obj_path, const std::string& mtl_path, const std::string& albedo_png, const std::string& normal_png,
                           const float* xyz, const float* nrm, size_t nv, const int32_t* faces, const float* uv, size_t nf, const std::string& ao_png = "") {
    std::string s;
    s.reserve(64 * nv + 120 * nf + 256);
    char line[256];
    s += "# baked level-of-detail mesh: " + std::to_string(nv) + " vertices, " + std::to_string(nf) + " faces\n";
    s += "mtllib " + path_basename(mtl_path) + "\n";
    for (size_t v = 0; v < nv; ++v) { snprintf(line, sizeof line, "v %.9g %.9g %.9g\n", xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]); s += line; }
    for (size_t v = 0; v < nv; ++v) { snprintf(line, sizeof line, "vn %.9g %.9g %.9g\n", nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]); s += line; }
    for (size_t q = 0; q < 3 * nf; ++q) { snprintf(line, sizeof line, "vt %.9g %.9g\n", uv[2 * q], 1.0f - uv[2 * q + 1]); s += line; }
    s += "usemtl baked\n";
    for (size_t f = 0; f < nf; ++f) {
        const long long a = faces[3 * f] + 1ll, b = faces[3 * f + 1] + 1ll, c = faces[3 * f + 2] + 1ll, t = 3ll * (long long)f + 1;
        snprintf(line, sizeof line, "f %lld/%lld/%lld %lld/%lld/%lld %lld/%lld/%lld\n", a, t, a, b, t + 1, b, c, t + 2, c);
        s += line;
    }
    const bool ok = save_text(obj_path, s);
    const std::string m = "newmtl baked\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nmap_Kd " + path_basename(albedo_png) + "\nnorm " + path_basename(normal_png) + "\n"
                          + (ao_png.empty() ? "" : "map_Ka " + path_basename(ao_png) + "\n");      // (--mesh-bake-ao: the ambient-occlusion map)
    return save_text(mtl_path, m) && ok;
}

}  // namespace psgsdf_host
