// png_writer.hpp -- 8-bit PNG encoding with zlib only (gray or RGB, filter type 0, one IDAT chunk): the images of `voxelPS --render-keyframes`.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace psgsdf_host {

// px: row-major, `channels` (1 or 3) interleaved bytes per pixel
inline bool write_png(const std::string& path, int width, int height, int channels, const uint8_t* px) {
    if (width <= 0 || height <= 0 || (channels != 1 && channels != 3)) return false;
    const size_t stride = (size_t)width * channels;
    std::vector<unsigned char> raw((stride + 1) * height);
    for (int y = 0; y < height; ++y) {
        raw[(stride + 1) * y] = 0;      // filter: none
        std::copy(px + stride * y, px + stride * (y + 1), raw.begin() + (stride + 1) * y + 1);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
    z.resize(zn);
    std::vector<unsigned char> out = {137, 80, 78, 71, 13, 10, 26, 10};
    auto put32 = [&](uint32_t v) { out.push_back(v >> 24); out.push_back((v >> 16) & 255); out.push_back((v >> 8) & 255); out.push_back(v & 255); };
    auto chunk = [&](const char* type, const std::vector<unsigned char>& data) {
        put32((uint32_t)data.size());
        const size_t at = out.size();
        out.insert(out.end(), type, type + 4);
        out.insert(out.end(), data.begin(), data.end());
        put32((uint32_t)crc32(0L, out.data() + at, (uInt)(out.size() - at)));
    };
    std::vector<unsigned char> ihdr;
    for (uint32_t v : {(uint32_t)width, (uint32_t)height}) for (int s = 24; s >= 0; s -= 8) ihdr.push_back((v >> s) & 255);
    ihdr.insert(ihdr.end(), {8, (unsigned char)(channels == 3 ? 2 : 0), 0, 0, 0});      // bit depth 8, colour type RGB / gray, deflate, filter 0, no interlace
    chunk("IHDR", ihdr);
    chunk("IDAT", z);
    chunk("IEND", {});
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    return (fclose(f) == 0) && ok;
}

// a float plane value as a byte: clamp to [0, 1], then round(255 v)
inline uint8_t unit_to_u8(float v) {
    v = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;      // (NaN -> 0)
    return (uint8_t)(v * 255.f + 0.5f);
}

}  // namespace psgsdf_host
