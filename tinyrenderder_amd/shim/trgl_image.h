// trgl_image.h — TGAColor / TGAImage with the reference's interface (tgaimage.h:29-104) and the
// byte-exact TGA file format of its writer (tgaimage.cpp:161-242): 18-byte header, no footer,
// imagedescriptor 0x00 when vflip (the default), RLE packets formed exactly as the reference forms
// them (its raw packets run up to AND INCLUDING the first pixel of the next repeated pair).
// The reader follows read_tga_file / load_rle_data (tgaimage.cpp:76-160).  Host-only; this is SURVEY.md §8(f) row N3.
// scale() and gaussian_blur() (tgaimage.cpp:246-324) are host loops over trgl_image::scale_bytes / blur_bytes below, the same functions
// the C ABI's TRGL_MEM_HOST paths run (trgl_image_scale, trgl_image_blur); compile with -ffp-contract=off, as everything that must
// match the reference's bytes.  shadow_mask_bytes / modulate_bytes are the host loops of the shadow post-pass (trgl_shadow_mask_image,
// trgl_image_modulate), which has no counterpart in the reference.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

namespace trgl_image {

// The weights of TGAImage::gaussian_blur (tgaimage.cpp:275-284) for radius >= 1, all in float: sigma = radius / 2, v[i] =
// exp(-(i * i) / (2 * sigma * sigma)) with the int -(i * i) converted, summed in index order from 0, each then divided by the sum.
// radius <= 46340, so that i * i fits an int.
inline void gaussian_weights(int radius, float* weights) {
    const float sigma = radius / 2.0f;
    float sum = 0;
    for (int i = -radius; i <= radius; ++i) {
        const float v = std::exp(float(-(i * i)) / (2 * sigma * sigma));
        weights[i + radius] = v;
        sum += v;
    }
    for (int k = 0; k <= 2 * radius; ++k) weights[k] /= sum;
}

// One pass of the separable blur (tgaimage.cpp:290-304 or :309-323) from `src` into `dst`, two images of w * h * bpp bytes that do not
// overlap: per byte a float sum from 0.0f over the taps k = -radius..radius in that order of byte(clamped neighbour) * weight - one
// rounded multiply and one rounded add per tap - stored truncated.  Neighbours lie along x (stride bpp, clamped to 0..w-1) or along y
// (stride w * bpp, clamped to 0..h-1); every channel is treated alike.  The sums of one row are kept side by side and the tap loop runs
// outside them: every sum still receives its own taps in the reference's order, and the inner loops are plain arrays for the compiler.
inline void blur_pass(const std::uint8_t* src, std::uint8_t* dst, int w, int h, int bpp, int radius, const float* weights, bool vertical) {
    const std::size_t row = std::size_t(w) * bpp;
    std::vector<float> accum(row);
    float* acc = accum.data();
    auto add = [acc](std::size_t b, std::uint8_t byte, float kv) { const float term = float(int(byte)) * kv; acc[b] = acc[b] + term; };
    for (int y = 0; y < h; ++y) {
        for (std::size_t b = 0; b < row; ++b) acc[b] = 0.0f;
        for (int k = -radius; k <= radius; ++k) {
            const float kv = weights[k + radius];
            if (vertical) {
                const int yy = y + k < 0 ? 0 : y + k > h - 1 ? h - 1 : y + k;
                const std::uint8_t* s = src + yy * row;
                for (std::size_t b = 0; b < row; ++b) add(b, s[b], kv);
            } else {
                const std::uint8_t* s = src + y * row;
                const int lo = k < 0 ? (-k < w ? -k : w) : 0, hi = k > 0 ? (w - k > 0 ? w - k : 0) : w;     // x in [lo, hi): x + k needs no clamp
                for (int x = 0; x < lo; ++x) for (int ch = 0; ch < bpp; ++ch) add(std::size_t(x) * bpp + ch, s[ch], kv);
                const std::ptrdiff_t shift = std::ptrdiff_t(k) * bpp;
                for (std::size_t b = std::size_t(lo) * bpp; b < std::size_t(hi > lo ? hi : lo) * bpp; ++b) add(b, s[std::ptrdiff_t(b) + shift], kv);
                for (int x = hi > lo ? hi : lo; x < w; ++x) for (int ch = 0; ch < bpp; ++ch) add(std::size_t(x) * bpp + ch, s[std::size_t(w - 1) * bpp + ch], kv);
            }
        }
        for (std::size_t b = 0; b < row; ++b) dst[y * row + b] = std::uint8_t(acc[b]);
    }
}
// TGAImage::gaussian_blur (tgaimage.cpp:286-323) in place on w * h * bpp bytes: the horizontal pass into `tmp` (as many bytes), the
// vertical pass back - so the vertical pass reads the horizontal pass's truncated bytes, as the reference's second copy does.
inline void blur_bytes(std::uint8_t* pixels, int w, int h, int bpp, int radius, const float* weights, std::uint8_t* tmp) {
    blur_pass(pixels, tmp, w, h, bpp, radius, weights, false);
    blur_pass(tmp, pixels, w, h, bpp, radius, weights, true);
}

// TGAImage::scale (tgaimage.cpp:251-261): dst(x, y) = src(x * w / w2, y * h / h2) in int arithmetic, bpp bytes per pixel.  The caller
// has checked that (w2 - 1) * w, (h2 - 1) * h and the byte counts fit an int.
inline void scale_bytes(const std::uint8_t* src, int w, int h, int bpp, std::uint8_t* dst, int w2, int h2) {
    for (int y = 0; y < h2; ++y) {
        const std::uint8_t* srow = src + std::size_t(y * h / h2) * w * bpp;
        std::uint8_t* drow = dst + std::size_t(y) * w2 * bpp;
        for (int x = 0; x < w2; ++x) std::memcpy(drow + std::size_t(x) * bpp, srow + std::size_t(x * w / w2) * bpp, bpp);
    }
}

// The shadow post-pass of trgl_shadow_mask_image (include/trgl.h, steps 1-8 there): one byte per camera pixel from its depth, the row-major
// M that carries the pixel centre (x + 0.5, y + 0.5, z, 1) into the light's screen space, and the light's depth map.  fp64, no contraction.
// A pixel that cannot be tested - background, behind the light, outside the light's depth range or its map - is lit (255).
inline std::uint8_t shadow_byte(double z, int x, int y, const double* M, const double* map, int map_w, int map_h,
                                double bias, double darkness, int radius) {
    if (!std::isfinite(z)) return 255;
    const double p[4] = { x + 0.5, y + 0.5, z, 1.0 };                          // the pixel centre of our_gl.cpp:149
    double q[4];
    for (int r = 0; r < 4; ++r) {                                              // geometry.h:122-127,187-192
        double sum = 0;
        for (int c = 0; c < 4; ++c) sum += M[4 * r + c] * p[c];
        q[r] = sum;
    }
    if (!(q[3] > 1e-12)) return 255;                                           // our_gl.cpp:94
    double s[3];
    for (int k = 0; k < 3; ++k) { s[k] = q[k] / q[3]; if (!std::isfinite(s[k])) return 255; }   // geometry.h:117
    if (s[2] < -1.0 || s[2] > 1.0) return 255;                                 // our_gl.cpp:103
    if (!(s[0] >= 0.0 && s[0] < double(map_w) && s[1] >= 0.0 && s[1] < double(map_h))) return 255;
    const int ix = int(s[0]), iy = int(s[1]);
    const double limit = s[2] - bias;
    // the taps that lie inside the map; one outside never occludes, and neither does +inf or NaN (`<` is false)
    const int x_lo = ix - radius < 0 ? 0 : ix - radius, x_hi = ix > map_w - 1 - radius ? map_w - 1 : ix + radius;
    const int y_lo = iy - radius < 0 ? 0 : iy - radius, y_hi = iy > map_h - 1 - radius ? map_h - 1 : iy + radius;
    int occluded = 0;
    for (int ty = y_lo; ty <= y_hi; ++ty) {
        const double* row = map + std::size_t(ty) * map_w;
        for (int tx = x_lo; tx <= x_hi; ++tx) occluded += row[tx] < limit ? 1 : 0;
    }
    const int total = (2 * radius + 1) * (2 * radius + 1);
    const double factor = 1.0 - (double(occluded) / double(total)) * darkness;  // the shape of main.cpp:360-361
    return (unsigned char)(255.0 * factor);                                    // main.cpp:760
}
inline void shadow_mask_bytes(const double* depth, int w, int h, const double* M, const double* map, int map_w, int map_h,
                              double bias, double darkness, int radius, std::uint8_t* mask) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const std::size_t i = std::size_t(x) + std::size_t(y) * w;
            mask[i] = shadow_byte(depth[i], x, y, M, map, map_w, map_h, bias, darkness, radius);
        }
}

// The composite's arithmetic (main.cpp:775-781) with a one-byte factor per pixel, in place: the colour channels (at most three) are
// multiplied by mask / 255.0 and truncated; alpha stays.  A mask byte of 255 is the factor 1.0 exactly and changes nothing.
inline void modulate_bytes(std::uint8_t* pixels, std::size_t npixels, int bpp, const std::uint8_t* mask) {
    const int nc = bpp < 3 ? bpp : 3;
    for (std::size_t i = 0; i < npixels; ++i) {
        const double f = double(mask[i]) / 255.0;                              // :775
        for (int c = 0; c < nc; ++c) {
            const double v = double(pixels[i * bpp + c]) * f;
            pixels[i * bpp + c] = (unsigned char)(v < 255.0 ? v : 255.0);      // std::min(255.0, v), :777-781
        }
    }
}

}  // namespace trgl_image

struct TGAColor {
    std::uint8_t bgra[4] = { 0, 0, 0, 255 };
    std::uint8_t bytespp = 4;
    TGAColor() = default;
    TGAColor(std::uint8_t R, std::uint8_t G, std::uint8_t B, std::uint8_t A = 255) : bgra{ B, G, R, A }, bytespp(4) {}
    TGAColor(std::uint8_t v) : bgra{ v, v, v, 255 }, bytespp(1) {}
    TGAColor(const std::uint8_t* p, std::uint8_t bpp) : bgra{ 0, 0, 0, 0 }, bytespp(bpp) { for (int i = 0; i < bpp; ++i) bgra[i] = p[i]; }
    std::uint8_t& operator[](int i) { return bgra[i]; }
    const std::uint8_t& operator[](int i) const { return bgra[i]; }
    TGAColor operator*(float k) const {
        TGAColor r = *this;
        if (k < 0.f) k = 0.f;
        if (k > 1.f) k = 1.f;
        for (int i = 0; i < 4; ++i) r.bgra[i] = std::uint8_t(bgra[i] * k);
        return r;
    }
    std::uint32_t packed() const { return bgra[0] | (std::uint32_t(bgra[1]) << 8) | (std::uint32_t(bgra[2]) << 16) | (std::uint32_t(bgra[3]) << 24); }
};

class TGAImage {
public:
    enum Format { GRAYSCALE = 1, RGB = 3, RGBA = 4 };
    TGAImage() = default;
    TGAImage(int width, int height, int bytespp, TGAColor clear = TGAColor()) : w(width), h(height), bpp(std::uint8_t(bytespp)) {
        data.resize(std::size_t(w) * h * bpp);
        for (std::size_t i = 0; i < std::size_t(w) * h; ++i) for (int k = 0; k < bpp; ++k) data[i * bpp + k] = clear.bgra[k];
    }
    int width() const { return w; }
    int height() const { return h; }
    int bytespp() const { return bpp; }
    std::uint8_t* buffer() { return data.empty() ? nullptr : data.data(); }
    const std::uint8_t* buffer() const { return data.empty() ? nullptr : data.data(); }
    TGAColor get(int x, int y) const {
        if (data.empty() || x < 0 || y < 0 || x >= w || y >= h) return TGAColor();
        return TGAColor(&data[(std::size_t(x) + std::size_t(y) * w) * bpp], bpp);
    }
    void set(int x, int y, const TGAColor& c) {
        if (data.empty() || x < 0 || y < 0 || x >= w || y >= h) return;
        std::memcpy(&data[(std::size_t(x) + std::size_t(y) * w) * bpp], c.bgra, bpp);
    }
    void flip_vertically() {
        std::size_t line = std::size_t(w) * bpp;
        std::vector<std::uint8_t> tmp(line);
        for (int y = 0; y < h / 2; ++y) {
            std::uint8_t* a = &data[y * line]; std::uint8_t* b = &data[(h - 1 - y) * line];
            std::memcpy(tmp.data(), a, line); std::memcpy(a, b, line); std::memcpy(b, tmp.data(), line);
        }
    }
    void flip_horizontally() {
        for (int y = 0; y < h; ++y) for (int x = 0; x < w / 2; ++x) for (int k = 0; k < bpp; ++k)
            std::swap(data[(std::size_t(x) + std::size_t(y) * w) * bpp + k], data[(std::size_t(w - 1 - x) + std::size_t(y) * w) * bpp + k]);
    }
    // tgaimage.cpp:246-267: nearest-texel resize in the reference's int arithmetic; false (and nothing changed) for a size <= 0 or an empty image
    bool scale(int w2, int h2) {
        if (w2 <= 0 || h2 <= 0 || data.empty()) return false;
        std::vector<std::uint8_t> tdata(std::size_t(w2) * h2 * bpp);
        trgl_image::scale_bytes(data.data(), w, h, bpp, tdata.data(), w2, h2);
        w = w2; h = h2;
        data.swap(tdata);
        return true;
    }
    // tgaimage.cpp:271-324: separable Gaussian blur with clamped edges, float weights and a byte-quantised intermediate; does nothing for
    // radius <= 0 or an empty image.  (The reference's int i * i overflows beyond radius 46340; such a radius is not meaningful there either.)
    void gaussian_blur(const int radius) {
        if (radius <= 0 || data.empty()) return;
        std::vector<float> kernel(std::size_t(radius) * 2 + 1);
        trgl_image::gaussian_weights(radius, kernel.data());
        std::vector<std::uint8_t> tmp(data.size());
        trgl_image::blur_bytes(data.data(), w, h, bpp, radius, kernel.data(), tmp.data());
    }

    // The exact bytes TGAImage::write_tga_file(name, vflip, rle) puts on disk.
    std::vector<std::uint8_t> encode_tga(bool vflip = true, bool rle = true) const {
        std::vector<std::uint8_t> out(18, 0);
        out[2] = bpp == 1 ? (rle ? 11 : 3) : (rle ? 10 : 2);
        out[12] = std::uint8_t(w & 0xff); out[13] = std::uint8_t((w >> 8) & 0xff);
        out[14] = std::uint8_t(h & 0xff); out[15] = std::uint8_t((h >> 8) & 0xff);
        out[16] = std::uint8_t(bpp * 8);
        out[17] = vflip ? 0x00 : 0x20;
        if (!rle) { out.insert(out.end(), data.begin(), data.end()); return out; }
        const int npix = w * h, maxrun = 128;
        auto same = [&](int a, int b) { return std::memcmp(&data[std::size_t(a) * bpp], &data[std::size_t(b) * bpp], bpp) == 0; };
        for (int cur = 0; cur < npix;) {
            int run = 1;
            while (cur + run < npix && run < maxrun && same(cur + run, cur)) ++run;
            if (run > 1) {                                   // repeat packet
                out.push_back(std::uint8_t(run - 1 + 128));
                out.insert(out.end(), &data[std::size_t(cur) * bpp], &data[std::size_t(cur) * bpp] + bpp);
            } else {                                         // literal packet: stops AFTER meeting an equal neighbour pair
                while (cur + run < npix && run < maxrun && !same(cur + run, cur + run - 1)) ++run;
                out.push_back(std::uint8_t(run - 1));
                out.insert(out.end(), &data[std::size_t(cur) * bpp], &data[std::size_t(cur) * bpp] + std::size_t(run) * bpp);
            }
            cur += run;
        }
        return out;
    }
    bool write_tga_file(const std::string& filename, bool vflip = true, bool rle = true) const {
        std::ofstream out(filename, std::ios::binary);
        if (!out.is_open()) return false;
        auto bytes = encode_tga(vflip, rle);
        out.write(reinterpret_cast<const char*>(bytes.data()), std::streamsize(bytes.size()));
        return bool(out);
    }
    // TGAImage::read_tga_file (tgaimage.cpp:76-126) + load_rle_data (:128-160) on a file image in memory, with the
    // reference's std::ifstream behaviour spelled out: a short read delivers what is there and fails the stream, after
    // which every read is a no-op - so a truncated raw image keeps zeros, a truncated RLE stream repeats the last
    // colour read (chunk headers then read as 0 = one raw pixel), and neither is an error.  Errors (false) are: header
    // shorter than 18 bytes, width/height 0, bits per pixel not 8/24/32, data type not 2/3/10/11, and an RLE packet
    // running past the last pixel (the reference writes one pixel out of bounds before it notices; that write is not
    // reproduced).
    bool decode_tga(const std::uint8_t* file, std::size_t size) {
        data.clear();
        std::size_t pos = 0; bool good = true;
        auto rd = [&](std::uint8_t* dst, std::size_t k) {
            if (!good) return;
            std::size_t avail = pos < size ? size - pos : 0, m = k < avail ? k : avail;
            if (m) std::memcpy(dst, file + pos, m);
            pos += m;
            if (m < k) good = false;
        };
        std::uint8_t hd[18] = { 0 };
        rd(hd, 18);
        if (!good) return false;                                             // :86-90
        w = hd[12] | (hd[13] << 8); h = hd[14] | (hd[15] << 8); bpp = std::uint8_t(hd[16] >> 3);   // :92-94
        if (w <= 0 || h <= 0 || (bpp != 1 && bpp != 3 && bpp != 4)) return false;                // :96-99
        data.assign(std::size_t(w) * h * bpp, 0);                            // :101
        pos += hd[0];                                                        // :103 seekg(idlength, cur)
        if (hd[2] == 2 || hd[2] == 3) {
            rd(data.data(), data.size());                                    // :105-108
        } else if (hd[2] == 10 || hd[2] == 11) {
            const int npix = w * h;
            int cur = 0;
            TGAColor c;                                                      // :132, {0,0,0,255}
            while (cur < npix) {
                std::uint8_t head = 0;
                rd(&head, 1);
                const bool raw = head < 128;
                const int count = raw ? head + 1 : head - 127;
                if (!raw) rd(c.bgra, bpp);
                for (int i = 0; i < count; ++i) {
                    if (raw) rd(c.bgra, bpp);
                    if (cur >= npix) return false;                           // :145 / :155
                    std::memcpy(&data[std::size_t(cur++) * bpp], c.bgra, bpp);
                }
            }
        } else return false;                                                 // :113-116
        if (!(hd[17] & 0x20)) flip_vertically();                             // :118
        if (hd[17] & 0x10) flip_horizontally();                              // :119
        return true;
    }
    bool read_tga_file(const std::string& filename) {
        std::ifstream in(filename, std::ios::binary);
        if (!in.is_open()) return false;
        std::vector<std::uint8_t> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        return decode_tga(bytes.data(), bytes.size());
    }

private:
    int w = 0, h = 0;
    std::uint8_t bpp = 0;
    std::vector<std::uint8_t> data;
};

// The mip chain of an image (include/trgl.h, "Mipmapped textures"; new work, the reference has none): levels 1 .. L-1 in the packed
// layout of trgl_mip_layout, built by the library's host path - no GPU is touched.  `chain` is empty for a 1 x 1 image.  Programs that
// call it link the library; the declarations repeat include/trgl.h so that this header still stands alone.
struct trgl_ctx;
extern "C" int trgl_mip_layout(int w, int h, int bpp, int* levels, int widths[16], int heights[16], std::size_t offsets[16], std::size_t* total);
extern "C" int trgl_image_mipmaps(trgl_ctx* ctx, const std::uint8_t* src, int w, int h, int bpp, std::uint8_t* dst, int mem_kind);
namespace trgl_image {
inline bool mipmaps(const TGAImage& img, std::vector<std::uint8_t>* chain, int* levels = nullptr) {
    std::size_t total = 0;
    int L = 0;
    if (!chain || trgl_mip_layout(img.width(), img.height(), img.bytespp(), &L, nullptr, nullptr, nullptr, &total) != 0) return false;
    chain->assign(total, 0);
    if (levels) *levels = L;
    return trgl_image_mipmaps(nullptr, img.buffer(), img.width(), img.height(), img.bytespp(), chain->data(), 0 /* TRGL_MEM_HOST */) == 0;
}
}  // namespace trgl_image
