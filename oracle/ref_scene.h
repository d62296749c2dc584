// ref_scene.h — TEST INFRASTRUCTURE, NOT PRODUCT.
//
// What oracle/ref_harness.cpp and oracle/ref_shaders.cpp share: the reader of the scene files oracle/orc.py writes, the
// FLAT / GOURAUD / CHECKER shaders on the reference's own TGAColor, and the scene loop around the reference's rasterize()
// (compiled in place from the reference tree, see oracle/Makefile).  The two harnesses differ only in how a PHONG or
// EYE draw is shaded: `Lit` below.
#pragma once

#include "our_gl.h"          // from -I<reference tree>
#include "trgl_oracle.h"     // orc_texture, trgl_uniforms, TRGL_* (layouts only)

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

namespace refscene {

struct Reader {
    std::vector<unsigned char> buf; size_t pos = 0;
    bool load(const char* path) {
        std::ifstream in(path, std::ios::binary);
        if (!in) return false;
        buf.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        return true;
    }
    template <class T> T get() { T v; std::memcpy(&v, &buf[pos], sizeof(T)); pos += sizeof(T); return v; }
    const unsigned char* take(size_t n) { const unsigned char* p = &buf[pos]; pos += n; return p; }
    void align8() { pos = (pos + 7) & ~size_t(7); }
};

inline TGAColor color_from_packed(uint32_t v) {
    return TGAColor((uint8_t)((v >> 16) & 0xff), (uint8_t)((v >> 8) & 0xff), (uint8_t)(v & 0xff), (uint8_t)((v >> 24) & 0xff));
}

struct FlatShader : IShader {
    TGAColor color;
    std::pair<bool, TGAColor> fragment(const vec3) const override { return { false, color }; }
};

struct GouraudShader : IShader {
    double intensity[3]; TGAColor base;
    std::pair<bool, TGAColor> fragment(const vec3 bar) const override {
        double i = intensity[0] * bar[0] + intensity[1] * bar[1] + intensity[2] * bar[2];
        return { false, base * (float)i };      // TGAColor::operator*(float), tgaimage.h:55-62
    }
};

// The discarding kind (include/trgl.h, TRGL_SHADER_CHECKER): exercises `if (discard) continue;` of the reference's rasterize()
// (our_gl.cpp:187-188) - no depth write, no colour write, no counters for a discarded fragment.
struct CheckerShader : IShader {
    TGAColor color; int cells;
    std::pair<bool, TGAColor> fragment(const vec3 bar) const override {
        const int a = (int)(bar[0] * cells), c = (int)(bar[1] * cells);
        return { ((a ^ c) & 1) != 0, color };
    }
};

// Writes what a scene run leaves: framebuffer bytes, z-buffer, the print_render_stats() line (our_gl.cpp:204-210), seconds.
inline int write_scene_output(const char* out_path, TGAImage& framebuffer, int W, int H, int bpp, double raster_seconds) {
    std::ostringstream captured;
    std::streambuf* old = std::cerr.rdbuf(captured.rdbuf());
    print_render_stats();
    std::cerr.rdbuf(old);
    std::string line = captured.str();

    std::ofstream out(out_path, std::ios::binary);
    size_t fb_bytes = (size_t)W * H * bpp;
    out.write((const char*)framebuffer.buffer(), fb_bytes);
    static const char pad[8] = { 0 };
    out.write(pad, (8 - fb_bytes % 8) % 8);
    out.write((const char*)zbuffer.data(), zbuffer.size() * sizeof(double));
    int32_t len = (int32_t)line.size();
    out.write((const char*)&len, 4);
    out.write(line.data(), len);
    out.write(pad, (8 - (4 + len) % 8) % 8);
    out.write((const char*)&raster_seconds, 8);
    return out ? 0 : 3;
}

// One scene file -> one frame.  Lit shades PHONG / EYE draws:
//   void draw(int kind, const trgl_uniforms& u, const std::vector<orc_texture>& tex)   once per such draw, before its triangles;
//   const IShader& triangle(const double* vary)                                       per triangle (24 varyings, trgl.h layout).
template <class Lit>
int run_scene(const char* in_path, const char* out_path, Lit& lit) {
    Reader r;
    if (!r.load(in_path)) { std::fprintf(stderr, "cannot read %s\n", in_path); return 2; }
    if (std::memcmp(r.take(8), "TRGSCN01", 8) != 0) { std::fprintf(stderr, "bad magic\n"); return 2; }
    int W = r.get<int32_t>(), H = r.get<int32_t>(), bpp = r.get<int32_t>();
    int ndraws = r.get<int32_t>(), ntex = r.get<int32_t>(); r.get<int32_t>();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Viewport[i][j] = r.get<double>();
    uint8_t clear[4]; std::memcpy(clear, r.take(4), 4); r.take(4);
    double zclear = r.get<double>();

    std::vector<orc_texture> tex(TRGL_MAX_TEXTURES, orc_texture{ nullptr, 0, 0, 0 });
    for (int t = 0; t < ntex; ++t) {
        int slot = r.get<int32_t>(), w = r.get<int32_t>(), h = r.get<int32_t>(), tb = r.get<int32_t>();
        tex[slot] = orc_texture{ r.take((size_t)w * h * tb), w, h, tb };
        r.align8();
    }

    TGAColor clear_color(clear, (uint8_t)4);
    TGAImage framebuffer(W, H, bpp, clear_color);
    init_zbuffer(W, H);
    if (!(zclear == std::numeric_limits<double>::infinity()))
        for (auto& z : zbuffer) z = zclear;

    double raster_seconds = 0.0;      // time inside the per-triangle rasterize() loops only
    for (int d = 0; d < ndraws; ++d) {
        int kind = r.get<int32_t>(); r.get<int32_t>();
        uint64_t n = r.get<uint64_t>();
        trgl_uniforms u; std::memcpy(&u, r.take(sizeof(u)), sizeof(u));
        const double* clip = (const double*)r.take(n * 12 * sizeof(double));
        const bool lit_kind = kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE;
        int K = kind == TRGL_SHADER_GOURAUD ? TRGL_VARY_GOURAUD : lit_kind ? 24 : 0;
        const double* vary = (const double*)r.take(n * K * sizeof(double));
        const uint32_t* colors = (const uint32_t*)r.take(n * sizeof(uint32_t));
        r.align8();

        FlatShader flat; GouraudShader gour; CheckerShader chk;
        chk.cells = u.reserved;
        if (lit_kind) lit.draw(kind, u, tex);
        auto t0 = std::chrono::steady_clock::now();
        for (uint64_t i = 0; i < n; ++i) {
            vec4 tri[3];
            for (int v = 0; v < 3; ++v) for (int c = 0; c < 4; ++c) tri[v][c] = clip[i * 12 + v * 4 + c];
            if (kind == TRGL_SHADER_FLAT) {
                flat.color = color_from_packed(colors[i]);
                rasterize(tri, flat, framebuffer);
            } else if (kind == TRGL_SHADER_CHECKER) {
                chk.color = color_from_packed(colors[i]);
                rasterize(tri, chk, framebuffer);
            } else if (kind == TRGL_SHADER_GOURAUD) {
                for (int v = 0; v < 3; ++v) gour.intensity[v] = vary[i * 3 + v];
                gour.base = color_from_packed(colors[i]);
                rasterize(tri, gour, framebuffer);
            } else {
                rasterize(tri, lit.triangle(vary + i * 24), framebuffer);
            }
        }
        raster_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return write_scene_output(out_path, framebuffer, W, H, bpp, raster_seconds);
}

}  // namespace refscene
