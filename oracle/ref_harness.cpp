// ref_harness.cpp — TEST INFRASTRUCTURE, NOT PRODUCT.
//
// Drives the reference's own rasterize() (compiled, unmodified, from /root/reference/our_gl.cpp +
// tgaimage.cpp where they lie — see oracle/Makefile; nothing of the reference is copied here) over
// scene files written by oracle/orc.py, and dumps framebuffer, z-buffer and the
// print_render_stats() line.  Used only in the build container to (1) validate the C restatement
// oracle/trgl_oracle.c bit-for-bit and (2) generate the golden fixtures under tests/golden/.
//
// One process per scene: the reference's diagnostic counters are file-static and never reset
// (our_gl.cpp:18-22).
//
// Shaders here are IShader subclasses (our_gl.h:36-52):
//   FLAT / GOURAUD / CHECKER are defined on the reference's own TGAColor (tgaimage.h:29-63); CHECKER is the one that discards;
//   PHONG / EYE call the C restatement's fragment (orc_fragment).  This harness does not link main.cpp;
//   the restated bodies are pinned by the second harness, oracle/ref_shaders.cpp, which does (against
//   declaration-only Assimp stand-ins) and shades with the reference's own PhongShader / EyeShader.
//   oracle/orc.py run_reference sends every scene with a PHONG or EYE draw there, so the goldens of
//   such scenes come from the reference's shaders; ref_harness keeps FLAT / GOURAUD / CHECKER scenes
//   and the restated up-call for direct comparison.
// Mode "vecops" evaluates geometry.h / tgaimage.h value ops on given inputs so the restatement's
// helpers can be compared with the real ones.

#include "ref_scene.h"

namespace {

using refscene::Reader;
using refscene::color_from_packed;

// PHONG / EYE through the C restatement's fragment (orc_fragment), for every triangle of the draw.
struct RestatedFragShader : IShader {
    int kind; const trgl_uniforms* u; const orc_texture* tex; const double* vary;
    std::pair<bool, TGAColor> fragment(const vec3 bar) const override {
        double b[3] = { bar[0], bar[1], bar[2] };
        uint8_t bgra[4];
        int bytespp = orc_fragment(kind, u, tex, vary, 0, b, bgra);
        TGAColor c(bgra, (uint8_t)4);
        c.bytespp = (uint8_t)bytespp;
        return { false, c };
    }
};

struct RestatedLit {
    RestatedFragShader rest; trgl_uniforms u;
    void draw(int kind, const trgl_uniforms& uu, const std::vector<orc_texture>& tex) {
        u = uu; rest.kind = kind; rest.u = &u; rest.tex = tex.data();
    }
    const IShader& triangle(const double* vary) { rest.vary = vary; return rest; }
};

int run_scene(const char* in_path, const char* out_path) {
    RestatedLit lit;
    return refscene::run_scene(in_path, out_path, lit);
}

// vecops: input = int32 count, then per item 3+3+16+9+3+1 doubles (v, n, M, v0v1v2, b, intensity) and
// uint32 colour; output per item: normalized(v)[3], (M*vec4(n,0)).xyz[3], v0*b0+v1*b1+v2*b2 [3],
// then 4 bytes (colour * (float)intensity).
int run_vecops(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path)) return 2;
    int count = r.get<int32_t>(); r.get<int32_t>();
    std::ofstream out(out_path, std::ios::binary);
    for (int i = 0; i < count; ++i) {
        vec3 v, n, v0, v1, v2, b; mat<4, 4> M;
        for (int k = 0; k < 3; ++k) v[k] = r.get<double>();
        for (int k = 0; k < 3; ++k) n[k] = r.get<double>();
        for (int a = 0; a < 4; ++a) for (int c = 0; c < 4; ++c) M[a][c] = r.get<double>();
        for (int k = 0; k < 3; ++k) v0[k] = r.get<double>();
        for (int k = 0; k < 3; ++k) v1[k] = r.get<double>();
        for (int k = 0; k < 3; ++k) v2[k] = r.get<double>();
        for (int k = 0; k < 3; ++k) b[k] = r.get<double>();
        double inten = r.get<double>();
        uint32_t packed = r.get<uint32_t>(); r.get<uint32_t>();
        vec3 nv = normalized(v);
        vec3 md = (M * make_vec4(n[0], n[1], n[2], 0.0)).xyz();
        vec3 ip = v0 * b[0] + v1 * b[1] + v2 * b[2];
        TGAColor sc = color_from_packed(packed) * (float)inten;
        double o[9] = { nv[0], nv[1], nv[2], md[0], md[1], md[2], ip[0], ip[1], ip[2] };
        out.write((const char*)o, sizeof(o));
        out.write((const char*)sc.bgra, 4);
        static const char pad[4] = { 0 };
        out.write(pad, 4);
    }
    return out ? 0 : 3;
}

// tga: input = int32 w,h,bpp,vflip,rle,pad + pixel bytes; output = the file TGAImage::write_tga_file produces.
int run_tga(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path)) return 2;
    int w = r.get<int32_t>(), h = r.get<int32_t>(), bpp = r.get<int32_t>(), vflip = r.get<int32_t>(), rle = r.get<int32_t>();
    r.get<int32_t>();
    TGAImage img(w, h, bpp);
    std::memcpy(img.buffer(), r.take((size_t)w * h * bpp), (size_t)w * h * bpp);
    return img.write_tga_file(out_path, vflip != 0, rle != 0) ? 0 : 3;      // tgaimage.cpp:161-191
}

// tgaread: input = a .tga file; output = int32 ok, w, h, bpp + (if ok) the TGAImage buffer after TGAImage::read_tga_file.
int run_tgaread(const char* in_path, const char* out_path) {
    TGAImage img;
    const bool ok = img.read_tga_file(in_path);                                   // tgaimage.cpp:76-126
    std::ofstream out(out_path, std::ios::binary);
    int32_t hd[4] = { ok ? 1 : 0, img.width(), img.height(), 0 };
    if (ok) hd[3] = img.get(0, 0).bytespp;                                         // TGAColor(p, bpp), tgaimage.h:47-51
    out.write((const char*)hd, sizeof hd);
    if (ok) out.write((const char*)img.buffer(), (std::streamsize)hd[1] * hd[2] * hd[3]);
    return out ? 0 : 3;
}

// sample2d: input = int32 w, h, bpp, count + texels (padded to 8) + count x 2 doubles (uv); output per sample: bgra[4], bytespp,
// 3 pad bytes, from the reference's own IShader::sample2D (our_gl.h:38-44) -> TGAImage::get (tgaimage.cpp:24-30).  Model::diffuse /
// normal / specular (model.cpp:415-459, not compilable here: Assimp) use the same clamp(int(uv * size), 0, size - 1) + get().
int run_sample2d(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path)) return 2;
    int w = r.get<int32_t>(), h = r.get<int32_t>(), bpp = r.get<int32_t>(), count = r.get<int32_t>();
    TGAImage img(w, h, bpp);
    std::memcpy(img.buffer(), r.take((size_t)w * h * bpp), (size_t)w * h * bpp);
    r.align8();
    std::ofstream out(out_path, std::ios::binary);
    for (int i = 0; i < count; ++i) {
        vec2 uv; uv.x = r.get<double>(); uv.y = r.get<double>();
        TGAColor c = IShader::sample2D(img, uv);
        unsigned char rec[8] = { c.bgra[0], c.bgra[1], c.bgra[2], c.bgra[3], c.bytespp, 0, 0, 0 };
        out.write((const char*)rec, 8);
    }
    return out ? 0 : 3;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "scene") == 0) return run_scene(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "vecops") == 0) return run_vecops(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "tga") == 0) return run_tga(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "tgaread") == 0) return run_tgaread(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "sample2d") == 0) return run_sample2d(argv[2], argv[3]);
    std::fprintf(stderr, "usage: ref_harness scene|vecops|tga|tgaread|sample2d <in> <out>\n");
    return 1;
}
