// user_prelude.h — what a user shader's source sees (include/trgl.h, "User shaders"): compiled by hiprtc ahead of the source,
// from the copy user_shaders.cpp embeds, for both fragment contracts (shade_user.h and raster_user.h) and for vertex shaders
// (vertex_user.h).  The sampler is the one k_shade uses (shade_common.h).
#pragma once
#include "shade_common.h"
#include "mip_core.h"

struct trgl_frag_in {
    double bar[3];               // perspective-correct barycentrics (our_gl.cpp:168-185)
    const double* vary;          // this triangle's K varyings (null when K = 0)
    const trgl_uniforms* u;      // the draw's uniform block
    uint32_t color;              // this triangle's `colors` entry, 0xffffffff when the draw has none (k_setup)
    const DevTexture* tex;       // the context's texture table (trgl_sample2D)
    uint32_t dst;                // with TRGL_SHADER_READS_DEST the pixel as TGAImage::get returns it now: bpp bytes, the rest zero; else 0
};
struct trgl_texel { uint32_t bgra; int bytespp; };   // TGAColor (tgaimage.h:29-31), bgra[0] in the low byte
// what trgl_fragment returns with TRGL_SHADER_MAY_DISCARD: std::pair<bool, TGAColor> of IShader::fragment (our_gl.h:51)
struct trgl_frag_out { bool discard; uint32_t bgra; };

// IShader::sample2D / Model::diffuse (model.cpp:415-459): clamp(int(uv * size), 0, size - 1), nearest texel; an empty slot samples
// as opaque white (model.cpp:416-418)
__device__ __forceinline__ trgl_texel trgl_sample2D(const trgl_frag_in& in, int slot, const double uv[2]) {
    const DevTexture* t = trgl_shade::tex_slot(in.tex, slot);
    if (!t) return trgl_texel{ 0xffffffffu, 4 };
    const trgl_shade::Color c = trgl_shade::tex_fetch(t, uv);
    return trgl_texel{ c.bgra, c.bytespp };
}

// ---- mipmapped textures (include/trgl.h, "Mipmapped textures"; the arithmetic is mip_core.h's, which the host compiles too) ----
// The slot as a mip view: level 0 and, behind it in the slot's own allocation, the levels trgl_texture_mipmaps built (DevTexture::pad
// holds their number).  false: the slot is empty.
__device__ __forceinline__ bool trgl_mip_view(const trgl_frag_in& in, int slot, trgl::MipView* v) {
    const DevTexture* t = trgl_shade::tex_slot(in.tex, slot);
    if (!t) return false;
    *v = trgl::MipView{ t->data, t->data, t->w, t->h, t->bpp, 1 + t->pad, true };
    return true;
}
// L and the size of level 0; 0 for an empty slot (w and h are then left alone)
__device__ __forceinline__ int trgl_texture_levels(const trgl_frag_in& in, int slot, int* w, int* h) {
    trgl::MipView v;
    if (!trgl_mip_view(in, slot, &v)) return 0;
    *w = v.w; *h = v.h;
    return v.levels;
}
// trgl_sample2D's rule on level `level` (clamped to 0..L-1)
__device__ __forceinline__ trgl_texel trgl_sample2D_level(const trgl_frag_in& in, int slot, const double uv[2], int level) {
    trgl::MipView v;
    if (!trgl_mip_view(in, slot, &v)) return trgl_texel{ 0xffffffffu, 4 };
    const trgl::MipTexel c = trgl::mip_sample_level(v, uv, level);
    return trgl_texel{ c.bgra, c.bytespp };
}
// bilinear on level `level`: weights in 1/256, texel centres at (i + 0.5) / size, clamp at the edges
__device__ __forceinline__ trgl_texel trgl_sample2D_linear(const trgl_frag_in& in, int slot, const double uv[2], int level) {
    trgl::MipView v;
    if (!trgl_mip_view(in, slot, &v)) return trgl_texel{ 0xffffffffu, 4 };
    const trgl::MipTexel c = trgl::mip_sample_linear(v, uv, level);
    return trgl_texel{ c.bgra, c.bytespp };
}
// trilinear: the bilinear samples of levels floor(lod) and floor(lod) + 1, blended in 1/256
__device__ __forceinline__ trgl_texel trgl_sample2D_trilinear(const trgl_frag_in& in, int slot, const double uv[2], double lod) {
    trgl::MipView v;
    if (!trgl_mip_view(in, slot, &v)) return trgl_texel{ 0xffffffffu, 4 };
    const trgl::MipTexel c = trgl::mip_sample_trilinear(v, uv, lod);
    return trgl_texel{ c.bgra, c.bytespp };
}
// the level of detail of this pixel from the four per-triangle doubles trgl_lod_stage left in the varyings
__device__ __forceinline__ double trgl_mip_lod(const double bar[3], const double k[4], int tex_w, int tex_h) {
    return trgl::mip_lod(bar, k, tex_w, tex_h);
}

// source-over with the source's alpha byte a, in integers (include/trgl.h, "User shaders that blend"): per B, G, R
// (s a + d (255 - a) + 127) / 255, and for the alpha byte (255 a + d_a (255 - a) + 127) / 255
__device__ __forceinline__ uint32_t trgl_blend_over(uint32_t src, uint32_t dst) {
    const uint32_t a = src >> 24, na = 255u - a;
    uint32_t out = 0;
    for (int i = 0; i < 24; i += 8) out |= ((((src >> i) & 255u) * a + ((dst >> i) & 255u) * na + 127u) / 255u) << i;
    return out | (((255u * a + (dst >> 24) * na + 127u) / 255u) << 24);
}

// ---- user vertex shaders (include/trgl.h, "User vertex shaders"; the kernel behind the source is vertex_user.h) ----
// what IShader::vertex(face, nth) (our_gl.h:46) reads: the vertex the index buffer names, the draw's uniforms, the global Perspective
struct trgl_vert_in {
    const double* vertex;        // this vertex's record, `stride` doubles (Model::vertices[index])
    int stride;
    uint32_t index;              // the entry of the index buffer, indices[3 * face + nth]
    int face, nth;               // the arguments of IShader::vertex; nth is 0, 1 or 2
    const trgl_uniforms* u;      // the draw's uniform block (texture slots -1 when the draw passed none)
    const double* projection;    // 16 doubles, row-major
    uint32_t instance;           // instanced calls: the instance's original number; else 0
    const double* inst;          // instanced calls: this instance's record (null when the call has none); else null
    int inst_stride;             // instanced calls: doubles per instance record; else 0
};
// what it leaves: its return value and the shader's varying member arrays
struct trgl_vert_out {
    double clip[4];              // the return value of vertex(); (0, 0, 0, 0) until written
    double* vary;                // this TRIANGLE's K doubles, shared by the three calls of the face, zero before them (null when K = 0)
};
