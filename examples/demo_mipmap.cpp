// demo_mipmap.cpp — mipmapped textures over the C ABI (new work; include/trgl.h, "Mipmapped textures").
// A checkerboard ground plane recedes under perspective; above the horizon hangs a small screen that shows the frame drawn so far.
//   * the board is uploaded into slot 0 and trgl_texture_mipmaps builds its chain in HBM;
//   * the plane's rows come from trgl_vertex_stage, trgl_lod_stage appends the four level-of-detail doubles, trgl_draw draws them with a
//     user kind;
//   * the frame with the plane is captured into slot 1 (trgl_texture_from_framebuffer), gets a chain too, and the screen samples it.
// The scene is drawn twice: with a kind that calls trgl_sample2D (one nearest texel of level 0: the far cells alias into noise) and with
// one that calls trgl_sample2D_trilinear(..., trgl_mip_lod(...)) (the far cells fade into their mean).
//   demo_mipmap <nearest.tga> <trilinear.tga>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/trgl.h"

static const int W = 160, H = 120, T = 256, CELL = 8;

// varyings: the 24 doubles of the built-in vertex stage, u v of the three vertices first; trgl_lod_stage wrote doubles 20..23
static const char* kNearest = R"(
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    return trgl_sample2D(in, in.u->tex_diffuse, uv).bgra | 0xff000000u;
}
)";
static const char* kTrilinear = R"(
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    int w = 1, h = 1;
    trgl_texture_levels(in, in.u->tex_diffuse, &w, &h);
    return trgl_sample2D_trilinear(in, in.u->tex_diffuse, uv, trgl_mip_lod(in.bar, v + 20, w, h)).bgra | 0xff000000u;
}
)";

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_mipmap: %s: %d: %s\n", #call, rc_, trgl_last_error(ctx)); return 2; } \
    } while (0)

struct Quad { double verts[4][14]; double clip[2][12]; double vary[2][24]; };

// four corners (x, y, z) with uv (0,0) (1,0) (1,1) (0,1): pos3, normal3, uv2, tangent3, bitangent3 per vertex
static void make_quad(Quad& q, const double corners[4][3]) {
    static const double uv[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
    std::memset(&q, 0, sizeof(q));
    for (int i = 0; i < 4; ++i) {
        for (int a = 0; a < 3; ++a) q.verts[i][a] = corners[i][a];
        q.verts[i][4] = 1.0;
        q.verts[i][6] = uv[i][0]; q.verts[i][7] = uv[i][1];
    }
}

static bool write_tga(trgl_ctx* ctx, const char* path) {
    std::vector<uint8_t> px((size_t)W * H * 3), file(trgl_tga_max_size(W, H, 3));
    size_t len = file.size();
    if (trgl_read_framebuffer(ctx, px.data()) != TRGL_OK) return false;
    if (trgl_tga_encode(px.data(), W, H, 3, 1, 1, file.data(), &len) != TRGL_OK) return false;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(file.data(), 1, len, f) == len;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: demo_mipmap <nearest.tga> <trilinear.tga>\n"); return 1; }
    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_mipmap: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double viewport[16] = { W / 2.0, 0, 0, W / 2.0, 0, H / 2.0, 0, H / 2.0, 0, 0, 1, 0, 0, 0, 0, 1 };

    std::vector<uint8_t> board((size_t)T * T * 3);
    for (int y = 0; y < T; ++y)
        for (int x = 0; x < T; ++x) {
            const bool light = ((x / CELL + y / CELL) & 1) != 0;
            uint8_t* p = &board[((size_t)y * T + x) * 3];
            p[0] = light ? 230 : 30; p[1] = light ? 230 : 40; p[2] = light ? 230 : 200;
        }
    CHECK(trgl_upload_texture(ctx, 0, board.data(), T, T, 3));
    CHECK(trgl_texture_mipmaps(ctx, 0));

    int kinds[2] = { -1, -1 };
    CHECK(trgl_register_shader(ctx, kNearest, 24, &kinds[0]));
    CHECK(trgl_register_shader(ctx, kTrilinear, 24, &kinds[1]));

    double proj[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -1.0 / 3.0, 1 };
    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    for (int i = 0; i < 4; ++i) u.model_view[5 * i] = 1.0;
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_normal = u.tex_specular = -1;

    const double ground[4][3] = { { -1.2, -0.9, 0.5 }, { 1.2, -0.9, 0.5 }, { 14.0, 0.6, -24.0 }, { -14.0, 0.6, -24.0 } };
    const double screen[4][3] = { { 0.30, 0.30, 0.0 }, { 0.90, 0.30, 0.0 }, { 0.90, 0.85, 0.0 }, { 0.30, 0.85, 0.0 } };
    const uint32_t faces[6] = { 0, 1, 2, 0, 2, 3 };
    Quad quads[2];
    make_quad(quads[0], ground);
    make_quad(quads[1], screen);
    for (Quad& q : quads) {
        CHECK(trgl_vertex_stage(ctx, -1, &u, proj, &q.verts[0][0], 14, 4, faces, 2, &q.clip[0][0], &q.vary[0][0], TRGL_MEM_HOST));
        CHECK(trgl_lod_stage(nullptr, viewport, &q.clip[0][0], &q.vary[0][0], 2, 24, 0, 20, TRGL_MEM_HOST));
    }

    const uint8_t sky[4] = { 40, 30, 20, 255 };
    for (int pass = 0; pass < 2; ++pass) {
        CHECK(trgl_clear(ctx, sky, 1.0 / 0.0));
        u.tex_diffuse = 0;
        CHECK(trgl_draw(ctx, kinds[pass], &u, &quads[0].clip[0][0], &quads[0].vary[0][0], nullptr, 2, TRGL_MEM_HOST));
        CHECK(trgl_texture_from_framebuffer(ctx, 1, 1));      // the frame so far, without leaving HBM; the second pass reuses the slot's memory
        CHECK(trgl_texture_mipmaps(ctx, 1));
        u.tex_diffuse = 1;
        CHECK(trgl_draw(ctx, kinds[pass], &u, &quads[1].clip[0][0], &quads[1].vary[0][0], nullptr, 2, TRGL_MEM_HOST));
        if (!write_tga(ctx, argv[1 + pass])) { std::fprintf(stderr, "demo_mipmap: cannot write %s\n", argv[1 + pass]); return 3; }
    }
    trgl_destroy(ctx);
    return 0;
}
