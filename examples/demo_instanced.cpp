// demo_instanced.cpp — one mesh under many model matrices, gated by occlusion codes that never leave HBM (include/trgl.h:
// trgl_occlusion_boxes, trgl_draw_instanced), over the C ABI.
// An occluder wall is drawn first.  The boxes of a grid of cubes behind it are asked against the depths it left, with boxes and codes in
// device memory: trgl_occlusion_boxes queues the query and does not wait.  One trgl_draw_instanced call then draws the cube under every
// matrix whose code has bit 0 set - the codes array is its `visible` argument as it is - and waits once, for the count of drawn cubes.
//   demo_instanced [width height] [all | shim]
// prints the print_render_stats() line (stderr), the number of cubes drawn and the FNV-1a digest of the frame.  With `all` the codes are
// ignored: the digest and fragments_drawn must be the same, since a cube that was skipped had no fragment to give.  With `shim` the same
// scene goes through the shim instead (gl_occlusion_test, whose codes come to the host, and gl_draw_instanced): the same output.
// Every number of the scene is a dyadic fraction and every product is summed in geometry.h's order, so the scene is the same doubles
// wherever it is restated (tests/test_instanced_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_instanced: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_instanced: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

// geometry.h:122-127 and 196-205: sums from 0, left to right
static double dot4(const double* m, double x, double y, double z, double w) {
    double s = 0;
    s += m[0] * x; s += m[1] * y; s += m[2] * z; s += m[3] * w;
    return s;
}
static void mat_mul(const double* a, const double* b, double* out) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            out[4 * i + j] = s;
        }
}

// stands in for the reference's Model where PhongShaderT asks it: a material without maps
struct NoMaps {
    vec3 vert(int, int) const { return vec3(); } vec3 normal(int, int) const { return vec3(); } vec2 uv(int, int) const { return vec2(); }
    int diffuse_slot() const { return -1; } int normal_slot() const { return -1; } int specular_slot() const { return -1; }
};

static void print_digest(const std::uint8_t* px, size_t bytes, unsigned long long drawn, int n) {
    std::uint64_t digest = 1469598103934665603ull;                              // FNV-1a over the frame's bytes
    for (size_t i = 0; i < bytes; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    std::printf("cubes drawn: %llu of %d\nframe digest: %016llx\n", drawn, n, (unsigned long long)digest);
}

// the scene through the shim: the loop over models of main.cpp:647-736 as gl_occlusion_test + one gl_draw_instanced
static int run_shim(int W, int H, const double* model_view, const double* projection, const double* wall_clip, const double* cube,
                    const std::uint32_t* faces, const std::vector<double>& matrices, const std::vector<double>& boxes, int N) {
    TGAImage fb(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    init_viewport(0, 0, W, H);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
    FlatShader flat;
    flat.color = TGAColor(0x80, 0x88, 0x90);
    for (int t = 0; t < 2; ++t) {
        Triangle clip;
        for (int v = 0; v < 3; ++v) clip[v] = make_vec4(wall_clip[12 * t + 4 * v], wall_clip[12 * t + 4 * v + 1], wall_clip[12 * t + 4 * v + 2], wall_clip[12 * t + 4 * v + 3]);
        rasterize(clip, flat, fb);
    }
    std::vector<AABB> world(N);
    std::vector<mat<4, 4>> models(N);
    for (int k = 0; k < N; ++k) {
        for (int a = 0; a < 3; ++a) { world[k].min[a] = boxes[6 * size_t(k) + a]; world[k].max[a] = boxes[6 * size_t(k) + 3 + a]; }
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) models[k][r][c] = matrices[16 * size_t(k) + 4 * r + c];
    }
    const std::vector<std::uint8_t> codes = gl_occlusion_test(world, Perspective * ModelView);
    NoMaps none;
    PhongShaderT<NoMaps> shader(&none);                                        // constructed once, under the view's ModelView
    shader.key_light_dir_eye = shader.fill_light_dir_eye = shader.rim_light_dir_eye = make_vec3(0.0, 0.0, 1.0);
    unsigned long long drawn = 0;
    for (std::uint8_t c : codes) drawn += gl_occlusion_draw(c) ? 1 : 0;
    if (!gl_draw_instanced(shader, cube, 8, 8, faces, 12, models, fb, codes.data()) || !gl_flush(fb)) {
        std::fprintf(stderr, "demo_instanced: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 2;
    }
    print_render_stats();
    print_digest(fb.buffer(), size_t(W) * H * 3, drawn, N);
    gl_shutdown();
    return 0;
}

int main(int argc, char** argv) {
    const bool all = argc > 1 && std::strcmp(argv[argc - 1], "all") == 0;
    const bool shim = argc > 1 && std::strcmp(argv[argc - 1], "shim") == 0;
    const int nsize = argc - 1 - (all || shim ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_instanced [width height] [all | shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_instanced: bad size\n"); return 1; }

    // the camera: five units in front of the origin, looking down -z
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    double view_proj[16];
    mat_mul(projection, model_view, view_proj);                                 // main.cpp:623

    // the occluder: a wall over the left half of the view, at z = 0
    const double wall[4][3] = { { -6, -4, 0 }, { 0, -4, 0 }, { 0, 4, 0 }, { -6, 4, 0 } };
    const int corner[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
    double wall_clip[24];
    for (int t = 0; t < 2; ++t)
        for (int v = 0; v < 3; ++v) {
            const double* p = wall[corner[t][v]];
            double eye[4];
            for (int r = 0; r < 4; ++r) eye[r] = dot4(model_view + 4 * r, p[0], p[1], p[2], 1.0);
            for (int r = 0; r < 4; ++r) wall_clip[12 * t + 4 * v + r] = dot4(projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
        }
    const std::uint32_t wall_colors[2] = { 0xff808890u, 0xff808890u };

    // the mesh: a cube of side 1 (position, normal = position / 2, uv), 12 faces
    double cube[8][8];
    for (int k = 0; k < 8; ++k) {
        const double p[3] = { k & 1 ? 0.5 : -0.5, k & 2 ? 0.5 : -0.5, k & 4 ? 0.5 : -0.5 };
        for (int a = 0; a < 3; ++a) { cube[k][a] = p[a]; cube[k][3 + a] = p[a] * 0.5; }
        cube[k][6] = p[0] + 0.5; cube[k][7] = p[1] + 0.5;
    }
    const std::uint32_t faces[12][3] = { { 0, 2, 1 }, { 1, 2, 3 }, { 4, 5, 6 }, { 5, 7, 6 }, { 0, 1, 4 }, { 1, 5, 4 },
                                         { 2, 6, 3 }, { 3, 6, 7 }, { 0, 4, 2 }, { 2, 4, 6 }, { 1, 3, 5 }, { 3, 7, 5 } };

    // the instances: cubes of side 1/4 on a 12 x 6 grid three units behind the wall's plane, and their boxes (the cube and half as much again)
    const int NX = 12, NY = 6, N = NX * NY;
    std::vector<double> matrices(size_t(N) * 16, 0.0), boxes(size_t(N) * 6);
    for (int j = 0; j < NY; ++j)
        for (int i = 0; i < NX; ++i) {
            const int k = j * NX + i;
            const double c[3] = { -2.75 + 0.5 * i, -1.25 + 0.5 * j, -3.0 };
            double* m = &matrices[size_t(k) * 16];
            m[0] = m[5] = m[10] = 0.25; m[15] = 1.0;
            m[3] = c[0]; m[7] = c[1]; m[11] = c[2];
            for (int a = 0; a < 3; ++a) { boxes[6 * size_t(k) + a] = c[a] - 0.1875; boxes[6 * size_t(k) + 3 + a] = c[a] + 0.1875; }
        }

    if (shim) return run_shim(W, H, model_view, projection, wall_clip, &cube[0][0], &faces[0][0], matrices, boxes, N);

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_instanced: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_boxes = nullptr; double* d_matrices = nullptr; std::uint8_t* d_codes = nullptr;
    HIP(hipMalloc((void**)&d_boxes, boxes.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_matrices, matrices.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_codes, size_t(N)));
    HIP(hipMemcpy(d_boxes, boxes.data(), boxes.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_matrices, matrices.data(), matrices.size() * sizeof(double), hipMemcpyHostToDevice));

    CHECK(trgl_draw(ctx, TRGL_SHADER_FLAT, nullptr, wall_clip, nullptr, wall_colors, 2, TRGL_MEM_HOST));
    // the query flushes the wall and runs behind it on the context's stream; the codes stay where the draw will read them
    CHECK(trgl_occlusion_boxes(ctx, view_proj, d_boxes, uint64_t(N), TRGL_MEM_DEVICE, -1, d_codes, TRGL_MEM_DEVICE));

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    CHECK(trgl_draw_instanced(ctx, -1, TRGL_SHADER_PHONG, &u, projection, &cube[0][0], 8, 8, &faces[0][0], 12, nullptr, TRGL_MEM_HOST,
                              d_matrices, 16, uint64_t(N), nullptr, all ? nullptr : d_codes, TRGL_MEM_DEVICE));
    CHECK(trgl_flush(ctx));

    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    CHECK(trgl_read_framebuffer(ctx, px.data()));
    trgl_stats st;
    CHECK(trgl_get_stats(ctx, &st));
    char line[1024];
    CHECK(trgl_format_stats(&st, line, sizeof(line)));
    std::fprintf(stderr, "%s\n", line);
    print_digest(px.data(), px.size(), (unsigned long long)((st.triangles_rasterized - 2) / 12), N);

    (void)hipFree(d_boxes); (void)hipFree(d_matrices); (void)hipFree(d_codes);
    trgl_destroy(ctx);
    return 0;
}
