// demo_sorted.cpp — translucent instances drawn back to front without leaving HBM (include/trgl.h: trgl_instance_depths,
// trgl_depth_order, trgl_draw_instanced_ordered), over the C ABI.
// 192 translucent quads (a kind that blends with trgl_blend_over: reads the pixel, leaves the depth alone) at scattered depths in front
// of an opaque FLAT wall.  Matrices, colours, depths and the order live in device memory.  The frame is drawn twice: the quads in
// array order (trgl_draw_instanced), and through depths, order and the ordered draw - the second is what a blending renderer means.
// Then an OPAQUE kind that discards its fainter fragments draws the same quads in array order, back to front and front to back:
// drawn nearest first, most later fragments fail the depth test and never reach trgl_fragment.
//   demo_sorted [width height] [shim_back | shim_front]
// prints the digests of the two translucent frames and fragments_drawn under the three orders; exits with 3 unless front to back
// drew fewer fragments than back to front.  With `shim_back` / `shim_front` the quads go through the shim instead, as an opaque Phong
// material in host memory (gl_instance_depths, gl_depth_order, gl_draw_instanced_ordered): the print_render_stats() line (stderr) and
// the frame's digest - the frame is the same in both directions, fragments_drawn is not.
// Every number of the scene is a dyadic fraction, so the scene is the same doubles wherever it is restated
// (tests/test_sorted_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_sorted: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_sorted: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

// both kinds take the 24 varyings of the built-in vertex stage and do not look at them
static const char* kGlassSource = R"(
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
)";
static const char* kCutoutSource = R"(
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ (in.color >> 24) < 96u, in.color }; }
)";

// geometry.h:122-127: summed from 0, left to right
static double dot4(const double* m, double x, double y, double z, double w) {
    double s = 0;
    s += m[0] * x; s += m[1] * y; s += m[2] * z; s += m[3] * w;
    return s;
}

static unsigned long long fnv1a(const std::vector<std::uint8_t>& px) {
    std::uint64_t digest = 1469598103934665603ull;
    for (std::uint8_t b : px) { digest ^= b; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

// stands in for the reference's Model where PhongShaderT asks it: a material without maps
struct NoMaps {
    vec3 vert(int, int) const { return vec3(); } vec3 normal(int, int) const { return vec3(); } vec2 uv(int, int) const { return vec2(); }
    int diffuse_slot() const { return -1; } int normal_slot() const { return -1; } int specular_slot() const { return -1; }
};

// the scene through the shim: what a caller of the reference does by sorting its models in front of the loop of main.cpp:647-736
static int run_shim(int W, int H, bool front_to_back, const double* model_view, const double* projection, const double* wall_clip,
                    const double* quad, const std::uint32_t* faces, const std::vector<double>& matrices, int N) {
    TGAImage fb(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    init_viewport(0, 0, W, H);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
    FlatShader flat;
    flat.color = TGAColor(0x50, 0x60, 0x70);
    for (int t = 0; t < 2; ++t) {
        Triangle clip;
        for (int v = 0; v < 3; ++v) clip[v] = make_vec4(wall_clip[12 * t + 4 * v], wall_clip[12 * t + 4 * v + 1], wall_clip[12 * t + 4 * v + 2], wall_clip[12 * t + 4 * v + 3]);
        rasterize(clip, flat, fb);
    }
    std::vector<mat<4, 4>> models(N);
    for (int k = 0; k < N; ++k)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) models[k][r][c] = matrices[16 * size_t(k) + 4 * r + c];
    NoMaps none;
    PhongShaderT<NoMaps> shader(&none);                                        // constructed once, under the view's ModelView
    shader.key_light_dir_eye = shader.fill_light_dir_eye = shader.rim_light_dir_eye = make_vec3(0.0, 0.0, 1.0);
    const std::vector<double> depths = gl_instance_depths(models, make_vec3(0.0, 0.0, 0.0));
    const std::vector<std::uint32_t> order = gl_depth_order(depths, front_to_back);
    if (!gl_draw_instanced_ordered(shader, quad, 8, 4, faces, 2, models, order, fb) || !gl_flush(fb)) {
        std::fprintf(stderr, "demo_sorted: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 2;
    }
    print_render_stats();
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < size_t(W) * H * 3; ++i) { digest ^= fb.buffer()[i]; digest *= 1099511628211ull; }
    std::printf("first drawn: %u\nframe digest: %016llx\n", order.empty() ? 0u : order[0], (unsigned long long)digest);
    gl_shutdown();
    return 0;
}

enum Order { ARRAY = -1, BACK_TO_FRONT = TRGL_ORDER_BACK_TO_FRONT, FRONT_TO_BACK = TRGL_ORDER_FRONT_TO_BACK };

int main(int argc, char** argv) {
    const bool shim_back = argc > 1 && std::strcmp(argv[argc - 1], "shim_back") == 0;
    const bool shim_front = argc > 1 && std::strcmp(argv[argc - 1], "shim_front") == 0;
    const int nsize = argc - 1 - (shim_back || shim_front ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_sorted [width height] [shim_back | shim_front]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_sorted: bad size\n"); return 1; }

    // the camera: five units in front of the origin, looking down -z (visible points have negative view z)
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };

    // the opaque layer: a wall across the view at z = -4, behind every quad
    const double wall[4][3] = { { -8, -5, -4 }, { 8, -5, -4 }, { 8, 5, -4 }, { -8, 5, -4 } };
    const int corner[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
    double wall_clip[24];
    for (int t = 0; t < 2; ++t)
        for (int v = 0; v < 3; ++v) {
            const double* p = wall[corner[t][v]];
            double eye[4];
            for (int r = 0; r < 4; ++r) eye[r] = dot4(model_view + 4 * r, p[0], p[1], p[2], 1.0);
            for (int r = 0; r < 4; ++r) wall_clip[12 * t + 4 * v + r] = dot4(projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
        }
    const std::uint32_t wall_colors[2] = { 0xff506070u, 0xff506070u };

    // the mesh: a quad of side 1 in the plane z = 0 (position, normal, uv), two faces
    const double quad[4][8] = { { -0.5, -0.5, 0, 0, 0, 1, 0, 0 }, { 0.5, -0.5, 0, 0, 0, 1, 1, 0 }, { 0.5, 0.5, 0, 0, 0, 1, 1, 1 }, { -0.5, 0.5, 0, 0, 0, 1, 0, 1 } };
    const std::uint32_t faces[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };

    // the instances: 16 x 12 quads of side 3/4 on a grid that they overlap, each at a depth of its own in [-3, 1) that has nothing to
    // do with its place in the array; colours with alphas from 64 to 191
    const int NX = 16, NY = 12, N = NX * NY;
    std::vector<double> matrices(size_t(N) * 16, 0.0);
    std::vector<std::uint32_t> colors(N);
    for (int k = 0; k < N; ++k) {
        double* m = &matrices[size_t(k) * 16];
        m[0] = m[5] = m[10] = 0.75; m[15] = 1.0;
        m[3] = -2.5 + 0.3125 * (k % NX); m[7] = -1.375 + 0.25 * (k / NX); m[11] = -3.0 + ((k * 37) % 64) / 16.0;
        colors[k] = ((std::uint32_t(k) * 2654435761u) >> 8) | ((64u + std::uint32_t(k * 53) % 128u) << 24);
    }
    if (shim_back || shim_front) return run_shim(W, H, shim_front, model_view, projection, wall_clip, &quad[0][0], &faces[0][0], matrices, N);
    const double origin[3] = { 0, 0, 0 };                                     // the point of the mesh whose depth orders the instances

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_sorted: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    int glass = -1, cutout = -1;
    CHECK(trgl_register_shader_ex(ctx, kGlassSource, 24, TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE, &glass));
    CHECK(trgl_register_shader_ex(ctx, kCutoutSource, 24, TRGL_SHADER_MAY_DISCARD, &cutout));

    double* d_matrices = nullptr; std::uint32_t* d_colors = nullptr; double* d_depths = nullptr; std::uint32_t* d_order = nullptr;
    HIP(hipMalloc((void**)&d_matrices, matrices.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_colors, size_t(N) * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_depths, size_t(N) * sizeof(double)));
    HIP(hipMalloc((void**)&d_order, size_t(N) * sizeof(std::uint32_t)));
    HIP(hipMemcpy(d_matrices, matrices.data(), matrices.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_colors, colors.data(), size_t(N) * sizeof(std::uint32_t), hipMemcpyHostToDevice));

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    const std::uint8_t clear[4] = { 48, 32, 24, 255 };

    struct Run { const char* what; int kind; Order order; };
    const Run runs[5] = { { "translucent, array order", 0, ARRAY }, { "translucent, back to front", 0, BACK_TO_FRONT },
                          { "cutout, array order", 1, ARRAY }, { "cutout, back to front", 1, BACK_TO_FRONT }, { "cutout, front to back", 1, FRONT_TO_BACK } };
    unsigned long long frags[5] = { 0, 0, 0, 0, 0 };
    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    for (int r = 0; r < 5; ++r) {
        const int kind = runs[r].kind == 0 ? glass : cutout;
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_reset_stats(ctx));
        CHECK(trgl_draw(ctx, TRGL_SHADER_FLAT, nullptr, wall_clip, nullptr, wall_colors, 2, TRGL_MEM_HOST));
        if (runs[r].order == ARRAY) {
            CHECK(trgl_draw_instanced(ctx, -1, kind, &u, projection, &quad[0][0], 8, 4, &faces[0][0], 2, nullptr, TRGL_MEM_HOST,
                                      d_matrices, 16, uint64_t(N), d_colors, nullptr, TRGL_MEM_DEVICE));
        } else {
            // depths, keys, sort and the gather of the matrices all run on the context's stream; nothing comes to the host but the
            // count of drawn instances
            CHECK(trgl_instance_depths(ctx, model_view, origin, d_matrices, 16, uint64_t(N), TRGL_MEM_DEVICE, d_depths));
            CHECK(trgl_depth_order(ctx, d_depths, uint64_t(N), int(runs[r].order), TRGL_MEM_DEVICE, d_order));
            CHECK(trgl_draw_instanced_ordered(ctx, -1, kind, &u, projection, &quad[0][0], 8, 4, &faces[0][0], 2, nullptr, TRGL_MEM_HOST,
                                              d_matrices, 16, uint64_t(N), d_colors, nullptr, TRGL_MEM_DEVICE, d_order, uint64_t(N), TRGL_MEM_DEVICE));
        }
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        frags[r] = (unsigned long long)st.fragments_drawn;
        std::printf("%s: digest %016llx fragments_drawn %llu\n", runs[r].what, fnv1a(px), frags[r]);
    }

    (void)hipFree(d_matrices); (void)hipFree(d_colors); (void)hipFree(d_depths); (void)hipFree(d_order);
    trgl_destroy(ctx);
    if (!(frags[4] < frags[3])) { std::fprintf(stderr, "demo_sorted: front to back drew %llu fragments, back to front %llu\n", frags[4], frags[3]); return 3; }
    return 0;
}
