// demo_glass.cpp — a closed translucent mesh drawn back to front, triangle by triangle, without leaving HBM (include/trgl.h:
// trgl_triangle_depths, trgl_depth_order, trgl_draw_ordered), over the C ABI.
// An opaque FLAT wall, then a glass box (six faces of 4 x 4 quads, 192 triangles; a kind that blends with trgl_blend_over: reads the
// pixel, leaves the depth alone) seen from above one of its edges, so that near and far faces overlap on the screen.  The box is drawn
// three ways:
//   array order      : trgl_vertex_stage, then trgl_draw of its rows as they come
//   sorted triangles : trgl_vertex_stage -> trgl_triangle_depths -> trgl_depth_order -> trgl_draw_ordered, every array in device memory
//   sorted quads     : the same with group = 2: the two triangles of a quad move together, ordered by the quad's farthest vertex
// The second is what a blending renderer means; the first depends on how the mesh happens to be stored.
//   demo_glass [width height] [shim]
// prints a digest of the frame and fragments_drawn per variant; exits with 3 if the sorted frame equals the unsorted one.
// With `shim` the box goes through the shim instead, as opaque FLAT quads in host memory drawn nearest first (gl_triangle_depths,
// gl_depth_order, gl_draw_ordered): the print_render_stats() line (stderr), the first quad drawn and the frame's digest.
// Every number of the scene is written as a literal or is a dyadic fraction, so the scene is the same doubles wherever it is restated
// (tests/test_glass_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_glass: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_glass: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

// takes the 24 varyings of the built-in vertex stage and does not look at them
static const char* kGlassSource = R"(
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
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

// the box through the shim: what a caller of the reference does by sorting its triangles in front of its rasterize() loop
static int run_shim(int W, int H, const double* model_view, const double* projection, const double* wall_clip, const std::vector<double>& vertices,
                    const std::vector<std::uint32_t>& indices) {
    TGAImage fb(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    init_viewport(0, 0, W, H);
    FlatShader flat;
    flat.color = TGAColor(0x50, 0x60, 0x70);
    for (int t = 0; t < 2; ++t) {
        Triangle clip;
        for (int v = 0; v < 3; ++v) clip[v] = make_vec4(wall_clip[12 * t + 4 * v], wall_clip[12 * t + 4 * v + 1], wall_clip[12 * t + 4 * v + 2], wall_clip[12 * t + 4 * v + 3]);
        rasterize(clip, flat, fb);
    }
    // the vertex stage on the host: eye = ModelView * (p, 1), clip = Perspective * eye (main.cpp:71-90)
    const size_t nt = indices.size() / 3;
    std::vector<double> rows(nt * 12);
    for (size_t t = 0; t < nt; ++t)
        for (int v = 0; v < 3; ++v) {
            const double* p = &vertices[size_t(indices[3 * t + v]) * 8];
            double eye[4];
            for (int r = 0; r < 4; ++r) eye[r] = dot4(model_view + 4 * r, p[0], p[1], p[2], 1.0);
            for (int r = 0; r < 4; ++r) rows[12 * t + 4 * v + r] = dot4(projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
        }
    const Triangle* clip = reinterpret_cast<const Triangle*>(rows.data());
    FlatShader box;
    box.color = TGAColor(0x20, 0xa0, 0xc0);
    const std::vector<double> depths = gl_triangle_depths(clip, nt, 2, TRGL_TRI_DEPTH_NEAREST);
    const std::vector<std::uint32_t> order = gl_depth_order(depths, true);
    if (!gl_draw_ordered(clip, nt, box, order, fb, 2) || !gl_flush(fb)) {
        std::fprintf(stderr, "demo_glass: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 2;
    }
    print_render_stats();
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < size_t(W) * H * 3; ++i) { digest ^= fb.buffer()[i]; digest *= 1099511628211ull; }
    std::printf("first drawn: %u\nframe digest: %016llx\n", order.empty() ? 0u : order[0], (unsigned long long)digest);
    gl_shutdown();
    return 0;
}

int main(int argc, char** argv) {
    const bool shim = argc > 1 && std::strcmp(argv[argc - 1], "shim") == 0;
    const int nsize = argc - 1 - (shim ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_glass [width height] [shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_glass: bad size\n"); return 1; }

    // the camera: the box turned about y (cos 0.8, sin 0.6) and tipped about x (cos 0.8, sin 0.6), five units down -z
    const double model_view[16] = { 0.8, 0, 0.6, 0,  0.36, 0.8, -0.48, 0,  -0.48, 0.6, 0.64, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    const double view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };

    // the opaque layer: a wall across the view at z = -4 (view space z = -9), behind the box
    const double wall[4][3] = { { -8, -5, -4 }, { 8, -5, -4 }, { 8, 5, -4 }, { -8, 5, -4 } };
    const int corner[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
    double wall_clip[24];
    for (int t = 0; t < 2; ++t)
        for (int v = 0; v < 3; ++v) {
            const double* p = wall[corner[t][v]];
            double eye[4];
            for (int r = 0; r < 4; ++r) eye[r] = dot4(view + 4 * r, p[0], p[1], p[2], 1.0);
            for (int r = 0; r < 4; ++r) wall_clip[12 * t + 4 * v + r] = dot4(projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
        }
    const std::uint32_t wall_colors[2] = { 0xff506070u, 0xff506070u };

    // the mesh: a box of side 2 about the origin; face f lies across axis f / 2 at +1 (even f) or -1 (odd f) and is cut into C x C quads,
    // each two triangles that follow one another in the index buffer (position, normal, uv per vertex; vertices are not shared
    // between faces)
    const int C = 4, NV = 6 * (C + 1) * (C + 1), NQ = 6 * C * C, NT = 2 * NQ;
    std::vector<double> vertices(size_t(NV) * 8, 0.0);
    std::vector<std::uint32_t> indices(size_t(NT) * 3), colors(NT);
    for (int f = 0; f < 6; ++f) {
        const int axis = f / 2, a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        const double side = (f % 2) ? -1.0 : 1.0;
        for (int j = 0; j <= C; ++j)
            for (int i = 0; i <= C; ++i) {
                double* v = &vertices[size_t((f * (C + 1) + j) * (C + 1) + i) * 8];
                v[axis] = side; v[a1] = -1.0 + 0.5 * i; v[a2] = -1.0 + 0.5 * j;
                v[3 + axis] = side;
                v[6] = 0.25 * i; v[7] = 0.25 * j;
            }
        for (int j = 0; j < C; ++j)
            for (int i = 0; i < C; ++i) {
                const int q = (f * C + j) * C + i;
                const std::uint32_t v00 = std::uint32_t((f * (C + 1) + j) * (C + 1) + i), v10 = v00 + 1, v01 = v00 + (C + 1), v11 = v01 + 1;
                const std::uint32_t tri[6] = { v00, v10, v11, v00, v11, v01 };
                for (int k = 0; k < 6; ++k) indices[size_t(q) * 6 + k] = tri[k];
                // one colour per quad, alphas from 64 to 191
                colors[2 * q] = colors[2 * q + 1] = ((std::uint32_t(q) * 2654435761u) >> 8) | ((64u + std::uint32_t(q * 53) % 128u) << 24);
            }
    }

    if (shim) return run_shim(W, H, model_view, projection, wall_clip, vertices, indices);

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_glass: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    int glass = -1;
    CHECK(trgl_register_shader_ex(ctx, kGlassSource, 24, TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE, &glass));

    double* d_vertices = nullptr; std::uint32_t* d_indices = nullptr; std::uint32_t* d_colors = nullptr;
    double* d_clip = nullptr; double* d_vary = nullptr; double* d_depths = nullptr; std::uint32_t* d_order = nullptr;
    HIP(hipMalloc((void**)&d_vertices, vertices.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_indices, indices.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_colors, colors.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_clip, size_t(NT) * 12 * sizeof(double)));
    HIP(hipMalloc((void**)&d_vary, size_t(NT) * 24 * sizeof(double)));
    HIP(hipMalloc((void**)&d_depths, size_t(NT) * sizeof(double)));
    HIP(hipMalloc((void**)&d_order, size_t(NT) * sizeof(std::uint32_t)));
    HIP(hipMemcpy(d_vertices, vertices.data(), vertices.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_indices, indices.data(), indices.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_colors, colors.data(), colors.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    const std::uint8_t clear[4] = { 48, 32, 24, 255 };

    struct Run { const char* what; std::uint32_t group; int mode; };          // group 0: array order
    const Run runs[3] = { { "array order", 0, 0 }, { "sorted triangles", 1, TRGL_TRI_DEPTH_CENTROID }, { "sorted quads", 2, TRGL_TRI_DEPTH_FARTHEST } };
    unsigned long long digests[3] = { 0, 0, 0 };
    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    for (int r = 0; r < 3; ++r) {
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_reset_stats(ctx));
        CHECK(trgl_draw(ctx, TRGL_SHADER_FLAT, nullptr, wall_clip, nullptr, wall_colors, 2, TRGL_MEM_HOST));
        // the rows of the mesh: made on the context's stream, and they stay in device memory
        CHECK(trgl_vertex_stage(ctx, -1, &u, projection, d_vertices, 8, uint64_t(NV), d_indices, uint64_t(NT), d_clip, d_vary, TRGL_MEM_DEVICE));
        if (runs[r].group == 0) {
            CHECK(trgl_draw(ctx, glass, &u, d_clip, d_vary, d_colors, uint64_t(NT), TRGL_MEM_DEVICE));
        } else {
            // depths, keys, sort and the gather of the rows all run on the context's stream; nothing comes to the host and nothing waits
            const std::uint32_t g = runs[r].group;
            CHECK(trgl_triangle_depths(ctx, d_clip, uint64_t(NT), g, runs[r].mode, TRGL_MEM_DEVICE, d_depths));
            CHECK(trgl_depth_order(ctx, d_depths, uint64_t(NT) / g, TRGL_ORDER_BACK_TO_FRONT, TRGL_MEM_DEVICE, d_order));
            CHECK(trgl_draw_ordered(ctx, glass, &u, d_clip, d_vary, d_colors, uint64_t(NT), TRGL_MEM_DEVICE, d_order, uint64_t(NT) / g, g, TRGL_MEM_DEVICE));
        }
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digests[r] = fnv1a(px);
        std::printf("%s: digest %016llx fragments_drawn %llu\n", runs[r].what, digests[r], (unsigned long long)st.fragments_drawn);
    }

    (void)hipFree(d_vertices); (void)hipFree(d_indices); (void)hipFree(d_colors); (void)hipFree(d_clip); (void)hipFree(d_vary);
    (void)hipFree(d_depths); (void)hipFree(d_order);
    trgl_destroy(ctx);
    if (digests[1] == digests[0]) { std::fprintf(stderr, "demo_glass: the sorted frame equals the unsorted one\n"); return 3; }
    return 0;
}
