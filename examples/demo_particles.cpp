// demo_particles.cpp — a cloud of textured, blended particles around an opaque box, and the box's wireframe on top; the particles'
// positions exist in device memory only (include/trgl.h: trgl_sprite_stage, trgl_draw_lines), over the C ABI.
//   1. the box: trgl_vertex_stage over its indexed mesh, drawn FLAT and opaque
//   2. 4096 particles, each a row (x, y, z, size) in HBM: trgl_sprite_stage -> trgl_triangle_depths (group 2: a quad's two triangles move
//      together) -> trgl_depth_order -> trgl_draw_ordered with a kind that samples a round blob at the quad's uv, multiplies the
//      particle's alpha with the texel's and blends with trgl_blend_over.  Every array stays on the device and nothing waits.
//   3. the edges of the box's triangles as lines 1.5 pixels wide: trgl_draw_lines over the mesh's own vertex and index buffers, with a
//      view matrix 1/64 nearer so that they win the depth test against the faces they lie on
//   demo_particles [width height] [shim]
// prints a digest of the frame and fragments_drawn after each step; exits with 3 if a step left the frame as it was.
// With `shim` the scene goes through the shim instead, from host arrays under the globals ModelView / Perspective / Viewport: the box by
// rasterize(), the first 512 particles as opaque FLAT squares 6 pixels wide (gl_draw_sprites), the wireframe by gl_draw_lines; it prints
// the print_render_stats() line (stderr) and the frame's digest.
// Every number of the scene is an integer, a literal or a dyadic fraction, so the scene is the same doubles wherever it is restated
// (tests/test_particles_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_particles: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_particles: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

// K = 6: the three (u, v) pairs of the quad's vertices.  The blob's alpha scales the particle's; an empty fragment is discarded.
static const char* kParticleSource = R"(
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (v[0] * in.bar[0] + v[2] * in.bar[1]) + v[4] * in.bar[2], (v[1] * in.bar[0] + v[3] * in.bar[1]) + v[5] * in.bar[2] };
    const uint32_t texel = trgl_sample2D(in, in.u->tex_diffuse, uv).bgra;
    const uint32_t a = ((texel >> 24) * (in.color >> 24) + 127u) / 255u;
    return trgl_frag_out{ a == 0u, trgl_blend_over((in.color & 0x00ffffffu) | (a << 24), in.dst) };
}
)";

static unsigned long long fnv1a(const std::vector<std::uint8_t>& px) {
    std::uint64_t digest = 1469598103934665603ull;
    for (std::uint8_t b : px) { digest ^= b; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

// geometry.h:122-127: summed from 0, left to right
static double dot4(const double* m, double x, double y, double z, double w) {
    double s = 0;
    s += m[0] * x; s += m[1] * y; s += m[2] * z; s += m[3] * w;
    return s;
}

// the scene through the shim: what a caller of the reference would do with a quad builder in front of its rasterize() loop
static int run_shim(int W, int H, const double* model_view, const double* projection, const std::vector<double>& vertices,
                    const std::vector<std::uint32_t>& indices, const std::vector<std::uint32_t>& edges, const std::vector<double>& particles,
                    const std::vector<std::uint32_t>& particle_colors) {
    TGAImage fb(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    init_viewport(0, 0, W, H);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
    FlatShader flat;
    flat.color = TGAColor(0x50, 0x60, 0x70);
    for (size_t t = 0; t < indices.size() / 3; ++t) {
        Triangle clip;
        for (int v = 0; v < 3; ++v) {
            const double* p = &vertices[size_t(indices[3 * t + v]) * 8];
            double eye[4], c[4];
            for (int r = 0; r < 4; ++r) eye[r] = dot4(model_view + 4 * r, p[0], p[1], p[2], 1.0);
            for (int r = 0; r < 4; ++r) c[r] = dot4(projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
            clip[v] = make_vec4(c[0], c[1], c[2], c[3]);
        }
        rasterize(clip, flat, fb);
    }
    bool ok = gl_draw_sprites(gl_sprite_params(6.0, TRGL_SPRITE_SCREEN), particles.data(), 4, 512, particle_colors.data(), flat, fb);
    ModelView[2][3] = -5.0 + 0.015625;
    FlatShader white;
    white.color = TGAColor(255, 255, 255);
    ok = gl_draw_lines(gl_line_params(1.5, 1.0), vertices.data(), 8, vertices.size() / 8, edges.data(), edges.size() / 2, nullptr, white, fb) && ok;
    if (!ok || !gl_flush(fb)) {
        std::fprintf(stderr, "demo_particles: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 2;
    }
    print_render_stats();
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < size_t(W) * H * 3; ++i) { digest ^= fb.buffer()[i]; digest *= 1099511628211ull; }
    std::printf("frame digest: %016llx\n", (unsigned long long)digest);
    gl_shutdown();
    return 0;
}

int main(int argc, char** argv) {
    const bool shim = argc > 1 && std::strcmp(argv[argc - 1], "shim") == 0;
    const int nsize = argc - 1 - (shim ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_particles [width height] [shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_particles: bad size\n"); return 1; }

    // the camera of demo_glass: the scene turned about y and tipped about x (cos 0.8, sin 0.6), five units down -z; near 1, far 17
    const double model_view[16] = { 0.8, 0, 0.6, 0,  0.36, 0.8, -0.48, 0,  -0.48, 0.6, 0.64, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };

    // the box: side 2 about the origin, each face C x C quads of two triangles (position, normal, uv per vertex)
    const int C = 2, NV = 6 * (C + 1) * (C + 1), NQ = 6 * C * C, NT = 2 * NQ;
    std::vector<double> vertices(size_t(NV) * 8, 0.0);
    std::vector<std::uint32_t> indices(size_t(NT) * 3), colors(NT), edges(size_t(NT) * 6), edge_colors(size_t(NT) * 3, 0xffffffffu);
    for (int f = 0; f < 6; ++f) {
        const int axis = f / 2, a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        const double side = (f % 2) ? -1.0 : 1.0;
        for (int j = 0; j <= C; ++j)
            for (int i = 0; i <= C; ++i) {
                double* v = &vertices[size_t((f * (C + 1) + j) * (C + 1) + i) * 8];
                // (the odd faces run the other way round, so that every face is counter-clockwise from outside)
                v[axis] = side; v[a1] = side * (-1.0 + 1.0 * i); v[a2] = -1.0 + 1.0 * j;
                v[3 + axis] = side;
                v[6] = 0.5 * i; v[7] = 0.5 * j;
            }
        for (int j = 0; j < C; ++j)
            for (int i = 0; i < C; ++i) {
                const int q = (f * C + j) * C + i;
                const std::uint32_t v00 = std::uint32_t((f * (C + 1) + j) * (C + 1) + i), v10 = v00 + 1, v01 = v00 + (C + 1), v11 = v01 + 1;
                const std::uint32_t tri[6] = { v00, v10, v11, v00, v11, v01 };
                for (int k = 0; k < 6; ++k) indices[size_t(q) * 6 + k] = tri[k];
                colors[2 * q] = colors[2 * q + 1] = 0xff000000u | (0x303030u + std::uint32_t(f) * 0x180c06u);
            }
    }
    for (int t = 0; t < NT; ++t)
        for (int e = 0; e < 3; ++e) { edges[size_t(t) * 6 + 2 * e] = indices[size_t(t) * 3 + e]; edges[size_t(t) * 6 + 2 * e + 1] = indices[size_t(t) * 3 + (e + 1) % 3]; }

    // the particles: x, y, z in [-2, 2) and a size in [1/16, 5/16) eye-space units, from a 32-bit LCG; alphas 96 .. 223
    const int NP = 4096;
    std::vector<double> particles(size_t(NP) * 4);
    std::vector<std::uint32_t> particle_colors(NP);
    std::uint32_t s = 12345u;
    auto next = [&s]() { s = s * 1664525u + 1013904223u; return s >> 8; };      // 24 bits
    for (int i = 0; i < NP; ++i) {
        for (int c = 0; c < 3; ++c) particles[size_t(i) * 4 + c] = double(next()) / 4194304.0 - 2.0;
        particles[size_t(i) * 4 + 3] = 0.0625 + double(next()) / 67108864.0;
        const std::uint32_t bgr = next() & 0x00ffffffu, alpha = 96u + (next() & 127u);
        particle_colors[i] = bgr | (alpha << 24);
    }
    // a round blob, 32 x 32 BGRA: white, alpha falling with the squared distance from the centre
    const int TS = 32;
    std::vector<std::uint8_t> blob(size_t(TS) * TS * 4, 255);
    for (int y = 0; y < TS; ++y)
        for (int x = 0; x < TS; ++x) {
            const int dx = 2 * x + 1 - TS, dy = 2 * y + 1 - TS, d2 = dx * dx + dy * dy;      // 0 .. 2 * 31^2
            blob[(size_t(y) * TS + x) * 4 + 3] = std::uint8_t(d2 >= 961 ? 0 : 255 - (255 * d2) / 961);
        }

    if (shim) return run_shim(W, H, model_view, projection, vertices, indices, edges, particles, particle_colors);

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_particles: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    CHECK(trgl_upload_texture(ctx, 0, blob.data(), TS, TS, 4));
    int particle_kind = -1;
    CHECK(trgl_register_shader_ex(ctx, kParticleSource, 6, TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE, &particle_kind));

    double* d_vertices = nullptr; std::uint32_t* d_indices = nullptr; std::uint32_t* d_colors = nullptr; std::uint32_t* d_edges = nullptr;
    std::uint32_t* d_edge_colors = nullptr; double* d_clip = nullptr; double* d_vary = nullptr;
    double* d_particles = nullptr; std::uint32_t* d_particle_colors = nullptr;
    double* d_quad_clip = nullptr; double* d_quad_vary = nullptr; std::uint32_t* d_quad_colors = nullptr; double* d_depths = nullptr; std::uint32_t* d_order = nullptr;
    HIP(hipMalloc((void**)&d_vertices, vertices.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_indices, indices.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_colors, colors.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_edges, edges.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_edge_colors, edge_colors.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_clip, size_t(NT) * 12 * sizeof(double)));
    HIP(hipMalloc((void**)&d_vary, size_t(NT) * 24 * sizeof(double)));
    HIP(hipMalloc((void**)&d_particles, particles.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_particle_colors, particle_colors.size() * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_quad_clip, size_t(NP) * 2 * 12 * sizeof(double)));
    HIP(hipMalloc((void**)&d_quad_vary, size_t(NP) * 2 * 6 * sizeof(double)));
    HIP(hipMalloc((void**)&d_quad_colors, size_t(NP) * 2 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_depths, size_t(NP) * sizeof(double)));
    HIP(hipMalloc((void**)&d_order, size_t(NP) * sizeof(std::uint32_t)));
    HIP(hipMemcpy(d_vertices, vertices.data(), vertices.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_indices, indices.data(), indices.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_colors, colors.data(), colors.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_edges, edges.data(), edges.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_edge_colors, edge_colors.data(), edge_colors.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    // (a simulation step would leave these here; from now on the host has no copy)
    HIP(hipMemcpy(d_particles, particles.data(), particles.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_particle_colors, particle_colors.data(), particle_colors.size() * sizeof(std::uint32_t), hipMemcpyHostToDevice));
    std::vector<double>().swap(particles);

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.tex_diffuse = 0; u.tex_normal = u.tex_specular = -1;
    const std::uint8_t clear[4] = { 48, 32, 24, 255 };
    CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));

    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    unsigned long long digests[3] = { 0, 0, 0 };
    const char* steps[3] = { "box", "particles", "wireframe" };
    for (int step = 0; step < 3; ++step) {
        if (step == 0) {
            CHECK(trgl_vertex_stage(ctx, -1, &u, projection, d_vertices, 8, uint64_t(NV), d_indices, uint64_t(NT), d_clip, d_vary, TRGL_MEM_DEVICE));
            CHECK(trgl_draw(ctx, TRGL_SHADER_FLAT, nullptr, d_clip, nullptr, d_colors, uint64_t(NT), TRGL_MEM_DEVICE));
        } else if (step == 1) {
            trgl_sprite_params sp;
            std::memset(&sp, 0, sizeof(sp));
            std::memcpy(sp.model_view, model_view, sizeof(model_view));
            std::memcpy(sp.projection, projection, sizeof(projection));
            sp.mode = TRGL_SPRITE_VIEW; sp.size_offset = 3;
            // quads, their depths, the order and the gather of the rows all run on the context's stream
            CHECK(trgl_sprite_stage(ctx, &sp, d_particles, 4, d_particle_colors, uint64_t(NP), TRGL_MEM_DEVICE, d_quad_clip, d_quad_vary, d_quad_colors));
            CHECK(trgl_triangle_depths(ctx, d_quad_clip, uint64_t(NP) * 2, 2, TRGL_TRI_DEPTH_CENTROID, TRGL_MEM_DEVICE, d_depths));
            CHECK(trgl_depth_order(ctx, d_depths, uint64_t(NP), TRGL_ORDER_BACK_TO_FRONT, TRGL_MEM_DEVICE, d_order));
            CHECK(trgl_draw_ordered(ctx, particle_kind, &u, d_quad_clip, d_quad_vary, d_quad_colors, uint64_t(NP) * 2, TRGL_MEM_DEVICE,
                                    d_order, uint64_t(NP), 2, TRGL_MEM_DEVICE));
        } else {
            trgl_line_params lp;
            std::memset(&lp, 0, sizeof(lp));
            std::memcpy(lp.model_view, model_view, sizeof(model_view));
            std::memcpy(lp.projection, projection, sizeof(projection));
            lp.model_view[11] = -5.0 + 0.015625;
            lp.width = 1.5; lp.half_extent[0] = 0.5 * W; lp.half_extent[1] = 0.5 * H; lp.w_min = 1.0;
            CHECK(trgl_draw_lines(ctx, TRGL_SHADER_FLAT, nullptr, &lp, d_vertices, 8, uint64_t(NV), d_edges, d_edge_colors, uint64_t(NT) * 3, TRGL_MEM_DEVICE));
        }
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digests[step] = fnv1a(px);
        std::printf("%s: digest %016llx fragments_drawn %llu\n", steps[step], digests[step], (unsigned long long)st.fragments_drawn);
    }

    (void)hipFree(d_vertices); (void)hipFree(d_indices); (void)hipFree(d_colors); (void)hipFree(d_edges); (void)hipFree(d_edge_colors);
    (void)hipFree(d_clip); (void)hipFree(d_vary); (void)hipFree(d_particles); (void)hipFree(d_particle_colors);
    (void)hipFree(d_quad_clip); (void)hipFree(d_quad_vary); (void)hipFree(d_quad_colors); (void)hipFree(d_depths); (void)hipFree(d_order);
    trgl_destroy(ctx);
    if (digests[1] == digests[0] || digests[2] == digests[1]) { std::fprintf(stderr, "demo_particles: a step left the frame as it was\n"); return 3; }
    return 0;
}
