// demo_outline.cpp — a bent arm drawn with PHONG and outlined: black silhouettes and open ends, grey creases.  The mesh, its edge list
// and the selected segments exist in device memory only (include/trgl.h: trgl_mesh_edges, trgl_edge_select, trgl_draw_outline), over
// the C ABI.
//   1. the rest mesh of demo_skinned (a beam along x of 13 rings of 4 vertices), its joints, weights and the palettes of two poses
//      are uploaded once; trgl_skin_stage makes the two skinned meshes, trgl_mesh_edges the edge records - once: they depend on the
//      indices alone - and the call waits for the 8-byte count of edges
//   2. per pose: trgl_edge_select with compaction into device arrays (its count is printed), then clear, trgl_draw_indexed of the
//      skinned mesh, trgl_draw_outline over the same vertices, flush, read the frame
//   demo_outline [width height] [shim]
// prints per pose the frame's digest, fragments_drawn, the number of edges and of selected ones; exits with 3 if the two poses gave
// the same frame or the same selection.
// With `shim` the second pose goes through the shim instead, from host arrays under the globals ModelView / Perspective / Viewport
// (gl_skin_stage, gl_draw_skinned, gl_mesh_edges, gl_draw_outline); it prints the print_render_stats() line (stderr) and the digest.
// The lines lie in the surface they outline, so they are drawn under a projection whose depth row is 1/64 nearer: the caller's bias.
// Every number of the scene is an integer, a literal or a quotient of two integers, so the scene is the same doubles wherever it is
// restated (tests/test_outline_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_outline: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_outline: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long fnv1a(const std::uint8_t* px, size_t n) {
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

// a joint's palette matrix: a turn about z by the angle whose cosine and sine are (c, s) around the point (px, 0, 0)
static void turn_about(double c, double s, double px, double* m) {
    const double v[16] = { c, -s, 0, px - c * px,  s, c, 0, -s * px,  0, 0, 1, 0,  0, 0, 0, 1 };
    std::memcpy(m, v, sizeof(v));
}

struct ArmPhong : IShader {
    trgl_uniforms uniforms{};
    bool describe(trgl_shader_desc& d) const override { d.kind = TRGL_SHADER_PHONG; d.uniforms = uniforms; d.color = 0xffffffffu; d.vertex_kind = -1; return true; }
};
struct LineFlat : IShader {
    bool describe(trgl_shader_desc& d) const override { d.kind = TRGL_SHADER_FLAT; std::memset(&d.uniforms, 0, sizeof(d.uniforms)); d.color = 0xff000000u; d.vertex_kind = -1; return true; }
};

template <class T> static int upload(T** dev, const std::vector<T>& host) {
    if (hipMalloc((void**)dev, host.size() * sizeof(T)) != hipSuccess) return 1;
    return hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
}

int main(int argc, char** argv) {
    const bool shim = argc > 1 && std::strcmp(argv[argc - 1], "shim") == 0;
    const int nsize = argc - 1 - (shim ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_outline [width height] [shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_outline: bad size\n"); return 1; }

    // the camera: five units down -z; near 1, far 17 (demo_particles' projection); the lines' projection is 1/64 nearer in depth
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    const double eye[4] = { 0, 0, 5, 1 };                       // the camera's position in model space
    const double LINE_BIAS = 1.0 / 64, LINE_WIDTH = 2.0, ZNEAR = 1.0, CREASE_COS = 0.5;
    const std::uint32_t class_color[4] = { 0xff000000u, 0xff000000u, 0xff000000u, 0xff808080u };      // ANY, BOUNDARY, SILHOUETTE black; CREASE grey
    const std::uint32_t select = TRGL_EDGE_BOUNDARY | TRGL_EDGE_SILHOUETTE | TRGL_EDGE_CREASE;

    // the arm of demo_skinned: rings at x = -1.5 + r / 4, r = 0 .. 12; corner c of a ring at (y, z) = (+-1/4, +-1/4); bone b begins at
    // ring 4 b; a ring on a joint follows both bones by halves
    const int R = 13, S = 14, NV = 4 * R, NT = 8 * (R - 1), NJ = 3, NP = 2;
    const double cy[4] = { -0.25, 0.25, 0.25, -0.25 }, cz[4] = { -0.25, -0.25, 0.25, 0.25 };
    std::vector<double> vertices(size_t(NV) * S, 0.0), weights(size_t(NV) * 2);
    std::vector<std::uint16_t> joints(size_t(NV) * 2);
    std::vector<std::uint32_t> indices(size_t(NT) * 3);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < 4; ++c) {
            const int i = 4 * r + c, bone = r / 4 > 2 ? 2 : r / 4;
            double* v = &vertices[size_t(i) * S];
            v[0] = -1.5 + r / 4.0; v[1] = cy[c]; v[2] = cz[c];
            v[3] = 0.0; v[4] = cy[c] < 0 ? -0.6 : 0.6; v[5] = cz[c] < 0 ? -0.8 : 0.8;
            v[6] = r / 12.0; v[7] = c / 4.0;
            v[8] = 1.0;
            const bool on_joint = r % 4 == 0 && r > 0 && r < 12;
            joints[size_t(i) * 2] = std::uint16_t(bone); joints[size_t(i) * 2 + 1] = std::uint16_t(bone > 0 ? bone - 1 : 0);
            weights[size_t(i) * 2] = on_joint ? 0.5 : 1.0; weights[size_t(i) * 2 + 1] = on_joint ? 0.5 : 0.0;
        }
    for (int r = 0; r + 1 < R; ++r)
        for (int c = 0; c < 4; ++c) {
            const std::uint32_t a = std::uint32_t(4 * r + c), b = std::uint32_t(4 * r + (c + 1) % 4), a2 = a + 4, b2 = b + 4;
            const std::uint32_t tri[6] = { a, b2, a2, a, b, b2 };      // counter-clockwise from outside
            for (int k = 0; k < 6; ++k) indices[(size_t(r) * 4 + c) * 6 + k] = tri[k];
        }
    // the palettes, written out: pose 0 is the rest pose; pose 1 turns the forearm (joint 1, at x = -0.5) and the hand (joint 2, x = 0.5)
    std::vector<double> palettes(size_t(NP) * NJ * 16);
    for (int j = 0; j < NJ; ++j) turn_about(1.0, 0.0, 0.0, &palettes[size_t(j) * 16]);
    turn_about(1.0, 0.0, 0.0, &palettes[size_t(NJ) * 16]);
    turn_about(0.8, 0.6, -0.5, &palettes[size_t(NJ + 1) * 16]);
    turn_about(0.8, 0.6, -0.5, &palettes[size_t(NJ + 2) * 16]);

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;

    trgl_edge_params ep;
    std::memset(&ep, 0, sizeof(ep));
    std::memcpy(ep.eye, eye, sizeof(eye));
    std::memcpy(ep.class_color, class_color, sizeof(class_color));
    ep.crease_cos = CREASE_COS; ep.select = select; ep.compact = 1;

    if (shim) {
        TGAImage fb(W, H, TGAImage::RGB);
        init_zbuffer(W, H);
        init_viewport(0, 0, W, H);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
        std::vector<mat<4, 4>> palette(NJ);
        std::memcpy(static_cast<void*>(palette.data()), &palettes[size_t(NJ) * 16], sizeof(double) * 16 * NJ);
        ArmPhong phong;
        phong.uniforms = u;
        LineFlat flat;
        const trgl_skin_params sp = gl_skin_params(S, 2, NJ, TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT);
        std::vector<double> skinned;
        std::vector<std::uint32_t> edges;
        bool ok = gl_skin_stage(sp, vertices.data(), NV, joints.data(), weights.data(), palette, skinned);
        ok = ok && gl_mesh_edges(indices.data(), NT, NV, edges);
        ok = ok && gl_draw_skinned(phong, sp, vertices.data(), NV, joints.data(), weights.data(), palette, indices.data(), NT, fb);
        Perspective[2][3] = projection[11] - LINE_BIAS;
        ok = ok && gl_draw_outline(gl_edge_params(eye, CREASE_COS, select, class_color), LINE_WIDTH, ZNEAR, skinned.data(), S, NV, indices.data(), NT, edges,
                                   flat, fb);
        if (!ok || !gl_flush(fb)) {
            std::fprintf(stderr, "demo_outline: %s (code %d)\n", gl_last_error_message(), gl_last_error());
            return 2;
        }
        print_render_stats();
        std::printf("frame digest: %016llx\n", fnv1a(fb.buffer(), size_t(W) * H * 3));
        gl_shutdown();
        return 0;
    }

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_outline: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_vertices = nullptr; double* d_weights = nullptr; std::uint16_t* d_joints = nullptr; std::uint32_t* d_indices = nullptr;
    double* d_palettes = nullptr; double* d_skinned = nullptr;
    std::uint32_t* d_edges = nullptr; std::uint32_t* d_segments = nullptr; std::uint32_t* d_colors = nullptr;
    if (upload(&d_vertices, vertices) || upload(&d_weights, weights) || upload(&d_joints, joints) || upload(&d_indices, indices) ||
        upload(&d_palettes, palettes)) {
        std::fprintf(stderr, "demo_outline: upload failed\n");
        return 2;
    }
    HIP(hipMalloc((void**)&d_skinned, size_t(NP) * NV * S * sizeof(double)));
    HIP(hipMalloc((void**)&d_edges, size_t(3) * NT * 4 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_segments, size_t(3) * NT * 2 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_colors, size_t(3) * NT * sizeof(std::uint32_t)));

    // load time: the two skinned meshes and the edge records; the one wait is for the count of edges
    trgl_skin_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.vertex_stride = S; sp.n_influences = 2; sp.n_joints = NJ; sp.flags = TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT;
    sp.n_poses = NP; sp.palette_stride = 16 * NJ;
    CHECK(trgl_skin_stage(ctx, &sp, d_vertices, NV, d_joints, d_weights, d_palettes, TRGL_MEM_DEVICE, d_skinned));
    std::uint64_t n_edges = 0;
    CHECK(trgl_mesh_edges(ctx, d_indices, NT, NV, TRGL_MEM_DEVICE, d_edges, &n_edges));

    trgl_line_params lp;
    std::memset(&lp, 0, sizeof(lp));
    std::memcpy(lp.model_view, model_view, sizeof(model_view));
    std::memcpy(lp.projection, projection, sizeof(projection));
    lp.projection[11] = projection[11] - LINE_BIAS;
    lp.width = LINE_WIDTH; lp.half_extent[0] = W / 2.0; lp.half_extent[1] = H / 2.0; lp.w_min = ZNEAR;

    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    unsigned long long digests[2] = { 0, 0 };
    std::uint64_t selected[2] = { 0, 0 };
    const std::uint8_t clear[4] = { 200, 208, 216, 255 };
    for (int q = 0; q < NP; ++q) {
        const double* pose = d_skinned + size_t(q) * NV * S;
        // the selection alone, as a caller keeps it for draws of its own (trgl_draw_lines over d_segments / d_colors)
        CHECK(trgl_edge_select(ctx, &ep, pose, S, NV, d_indices, NT, d_edges, n_edges, TRGL_MEM_DEVICE, nullptr, d_segments, d_colors, &selected[q]));
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_draw_indexed(ctx, TRGL_SHADER_PHONG, &u, projection, pose, S, NV, d_indices, NT, TRGL_MEM_DEVICE));
        CHECK(trgl_draw_outline(ctx, TRGL_SHADER_FLAT, nullptr, &lp, &ep, pose, S, NV, d_indices, NT, d_edges, n_edges, TRGL_MEM_DEVICE));
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digests[q] = fnv1a(px.data(), px.size());
        std::printf("pose %d: digest %016llx fragments_drawn %llu edges %llu selected %llu\n", q, digests[q], (unsigned long long)st.fragments_drawn,
                    (unsigned long long)n_edges, (unsigned long long)selected[q]);
    }
    (void)hipFree(d_vertices); (void)hipFree(d_weights); (void)hipFree(d_joints); (void)hipFree(d_indices); (void)hipFree(d_palettes);
    (void)hipFree(d_skinned); (void)hipFree(d_edges); (void)hipFree(d_segments); (void)hipFree(d_colors);
    trgl_destroy(ctx);
    if (digests[0] == digests[1] || selected[0] == selected[1]) { std::fprintf(stderr, "demo_outline: the two poses gave the same outline\n"); return 3; }
    return 0;
}
