// demo_subdivide.cpp — a bent arm skinned as a coarse cage, refined twice by Loop subdivision, shaded with regenerated normals and
// outlined along the refined silhouette.  The cage, both refined meshes, their tables and the outline exist in device memory only
// (include/trgl.h: trgl_subdiv_topology, trgl_subdiv_vertices, trgl_mesh_edges, trgl_mesh_normals, trgl_draw_outline), over the C ABI.
//   1. load time: the rest cage of demo_skinned (13 rings of 4 vertices), joints, weights and the palettes of two poses are uploaded;
//      trgl_mesh_edges + trgl_subdiv_topology on the cage, the same pair on the refined mesh, and trgl_mesh_edges on the twice-refined
//      one for the outline.  Every n_edges is a capacity (3 * n_faces), so no count visits the host and nothing waits.
//   2. per pose: trgl_skin_stage of the 52 cage vertices, trgl_subdiv_vertices twice (smooth = 3: positions by Loop's rule, the rest by
//      midpoints), trgl_mesh_normals on the result - the unreferenced zero records of the capacities have zero normals, which is its
//      cue -, clear, trgl_draw_indexed, trgl_draw_outline, flush, read the frame.
//   demo_subdivide [width height] [shim]
// prints per pose the frame's digest and fragments_drawn; exits with 3 if the two poses gave the same frame.
// With `shim` the second pose goes through the shim instead, one level, from host arrays (gl_skin_stage, gl_mesh_edges,
// gl_subdiv_topology, gl_draw_subdivided); it prints the print_render_stats() line (stderr) and the digest.
// Every number of the scene is an integer, a literal or a quotient of two integers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_subdivide: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_subdivide: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

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

template <class T> static int upload(T** dev, const std::vector<T>& host) {
    if (hipMalloc((void**)dev, host.size() * sizeof(T)) != hipSuccess) return 1;
    return hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
}

int main(int argc, char** argv) {
    const bool shim = argc > 1 && std::strcmp(argv[argc - 1], "shim") == 0;
    const int nsize = argc - 1 - (shim ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_subdivide [width height] [shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_subdivide: bad size\n"); return 1; }

    // the camera of demo_outline: five units down -z; near 1, far 17; the lines' projection is 1/64 nearer in depth
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    const double eye[4] = { 0, 0, 5, 1 };
    const double LINE_BIAS = 1.0 / 64, LINE_WIDTH = 2.0, ZNEAR = 1.0;

    // the arm of demo_skinned: rings at x = -1.5 + r / 4, r = 0 .. 12; corner c of a ring at (y, z) = (+-1/4, +-1/4)
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

    trgl_subdiv_params sub;
    std::memset(&sub, 0, sizeof(sub));
    sub.vertex_stride = S; sub.smooth = 3; sub.mode = TRGL_SUBDIV_LOOP;

    if (shim) {
        TGAImage fb(W, H, TGAImage::RGB);
        init_zbuffer(W, H);
        init_viewport(0, 0, W, H);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
        std::vector<mat<4, 4>> palette(NJ);
        std::memcpy(static_cast<void*>(palette.data()), &palettes[size_t(NJ) * 16], sizeof(double) * 16 * NJ);
        ArmPhong phong;
        phong.uniforms = u;
        const trgl_skin_params sp = gl_skin_params(S, 2, NJ, TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT);
        std::vector<double> skinned;
        std::vector<std::uint32_t> edges, stencils;
        std::vector<unsigned int> refined;
        bool ok = gl_skin_stage(sp, vertices.data(), NV, joints.data(), weights.data(), palette, skinned);
        ok = ok && gl_mesh_edges(indices.data(), NT, NV, edges);
        ok = ok && gl_subdiv_topology(indices.data(), NT, NV, edges, refined, stencils);
        ok = ok && gl_draw_subdivided(phong, gl_subdiv_params(S), skinned.data(), NV, stencils, edges.size() / 4, refined.data(), refined.size() / 3, fb);
        if (!ok || !gl_flush(fb)) {
            std::fprintf(stderr, "demo_subdivide: %s (code %d)\n", gl_last_error_message(), gl_last_error());
            return 2;
        }
        print_render_stats();
        std::printf("frame digest: %016llx\n", fnv1a(fb.buffer(), size_t(W) * H * 3));
        gl_shutdown();
        return 0;
    }

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_subdivide: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_vertices = nullptr; double* d_weights = nullptr; std::uint16_t* d_joints = nullptr; std::uint32_t* d_indices = nullptr;
    double* d_palettes = nullptr;
    if (upload(&d_vertices, vertices) || upload(&d_weights, weights) || upload(&d_joints, joints) || upload(&d_indices, indices) ||
        upload(&d_palettes, palettes)) {
        std::fprintf(stderr, "demo_subdivide: upload failed\n");
        return 2;
    }
    // the three meshes: vertices V[l], faces F[l]; the edge capacity of level l is E[l] = 3 F[l], and V[l + 1] = V[l] + E[l]
    const std::uint64_t V[3] = { std::uint64_t(NV), std::uint64_t(NV) + 3ull * NT, std::uint64_t(NV) + 3ull * NT + 12ull * NT };
    const std::uint64_t F[3] = { std::uint64_t(NT), 4ull * NT, 16ull * NT };
    const std::uint64_t E[3] = { 3 * F[0], 3 * F[1], 3 * F[2] };
    std::uint32_t* d_edges[3] = { nullptr, nullptr, nullptr };
    std::uint32_t* d_index[3] = { d_indices, nullptr, nullptr };
    std::uint32_t* d_stencils[2] = { nullptr, nullptr };
    double* d_mesh[3] = { nullptr, nullptr, nullptr };
    for (int l = 0; l < 3; ++l) {
        HIP(hipMalloc((void**)&d_edges[l], E[l] * 4 * sizeof(std::uint32_t)));
        HIP(hipMalloc((void**)&d_mesh[l], V[l] * S * sizeof(double)));
        if (l) HIP(hipMalloc((void**)&d_index[l], F[l] * 3 * sizeof(std::uint32_t)));
        if (l < 2) HIP(hipMalloc((void**)&d_stencils[l], trgl_subdiv_stencil_words(V[l], E[l]) * sizeof(std::uint32_t)));
    }
    // load time: nothing below waits
    for (int l = 0; l < 3; ++l) {
        CHECK(trgl_mesh_edges(ctx, d_index[l], F[l], V[l], TRGL_MEM_DEVICE, d_edges[l], nullptr));
        if (l < 2) CHECK(trgl_subdiv_topology(ctx, d_index[l], F[l], V[l], d_edges[l], E[l], TRGL_MEM_DEVICE, d_index[l + 1], d_stencils[l]));
    }

    trgl_skin_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.vertex_stride = S; sp.n_influences = 2; sp.n_joints = NJ; sp.flags = TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT;
    sp.n_poses = 1; sp.palette_stride = 0;
    trgl_edge_params ep;
    std::memset(&ep, 0, sizeof(ep));
    std::memcpy(ep.eye, eye, sizeof(eye));
    for (int k = 0; k < 4; ++k) ep.class_color[k] = 0xff000000u;
    ep.crease_cos = -2.0; ep.select = TRGL_EDGE_BOUNDARY | TRGL_EDGE_SILHOUETTE; ep.compact = 1;
    trgl_line_params lp;
    std::memset(&lp, 0, sizeof(lp));
    std::memcpy(lp.model_view, model_view, sizeof(model_view));
    std::memcpy(lp.projection, projection, sizeof(projection));
    lp.projection[11] = projection[11] - LINE_BIAS;
    lp.width = LINE_WIDTH; lp.half_extent[0] = W / 2.0; lp.half_extent[1] = H / 2.0; lp.w_min = ZNEAR;

    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    unsigned long long digests[2] = { 0, 0 };
    const std::uint8_t clear[4] = { 200, 208, 216, 255 };
    for (int q = 0; q < NP; ++q) {
        CHECK(trgl_skin_stage(ctx, &sp, d_vertices, NV, d_joints, d_weights, d_palettes + size_t(q) * NJ * 16, TRGL_MEM_DEVICE, d_mesh[0]));
        for (int l = 0; l < 2; ++l) CHECK(trgl_subdiv_vertices(ctx, &sub, d_mesh[l], V[l], d_stencils[l], E[l], TRGL_MEM_DEVICE, d_mesh[l + 1]));
        CHECK(trgl_mesh_normals(ctx, d_mesh[2], S, V[2], d_index[2], F[2], TRGL_MEM_DEVICE, nullptr));
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_draw_indexed(ctx, TRGL_SHADER_PHONG, &u, projection, d_mesh[2], S, V[2], d_index[2], F[2], TRGL_MEM_DEVICE));
        CHECK(trgl_draw_outline(ctx, TRGL_SHADER_FLAT, nullptr, &lp, &ep, d_mesh[2], S, V[2], d_index[2], F[2], d_edges[2], E[2], TRGL_MEM_DEVICE));
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digests[q] = fnv1a(px.data(), px.size());
        std::printf("pose %d: digest %016llx fragments_drawn %llu vertices %llu faces %llu\n", q, digests[q], (unsigned long long)st.fragments_drawn,
                    (unsigned long long)V[2], (unsigned long long)F[2]);
    }
    (void)hipFree(d_vertices); (void)hipFree(d_weights); (void)hipFree(d_joints); (void)hipFree(d_palettes);
    for (int l = 0; l < 3; ++l) { (void)hipFree(d_edges[l]); (void)hipFree(d_mesh[l]); (void)hipFree(d_index[l]); }
    for (int l = 0; l < 2; ++l) (void)hipFree(d_stencils[l]);
    trgl_destroy(ctx);
    if (digests[0] == digests[1]) { std::fprintf(stderr, "demo_subdivide: the two poses gave the same frame\n"); return 3; }
    return 0;
}
