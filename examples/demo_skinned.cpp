// demo_skinned.cpp — an arm of three bones bent under three poses and drawn with PHONG; neither the palettes nor the skinned
// vertices ever exist in host memory (include/trgl.h: trgl_pose_palette, trgl_skin_stage, trgl_draw_skinned), over the C ABI.
//   1. the rest mesh (a beam along x of 13 rings of 4 vertices, 14 doubles per vertex), its joint numbers and weights, the hierarchy,
//      the inverse bind matrices and the local joint matrices of three poses are uploaded once
//   2. trgl_pose_palette composes the three palettes on the device; trgl_skin_stage makes the three skinned meshes from them in one
//      call; trgl_mesh_bounds reduces each on the device (what a caller feeds to its frustum test)
//   3. per pose: clear, trgl_draw_skinned under that pose's palette, flush, read the frame
//   demo_skinned [width height] [shim]
// prints per pose the frame's digest, fragments_drawn and the bounds; exits with 3 if two poses gave the same frame.
// With `shim` the last pose goes through the shim instead, from host arrays under the globals ModelView / Perspective / Viewport
// (gl_pose_palette, gl_draw_skinned); it prints the print_render_stats() line (stderr) and the frame's digest.
// Every number of the scene is an integer, a literal or a quotient of two integers, so the scene is the same doubles wherever it is
// restated (tests/test_skinned_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_skinned: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_skinned: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long fnv1a(const std::uint8_t* px, size_t n) {
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

// a joint's local matrix: a turn about z by the angle whose cosine and sine are (c, s), then a step of tx along the parent's x
static void joint_matrix(double c, double s, double tx, double* m) {
    const double v[16] = { c, -s, 0, tx,  s, c, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
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
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_skinned [width height] [shim]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 320, H = nsize ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_skinned: bad size\n"); return 1; }

    // the camera: five units down -z; near 1, far 17 (demo_particles' projection)
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };

    // the arm: rings at x = -1.5 + r / 4, r = 0 .. 12; corner c of a ring at (y, z) = (+-1/4, +-1/4), counter-clockwise seen from +x;
    // bone b begins at ring 4 b; a ring on a joint follows both bones by halves
    const int R = 13, S = 14, NV = 4 * R, NT = 8 * (R - 1), NJ = 3, NP = 3;
    const double cy[4] = { -0.25, 0.25, 0.25, -0.25 }, cz[4] = { -0.25, -0.25, 0.25, 0.25 };
    std::vector<double> vertices(size_t(NV) * S, 0.0), weights(size_t(NV) * 2);
    std::vector<std::uint16_t> joints(size_t(NV) * 2);
    std::vector<std::uint32_t> indices(size_t(NT) * 3);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < 4; ++c) {
            const int i = 4 * r + c, bone = r / 4 > 2 ? 2 : r / 4;
            double* v = &vertices[size_t(i) * S];
            v[0] = -1.5 + r / 4.0; v[1] = cy[c]; v[2] = cz[c];
            v[3] = 0.0; v[4] = cy[c] < 0 ? -0.6 : 0.6; v[5] = cz[c] < 0 ? -0.8 : 0.8;      // a unit normal away from the axis
            v[6] = r / 12.0; v[7] = c / 4.0;
            v[8] = 1.0;                                                                       // the tangent along the bone
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
    // joints at x = -1.5, -0.5, 0.5 in the rest pose; pose 0 is the rest pose, pose 1 bends the elbow, pose 2 the elbow and the wrist
    const std::vector<std::int32_t> parents = { -1, 0, 1 };
    std::vector<double> inverse_bind(size_t(NJ) * 16), local(size_t(NP) * NJ * 16);
    for (int j = 0; j < NJ; ++j) joint_matrix(1.0, 0.0, 1.5 - j, &inverse_bind[size_t(j) * 16]);
    const double bend[3][3][2] = { { { 1, 0 }, { 1, 0 }, { 1, 0 } }, { { 1, 0 }, { 0.8, 0.6 }, { 1, 0 } }, { { 0.96, -0.28 }, { 0.6, 0.8 }, { 0.8, -0.6 } } };
    for (int q = 0; q < NP; ++q)
        for (int j = 0; j < NJ; ++j) joint_matrix(bend[q][j][0], bend[q][j][1], j == 0 ? -1.5 : 1.0, &local[(size_t(q) * NJ + j) * 16]);

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;

    if (shim) {
        TGAImage fb(W, H, TGAImage::RGB);
        init_zbuffer(W, H);
        init_viewport(0, 0, W, H);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { ModelView[r][c] = model_view[4 * r + c]; Perspective[r][c] = projection[4 * r + c]; }
        std::vector<mat<4, 4>> ib(NJ), loc(NJ), palette;
        std::memcpy(static_cast<void*>(ib.data()), inverse_bind.data(), sizeof(double) * 16 * NJ);
        std::memcpy(static_cast<void*>(loc.data()), &local[size_t(2) * NJ * 16], sizeof(double) * 16 * NJ);
        ArmPhong phong;
        phong.uniforms = u;
        bool ok = gl_pose_palette(parents, ib, loc, palette);
        ok = ok && gl_draw_skinned(phong, gl_skin_params(S, 2, NJ, TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT), vertices.data(), NV, joints.data(), weights.data(),
                                   palette, indices.data(), NT, fb);
        if (!ok || !gl_flush(fb)) {
            std::fprintf(stderr, "demo_skinned: %s (code %d)\n", gl_last_error_message(), gl_last_error());
            return 2;
        }
        print_render_stats();
        std::printf("frame digest: %016llx\n", fnv1a(fb.buffer(), size_t(W) * H * 3));
        gl_shutdown();
        return 0;
    }

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_skinned: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_vertices = nullptr; double* d_weights = nullptr; std::uint16_t* d_joints = nullptr; std::uint32_t* d_indices = nullptr;
    std::int32_t* d_parents = nullptr; double* d_inverse_bind = nullptr; double* d_local = nullptr; double* d_palettes = nullptr; double* d_skinned = nullptr;
    if (upload(&d_vertices, vertices) || upload(&d_weights, weights) || upload(&d_joints, joints) || upload(&d_indices, indices) ||
        upload(&d_parents, parents) || upload(&d_inverse_bind, inverse_bind) || upload(&d_local, local)) {
        std::fprintf(stderr, "demo_skinned: upload failed\n");
        return 2;
    }
    HIP(hipMalloc((void**)&d_palettes, size_t(NP) * NJ * 16 * sizeof(double)));
    HIP(hipMalloc((void**)&d_skinned, size_t(NP) * NV * S * sizeof(double)));

    // the palettes and the three skinned meshes: two launches on the context's stream, nothing waits
    CHECK(trgl_pose_palette(ctx, d_parents, d_inverse_bind, NJ, d_local, 16 * NJ, NP, TRGL_MEM_DEVICE, d_palettes, 16 * NJ));
    trgl_skin_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.vertex_stride = S; sp.n_influences = 2; sp.n_joints = NJ; sp.flags = TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT;
    sp.n_poses = NP; sp.palette_stride = 16 * NJ;
    CHECK(trgl_skin_stage(ctx, &sp, d_vertices, NV, d_joints, d_weights, d_palettes, TRGL_MEM_DEVICE, d_skinned));

    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    unsigned long long digests[3] = { 0, 0, 0 };
    const std::uint8_t clear[4] = { 24, 24, 32, 255 };
    sp.n_poses = 1; sp.palette_stride = 0;
    for (int q = 0; q < NP; ++q) {
        double lo[3], hi[3];
        CHECK(trgl_mesh_bounds(ctx, d_skinned + size_t(q) * NV * S, S, NV, TRGL_MEM_DEVICE, lo, hi));
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_draw_skinned(ctx, -1, TRGL_SHADER_PHONG, &u, projection, &sp, d_vertices, NV, d_joints, d_weights, d_palettes + size_t(q) * NJ * 16,
                                d_indices, NT, nullptr, TRGL_MEM_DEVICE));
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digests[q] = fnv1a(px.data(), px.size());
        std::printf("pose %d: digest %016llx fragments_drawn %llu bounds %.17g %.17g %.17g %.17g %.17g %.17g\n", q, digests[q],
                    (unsigned long long)st.fragments_drawn, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    }
    (void)hipFree(d_vertices); (void)hipFree(d_weights); (void)hipFree(d_joints); (void)hipFree(d_indices); (void)hipFree(d_parents);
    (void)hipFree(d_inverse_bind); (void)hipFree(d_local); (void)hipFree(d_palettes); (void)hipFree(d_skinned);
    trgl_destroy(ctx);
    if (digests[0] == digests[1] || digests[1] == digests[2]) { std::fprintf(stderr, "demo_skinned: two poses gave the same frame\n"); return 3; }
    return 0;
}
