// demo_instance_cull.cpp — a crowd culled and drawn from an array of matrices in HBM, over the C ABI (include/trgl.h):
//   1. trgl_mesh_bounds              the mesh's local box (Model::computeAABB)
//   2. trgl_instance_boxes           a world box per instance (Model::getWorldAABB), device memory
//   3. trgl_occlusion_boxes          a code byte per box against the depths drawn so far, device memory
//   4. trgl_frustum_boxes(MERGE)     the reference's own test, frustum.intersects(worldAABB), merged into those bytes
//   5. trgl_instance_depths          the view-space depth of every instance
//   6. trgl_depth_order              nearest first
//   7. trgl_draw_instanced_ordered   the draw, gated by the bytes
// The matrices are uploaded once; boxes, codes, depths and the order are made where they are and never exist in host memory.  What comes
// back is the 8-byte count of drawn instances inside the draw, and the frame.
// 272 cubes on a grid that reaches past both sides of the view, half of it behind a wall, and a row of cubes behind the eye.  The frame is
// drawn three times, under the same order: every instance, the instances occlusion leaves, and those occlusion and the frustum leave.
// A culled instance has no fragment to give, so the three frames and their fragments_drawn are equal - the demo exits with 3 if not -
// and the triangle counter tells how many instances each test removed.
//   demo_instance_cull [width height]
// Every number of the scene is a dyadic fraction, so the scene is the same doubles wherever it is restated
// (tests/test_instance_cull_demo_gpu.py draws it through the Python binding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/trgl.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_instance_cull: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_instance_cull: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

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

enum Cull { NONE = 0, OCCLUSION = 1, OCCLUSION_AND_FRUSTUM = 2 };

int main(int argc, char** argv) {
    if (argc != 1 && argc != 3) { std::fprintf(stderr, "usage: demo_instance_cull [width height]\n"); return 1; }
    const int W = argc == 3 ? std::atoi(argv[1]) : 320, H = argc == 3 ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_instance_cull: bad size\n"); return 1; }

    // the camera: five units in front of the origin, looking down -z
    const double model_view[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    double view_proj[16], view_proj_t[16], planes[24];
    for (int r = 0; r < 4; ++r)                                               // Perspective * ModelView (main.cpp:623), geometry.h:196-205
        for (int c = 0; c < 4; ++c)
            view_proj[4 * r + c] = dot4(projection + 4 * r, model_view[c], model_view[4 + c], model_view[8 + c], model_view[12 + c]);
    // Frustum::createFromMatrix reads m[r][3] +- m[r][k] (our_gl.cpp:217-250): the camera's six planes when it is handed the transpose
    // of a matrix that multiplies column vectors
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) view_proj_t[4 * r + c] = view_proj[4 * c + r];
    if (trgl_frustum_from_matrix(view_proj_t, planes) != TRGL_OK) return 2;

    // the occluder: a wall over the left half of the view at z = -1, in front of the grid
    const double wall[4][3] = { { -8, -5, -1 }, { 0, -5, -1 }, { 0, 5, -1 }, { -8, 5, -1 } };
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

    // the mesh: a cube of side 1 (position, outward normal / 2, uv), 12 faces
    double cube[8][8];
    for (int v = 0; v < 8; ++v) {
        const double p[3] = { (v & 1) ? 0.5 : -0.5, (v & 2) ? 0.5 : -0.5, (v & 4) ? 0.5 : -0.5 };
        for (int a = 0; a < 3; ++a) { cube[v][a] = p[a]; cube[v][3 + a] = p[a]; }
        cube[v][6] = p[0] + 0.5; cube[v][7] = p[1] + 0.5;
    }
    const std::uint32_t faces[12][3] = { { 0, 2, 1 }, { 1, 2, 3 }, { 4, 5, 6 }, { 5, 7, 6 }, { 0, 1, 4 }, { 1, 5, 4 },
                                         { 2, 6, 3 }, { 3, 6, 7 }, { 0, 4, 2 }, { 2, 4, 6 }, { 1, 3, 5 }, { 3, 7, 5 } };

    // the instances: 32 x 8 cubes of side 1/4, half a unit apart, at depths -3, -3.5 and -4 - the outer columns lie outside the view's
    // side planes, the left half behind the wall - and 16 more behind the eye, which occlusion alone leaves undecided (bit 0 set)
    const int NX = 32, NY = 8, BEHIND = 16, N = NX * NY + BEHIND;
    std::vector<double> matrices(size_t(N) * 16, 0.0);
    for (int k = 0; k < N; ++k) {
        double* m = &matrices[size_t(k) * 16];
        m[0] = m[5] = m[10] = 0.25; m[15] = 1.0;
        if (k < NX * NY) { m[3] = -7.75 + 0.5 * (k % NX); m[7] = -1.75 + 0.5 * (k / NX); m[11] = -3.0 - 0.5 * (k % 3); }
        else { m[3] = -3.75 + 0.5 * (k - NX * NY); m[7] = 0.0; m[11] = 7.0; }
    }
    const double origin[3] = { 0, 0, 0 };

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_instance_cull: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));

    double* d_matrices = nullptr; double* d_boxes = nullptr; std::uint8_t* d_codes = nullptr; double* d_depths = nullptr; std::uint32_t* d_order = nullptr;
    HIP(hipMalloc((void**)&d_matrices, matrices.size() * sizeof(double)));
    HIP(hipMalloc((void**)&d_boxes, size_t(N) * 6 * sizeof(double)));
    HIP(hipMalloc((void**)&d_codes, size_t(N)));
    HIP(hipMalloc((void**)&d_depths, size_t(N) * sizeof(double)));
    HIP(hipMalloc((void**)&d_order, size_t(N) * sizeof(std::uint32_t)));
    HIP(hipMemcpy(d_matrices, matrices.data(), matrices.size() * sizeof(double), hipMemcpyHostToDevice));

    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    const std::uint8_t clear[4] = { 48, 32, 24, 255 };

    // 1. the local box, once (48 bytes: it travels to the kernel as an argument)
    double local[6];
    CHECK(trgl_mesh_bounds(nullptr, &cube[0][0], 8, 8, TRGL_MEM_HOST, local, local + 3));

    const char* names[3] = { "every instance", "occlusion", "occlusion + frustum" };
    unsigned long long digest[3], frags[3], drawn[3];
    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    for (int run = NONE; run <= OCCLUSION_AND_FRUSTUM; ++run) {
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_reset_stats(ctx));
        CHECK(trgl_draw(ctx, TRGL_SHADER_FLAT, nullptr, wall_clip, nullptr, wall_colors, 2, TRGL_MEM_HOST));
        if (run >= OCCLUSION) {
            CHECK(trgl_instance_boxes(ctx, local, 0, d_matrices, 16, uint64_t(N), TRGL_MEM_DEVICE, d_boxes));                       // 2.
            CHECK(trgl_occlusion_boxes(ctx, view_proj, d_boxes, uint64_t(N), TRGL_MEM_DEVICE, -1, d_codes, TRGL_MEM_DEVICE));       // 3. (draws the wall first)
        }
        if (run == OCCLUSION_AND_FRUSTUM)
            CHECK(trgl_frustum_boxes(ctx, planes, d_boxes, uint64_t(N), TRGL_FRUSTUM_MERGE, TRGL_MEM_DEVICE, d_codes));             // 4.
        CHECK(trgl_instance_depths(ctx, model_view, origin, d_matrices, 16, uint64_t(N), TRGL_MEM_DEVICE, d_depths));               // 5.
        CHECK(trgl_depth_order(ctx, d_depths, uint64_t(N), TRGL_ORDER_FRONT_TO_BACK, TRGL_MEM_DEVICE, d_order));                    // 6.
        CHECK(trgl_draw_instanced_ordered(ctx, -1, TRGL_SHADER_PHONG, &u, projection, &cube[0][0], 8, 8, &faces[0][0], 12, nullptr, TRGL_MEM_HOST,
                                          d_matrices, 16, uint64_t(N), nullptr, run == NONE ? nullptr : d_codes, TRGL_MEM_DEVICE,
                                          d_order, uint64_t(N), TRGL_MEM_DEVICE));                                                  // 7.
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        digest[run] = fnv1a(px); frags[run] = (unsigned long long)st.fragments_drawn;
        drawn[run] = ((unsigned long long)st.triangles_rasterized - 2) / 12;                       // the wall's two triangles, then 12 per drawn instance
    }
    std::printf("instances: %d\nremoved by occlusion: %llu\nremoved by the frustum on top: %llu\ndrawn: %llu\n", N, drawn[0] - drawn[1],
                drawn[1] - drawn[2], drawn[2]);
    for (int run = 0; run < 3; ++run) std::printf("%s: digest %016llx fragments_drawn %llu\n", names[run], digest[run], frags[run]);

    (void)hipFree(d_matrices); (void)hipFree(d_boxes); (void)hipFree(d_codes); (void)hipFree(d_depths); (void)hipFree(d_order);
    trgl_destroy(ctx);
    if (digest[1] != digest[0] || digest[2] != digest[0] || frags[1] != frags[0] || frags[2] != frags[0]) {
        std::fprintf(stderr, "demo_instance_cull: a culled instance had a fragment to give\n");
        return 3;
    }
    return 0;
}
