// demo_weld.cpp — a cube as an OBJ reader delivers it - one vertex per (position, face normal) pair, 24 in all - welded by position in
// device memory, then refined and outlined (include/trgl.h: trgl_mesh_weld, trgl_mesh_edges, trgl_subdiv_topology,
// trgl_draw_subdivided, trgl_draw_outline), over the C ABI.
//   1. the 24 records (position +0, normal +3, uv +6) and the 12 faces are uploaded; trgl_mesh_edges on them as they are: every side of
//      every quad is a boundary, the mesh is split along its normal seams;
//   2. trgl_mesh_weld with key_offset 0, key_count 3: 8 vertices remain, the indices are renumbered;
//   3. trgl_mesh_edges on the welded indices: the cube's 12 edges and the 6 diagonals of its quads, none a boundary;
//   4. trgl_subdiv_topology, trgl_draw_subdivided (one level of Loop) and trgl_draw_outline over the capacities - 24 vertices, 36 records -,
//      so the chain from the weld to the draws needs no number on the host.
// The mesh, its edges and tables exist in device memory only; the only waits before the flush are the 8-byte counts this program prints.
//   demo_weld [width height]
// prints the edge and boundary counts before and after the weld and the frame's digest; exits with 3 if the welded cube is not closed.
// Every number of the scene is an integer, a literal or a quotient of two integers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../include/trgl.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_weld: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_weld: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long fnv1a(const std::uint8_t* px, size_t n) {
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

template <class T> static int upload(T** dev, const std::vector<T>& host) {
    if (hipMalloc((void**)dev, host.size() * sizeof(T)) != hipSuccess) return 1;
    return hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
}

int main(int argc, char** argv) {
    if (argc != 1 && argc != 3) { std::fprintf(stderr, "usage: demo_weld [width height]\n"); return 1; }
    const int W = argc == 3 ? std::atoi(argv[1]) : 320, H = argc == 3 ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_weld: bad size\n"); return 1; }

    // the cube turned about y and then about x by the angle with cosine 0.8 and sine 0.6, five units down -z; near 1, far 17
    const double model_view[16] = { 0.8, 0, 0.6, 0,  0.36, 0.8, -0.48, 0,  -0.48, 0.6, 0.64, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };
    const double eye[4] = { -2.4, 3, 3.2, 1 };                      // the camera in model space
    const double LINE_BIAS = 1.0 / 64, LINE_WIDTH = 2.0, ZNEAR = 1.0;

    // corner c of the cube at (+-1, +-1, +-1): bit 0 of c is x, bit 1 y, bit 2 z; six quads, counter-clockwise from outside
    const int S = 8, NV = 24, NF = 12;
    const int quad[6][4] = { { 0, 2, 3, 1 }, { 4, 5, 7, 6 }, { 0, 1, 5, 4 }, { 2, 6, 7, 3 }, { 0, 4, 6, 2 }, { 1, 3, 7, 5 } };
    const double normal[6][3] = { { 0, 0, -1 }, { 0, 0, 1 }, { 0, -1, 0 }, { 0, 1, 0 }, { -1, 0, 0 }, { 1, 0, 0 } };
    std::vector<double> vertices(size_t(NV) * S, 0.0);
    std::vector<std::uint32_t> indices;
    for (int q = 0; q < 6; ++q) {
        for (int k = 0; k < 4; ++k) {
            const int c = quad[q][k];
            double* v = &vertices[size_t(4 * q + k) * S];
            v[0] = (c & 1) ? 1.0 : -1.0; v[1] = (c & 2) ? 1.0 : -1.0; v[2] = (c & 4) ? 1.0 : -1.0;
            v[3] = normal[q][0]; v[4] = normal[q][1]; v[5] = normal[q][2];
            v[6] = (k == 1 || k == 2) ? 1.0 : 0.0; v[7] = k >= 2 ? 1.0 : 0.0;
        }
        const std::uint32_t b = std::uint32_t(4 * q);
        for (std::uint32_t i : { b, b + 1, b + 2, b, b + 2, b + 3 }) indices.push_back(i);
    }

    trgl_ctx* ctx = nullptr;
    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_weld: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_vertices = nullptr; std::uint32_t* d_indices = nullptr;
    if (upload(&d_vertices, vertices) || upload(&d_indices, indices)) { std::fprintf(stderr, "demo_weld: upload failed\n"); return 2; }
    const std::uint64_t EC = 3ull * NF;                             // the capacity of the edge records
    double* d_welded = nullptr; std::uint32_t* d_windices = nullptr; std::uint32_t* d_edges = nullptr; std::uint32_t* d_refined = nullptr;
    std::uint32_t* d_stencils = nullptr;
    HIP(hipMalloc((void**)&d_welded, size_t(NV) * S * sizeof(double)));
    HIP(hipMalloc((void**)&d_windices, size_t(NF) * 3 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_edges, EC * 4 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_refined, size_t(NF) * 12 * sizeof(std::uint32_t)));
    HIP(hipMalloc((void**)&d_stencils, trgl_subdiv_stencil_words(NV, EC) * sizeof(std::uint32_t)));

    trgl_edge_params boundary;
    std::memset(&boundary, 0, sizeof(boundary));
    std::memcpy(boundary.eye, eye, sizeof(eye));
    boundary.crease_cos = -2.0; boundary.select = TRGL_EDGE_BOUNDARY; boundary.compact = 1;

    // 1. as delivered
    std::uint64_t edges_before = 0, boundaries_before = 0, n_unique = 0, edges_after = 0, boundaries_after = 0;
    CHECK(trgl_mesh_edges(ctx, d_indices, NF, NV, TRGL_MEM_DEVICE, d_edges, &edges_before));
    CHECK(trgl_edge_select(ctx, &boundary, d_vertices, S, NV, d_indices, NF, d_edges, EC, TRGL_MEM_DEVICE, nullptr, nullptr, nullptr, &boundaries_before));
    // 2. welded by position
    trgl_weld_params wp;
    std::memset(&wp, 0, sizeof(wp));
    wp.vertex_stride = S; wp.key_offset = 0; wp.key_count = 3; wp.cell = 0.0;
    CHECK(trgl_mesh_weld(ctx, &wp, d_vertices, NV, d_indices, NF, TRGL_MEM_DEVICE, nullptr, nullptr, d_welded, d_windices, &n_unique));
    // 3. its edges
    CHECK(trgl_mesh_edges(ctx, d_windices, NF, NV, TRGL_MEM_DEVICE, d_edges, &edges_after));
    CHECK(trgl_edge_select(ctx, &boundary, d_welded, S, NV, d_windices, NF, d_edges, EC, TRGL_MEM_DEVICE, nullptr, nullptr, nullptr, &boundaries_after));
    std::printf("before the weld: %llu vertices, %llu edges, %llu of them boundaries\n", (unsigned long long)NV, (unsigned long long)edges_before,
                (unsigned long long)boundaries_before);
    std::printf("after the weld:  %llu vertices, %llu edges, %llu of them boundaries\n", (unsigned long long)n_unique, (unsigned long long)edges_after,
                (unsigned long long)boundaries_after);

    // 4. refined and outlined, over the capacities
    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    trgl_subdiv_params sub;
    std::memset(&sub, 0, sizeof(sub));
    sub.vertex_stride = S; sub.smooth = 3; sub.mode = TRGL_SUBDIV_LOOP;
    trgl_edge_params ep = boundary;
    for (int k = 0; k < 4; ++k) ep.class_color[k] = 0xff000000u;
    ep.crease_cos = 0.5; ep.select = TRGL_EDGE_SILHOUETTE | TRGL_EDGE_CREASE;
    trgl_line_params lp;
    std::memset(&lp, 0, sizeof(lp));
    std::memcpy(lp.model_view, model_view, sizeof(model_view));
    std::memcpy(lp.projection, projection, sizeof(projection));
    lp.projection[11] = projection[11] - LINE_BIAS;
    lp.width = LINE_WIDTH; lp.half_extent[0] = W / 2.0; lp.half_extent[1] = H / 2.0; lp.w_min = ZNEAR;
    const std::uint8_t clear[4] = { 200, 208, 216, 255 };
    CHECK(trgl_subdiv_topology(ctx, d_windices, NF, NV, d_edges, EC, TRGL_MEM_DEVICE, d_refined, d_stencils));
    CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
    CHECK(trgl_draw_subdivided(ctx, -1, TRGL_SHADER_PHONG, &u, projection, &sub, d_welded, NV, d_stencils, EC, d_refined, 4ull * NF, nullptr, TRGL_MEM_DEVICE));
    CHECK(trgl_draw_outline(ctx, TRGL_SHADER_FLAT, nullptr, &lp, &ep, d_welded, S, NV, d_windices, NF, d_edges, EC, TRGL_MEM_DEVICE));
    CHECK(trgl_flush(ctx));
    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    CHECK(trgl_read_framebuffer(ctx, px.data()));
    trgl_stats st;
    CHECK(trgl_get_stats(ctx, &st));
    std::printf("frame digest: %016llx fragments_drawn %llu\n", fnv1a(px.data(), px.size()), (unsigned long long)st.fragments_drawn);

    (void)hipFree(d_vertices); (void)hipFree(d_indices); (void)hipFree(d_welded); (void)hipFree(d_windices); (void)hipFree(d_edges);
    (void)hipFree(d_refined); (void)hipFree(d_stencils);
    trgl_destroy(ctx);
    if (n_unique != 8 || edges_after != 18 || boundaries_after != 0 || boundaries_before == 0) {
        std::fprintf(stderr, "demo_weld: the welded cube is not closed\n");
        return 3;
    }
    return 0;
}
