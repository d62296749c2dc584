// demo_lod.cpp — three levels of detail of one mesh made in device memory (include/trgl.h: trgl_mesh_weld, trgl_mesh_simplify,
// trgl_mesh_normals, trgl_draw_indexed), over the C ABI, and the same levels through the shim's host calls (gl_mesh_weld,
// gl_mesh_simplify) for comparison.
//   1. a sphere as a triangle soup - the octahedron subdivided five times, three records per face (position +0, a zero normal +3,
//      uv +6) -, or the faces of an OBJ file (trgl_obj_load), is uploaded and welded by position;
//   2. three chained trgl_mesh_simplify calls with doubling cells and mean_count 3, each over the CAPACITIES of the one before - the
//      fill faces of a level name no vertex and its fill records are named by nobody, so the next level drops both;
//   3. trgl_mesh_normals on each level (the kept records carry the zero normals of the input, so normals are generated) and a frame of
//      trgl_draw_indexed per level.
// The mesh and its levels exist in device memory only; the waits before the flushes are for the 16-byte counts this program prints.
//   demo_lod [width height [file.obj cell]]
// prints the counts of every level and the frames' digests, then what gl_mesh_clean keeps of a grid-welded level 0 - compared word for word
// with trgl_mesh_clean -; exits with 3 if a level is not smaller than the one before or anything differs from the shim's.  Every number of the generated scene is an integer, a literal, a quotient of two integers or a square root.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../tinyrenderder_amd/shim/trgl_gl.h"

#define CHECK(expr) do { const int rc_ = (expr); if (rc_ != TRGL_OK) { std::fprintf(stderr, "demo_lod: %s: %s (code %d)\n", #expr, trgl_last_error(ctx), rc_); return 2; } } while (0)
#define HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { std::fprintf(stderr, "demo_lod: %s: %s\n", #expr, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long fnv1a(const std::uint8_t* px, size_t n) {
    std::uint64_t digest = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    return (unsigned long long)digest;
}

template <class T> static int upload(T** dev, const std::vector<T>& host) {
    if (hipMalloc((void**)dev, host.size() * sizeof(T)) != hipSuccess) return 1;
    return hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
}

static const int S = 8;             // doubles per record

// the octahedron subdivided `level` times, every new corner pushed to the unit sphere, as a soup: three records per face
static void sphere_soup(int level, std::vector<double>& vertices, std::vector<unsigned int>& indices) {
    struct P { double x, y, z; };
    std::vector<P> pos = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 } };
    std::vector<std::uint32_t> f = { 0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5 };
    for (int l = 0; l < level; ++l) {
        std::map<std::pair<std::uint32_t, std::uint32_t>, std::uint32_t> mid;
        auto midpoint = [&](std::uint32_t a, std::uint32_t b) {
            const auto key = std::make_pair(a < b ? a : b, a < b ? b : a);
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const P p{ pos[key.first].x + pos[key.second].x, pos[key.first].y + pos[key.second].y, pos[key.first].z + pos[key.second].z };
            const double len = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
            pos.push_back(P{ p.x / len, p.y / len, p.z / len });
            return mid[key] = std::uint32_t(pos.size() - 1);
        };
        std::vector<std::uint32_t> finer;
        for (size_t i = 0; i < f.size(); i += 3) {
            const std::uint32_t a = f[i], b = f[i + 1], c = f[i + 2], ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
            for (std::uint32_t x : { a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca }) finer.push_back(x);
        }
        f.swap(finer);
    }
    vertices.assign(f.size() * S, 0.0);
    indices.resize(f.size());
    for (size_t i = 0; i < f.size(); ++i) {
        double* v = &vertices[i * S];
        v[0] = pos[f[i]].x; v[1] = pos[f[i]].y; v[2] = pos[f[i]].z;
        indices[i] = (unsigned int)i;
    }
}

int main(int argc, char** argv) {
    if (argc != 1 && argc != 3 && argc != 5) { std::fprintf(stderr, "usage: demo_lod [width height [file.obj cell]]\n"); return 1; }
    const int W = argc >= 3 ? std::atoi(argv[1]) : 320, H = argc >= 3 ? std::atoi(argv[2]) : 200;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_lod: bad size\n"); return 1; }
    double cell = 1.0 / 16;
    trgl_ctx* ctx = nullptr;

    std::vector<double> vertices;
    std::vector<unsigned int> indices;
    if (argc == 5) {
        double* v = nullptr; std::uint32_t* idx = nullptr; std::uint64_t nv = 0, nf = 0;
        CHECK(trgl_obj_load(argv[3], &v, &nv, &idx, &nf));
        vertices.assign(nv * S, 0.0);                                  // position and uv; the normals are generated per level
        for (std::uint64_t i = 0; i < nv; ++i) {
            for (int k = 0; k < 3; ++k) vertices[i * S + k] = v[i * 14 + k];
            vertices[i * S + 6] = v[i * 14 + 6]; vertices[i * S + 7] = v[i * 14 + 7];
        }
        indices.assign(idx, idx + 3 * nf);
        trgl_obj_free(v, idx);
        cell = std::atof(argv[4]);
        if (!(cell > 0)) { std::fprintf(stderr, "demo_lod: bad cell\n"); return 1; }
    } else {
        sphere_soup(5, vertices, indices);
    }
    const std::uint64_t NV = vertices.size() / S, NF = indices.size() / 3;

    // the sphere turned about y and then about x by the angle with cosine 0.8 and sine 0.6, five units down -z; near 1, far 17
    const double model_view[16] = { 0.8, 0, 0.6, 0,  0.36, 0.8, -0.48, 0,  -0.48, 0.6, 0.64, -5,  0, 0, 0, 1 };
    const double projection[16] = { 1.25, 0, 0, 0,  0, 2, 0, 0,  0, 0, -1.125, -2.25,  0, 0, -1, 0 };

    if (trgl_create(0, W, H, 3, &ctx) != TRGL_OK) { std::fprintf(stderr, "demo_lod: trgl_create: %s\n", trgl_last_error(nullptr)); return 2; }
    CHECK(trgl_init_viewport(ctx, 0, 0, W, H));
    double* d_soup = nullptr; std::uint32_t* d_soup_idx = nullptr;
    if (upload(&d_soup, vertices) || upload(&d_soup_idx, indices)) { std::fprintf(stderr, "demo_lod: upload failed\n"); return 2; }
    // level 0 is the welded mesh, levels 1 .. 3 its simplifications: four pairs of arrays at the capacities NV and NF
    double* d_v[4]; std::uint32_t* d_i[4];
    for (int l = 0; l < 4; ++l) {
        HIP(hipMalloc((void**)&d_v[l], NV * S * sizeof(double)));
        HIP(hipMalloc((void**)&d_i[l], NF * 3 * sizeof(std::uint32_t)));
    }
    std::uint64_t faces[4], verts[4];
    trgl_weld_params wp;
    std::memset(&wp, 0, sizeof(wp));
    wp.vertex_stride = S; wp.key_offset = 0; wp.key_count = 3;
    CHECK(trgl_mesh_weld(ctx, &wp, d_soup, NV, d_soup_idx, NF, TRGL_MEM_DEVICE, nullptr, nullptr, d_v[0], d_i[0], &verts[0]));
    faces[0] = NF;
    for (int l = 1; l < 4; ++l) {
        trgl_simplify_params sp;
        std::memset(&sp, 0, sizeof(sp));
        sp.vertex_stride = S; sp.mean_count = 3; sp.fill = TRGL_CLEAN_FILL_NONE; sp.cell = cell * double(1 << (l - 1));
        std::uint64_t counts[2];
        CHECK(trgl_mesh_simplify(ctx, &sp, d_v[l - 1], NV, d_i[l - 1], NF, TRGL_MEM_DEVICE, nullptr, nullptr, d_v[l], d_i[l], nullptr, counts));
        faces[l] = counts[0]; verts[l] = counts[1];
    }

    // the same through the shim, on the host, with real counts
    std::vector<std::uint32_t> remap;
    bool ok = gl_mesh_weld(gl_weld_params(S, 0, 3), vertices, indices, remap) && vertices.size() / S == verts[0];
    std::printf("level 0: welded, %llu faces, %llu vertices\n", (unsigned long long)faces[0], (unsigned long long)verts[0]);
    // gl_mesh_clean against trgl_mesh_clean in host memory, over a mesh that needs it: level 0 welded again on a grid (degenerate and
    // repeated faces), behind a record nobody names and in front of another, with its first whole face once more rotated and once mirrored
    std::string clean_line;
    if (ok) {
        std::vector<double> gv = vertices;
        std::vector<unsigned int> gi = indices;
        ok = gl_mesh_weld(gl_weld_params(S, 0, 3, 2 * cell), gv, gi, remap);
        std::vector<double> cv(S, 7.0);
        cv.insert(cv.end(), gv.begin(), gv.end());
        cv.insert(cv.end(), S, 7.0);
        std::vector<unsigned int> ci;
        for (unsigned int i : gi) ci.push_back(i + 1);
        std::size_t t = 0;                                              // the first face the weld left with three distinct corners
        while (3 * t + 3 < ci.size() && (ci[3 * t] == ci[3 * t + 1] || ci[3 * t + 1] == ci[3 * t + 2] || ci[3 * t + 2] == ci[3 * t])) ++t;
        for (unsigned int i : { ci[3 * t + 1], ci[3 * t + 2], ci[3 * t], ci[3 * t + 2], ci[3 * t + 1], ci[3 * t] }) ci.push_back(i);
        const std::size_t n = cv.size() / S, F = ci.size() / 3;
        for (int duplicates = 1; ok && duplicates >= 0; --duplicates) {
            trgl_clean_params cp;
            std::memset(&cp, 0, sizeof(cp));
            cp.vertex_stride = S; cp.flags = TRGL_CLEAN_VERTICES | (duplicates ? TRGL_CLEAN_DUPLICATES : 0u); cp.fill = TRGL_CLEAN_FILL_NONE;
            std::vector<double> wv(cv.size());
            std::vector<std::uint32_t> wi(ci.size()), wmap(n);
            std::uint64_t counts[2];
            CHECK(trgl_mesh_clean(nullptr, &cp, ci.data(), F, cv.data(), n, TRGL_MEM_HOST, wi.data(), nullptr, wmap.data(), nullptr, wv.data(), counts));
            std::vector<double> sv = cv;
            std::vector<unsigned int> si = ci;
            std::vector<std::uint32_t> smap;
            ok = gl_mesh_clean(S, sv, si, smap, duplicates != 0) && si.size() == 3 * counts[0] && sv.size() == S * counts[1] && smap == wmap &&
                 std::memcmp(si.data(), wi.data(), si.size() * sizeof(std::uint32_t)) == 0 && std::memcmp(sv.data(), wv.data(), sv.size() * sizeof(double)) == 0 &&
                 counts[0] < F && counts[1] + 2 <= n && smap.front() == 0xFFFFFFFFu && smap.back() == 0xFFFFFFFFu;
            char line[200];
            std::snprintf(line, sizeof(line), "%s%llu of %llu faces and %llu of %llu vertices", duplicates ? "clean: " : "; with repeated faces kept ",
                          (unsigned long long)counts[0], (unsigned long long)F, (unsigned long long)counts[1], (unsigned long long)n);
            clean_line += line;
        }
        // a call that fails leaves the three vectors as they were
        std::vector<double> sv = cv;
        std::vector<unsigned int> si = ci;
        std::vector<std::uint32_t> smap(3, 5u);
        si[4] = (unsigned int)n;
        const std::vector<unsigned int> before = si;
        ok = ok && !gl_mesh_clean(S, sv, si, smap) && gl_last_error() == TRGL_E_INVALID && si == before && sv.size() == cv.size() &&
             std::memcmp(sv.data(), cv.data(), cv.size() * sizeof(double)) == 0 && smap == std::vector<std::uint32_t>(3, 5u);
    }
    trgl_uniforms u;
    std::memset(&u, 0, sizeof(u));
    std::memcpy(u.model_view, model_view, sizeof(model_view));
    u.key_light_dir_eye[2] = u.fill_light_dir_eye[2] = u.rim_light_dir_eye[2] = 1.0;
    u.normal_map_strength = 1.0;
    u.tex_diffuse = u.tex_normal = u.tex_specular = -1;
    const std::uint8_t clear[4] = { 200, 208, 216, 255 };
    std::vector<std::uint8_t> px(size_t(W) * H * 3);
    for (int l = 1; l < 4; ++l) {
        const double c = cell * double(1 << (l - 1));
        ok = ok && gl_mesh_simplify(S, c, 3, vertices, indices, remap) && indices.size() / 3 == faces[l] && vertices.size() / S == verts[l];
        if (ok) {                                                       // ... and the device's words below the counts are the shim's
            std::vector<std::uint32_t> got(indices.size());
            std::vector<double> gv(vertices.size());
            HIP(hipMemcpy(got.data(), d_i[l], got.size() * sizeof(std::uint32_t), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(gv.data(), d_v[l], gv.size() * sizeof(double), hipMemcpyDeviceToHost));
            ok = std::memcmp(got.data(), indices.data(), got.size() * sizeof(std::uint32_t)) == 0 && std::memcmp(gv.data(), vertices.data(), gv.size() * sizeof(double)) == 0;
        }
        ok = ok && faces[l] < faces[l - 1] && verts[l] < verts[l - 1] && faces[l] > 0;
        CHECK(trgl_mesh_normals(ctx, d_v[l], S, verts[l], d_i[l], faces[l], TRGL_MEM_DEVICE, nullptr));
        CHECK(trgl_clear(ctx, clear, std::numeric_limits<double>::infinity()));
        CHECK(trgl_draw_indexed(ctx, TRGL_SHADER_PHONG, &u, projection, d_v[l], S, verts[l], d_i[l], faces[l], TRGL_MEM_DEVICE));
        CHECK(trgl_flush(ctx));
        CHECK(trgl_read_framebuffer(ctx, px.data()));
        trgl_stats st;
        CHECK(trgl_get_stats(ctx, &st));
        std::printf("level %d: cell %.17g, %llu faces, %llu vertices, frame digest %016llx fragments_drawn %llu\n", l, c, (unsigned long long)faces[l],
                    (unsigned long long)verts[l], fnv1a(px.data(), px.size()), (unsigned long long)st.fragments_drawn);
    }

    std::printf("%s\n", clean_line.c_str());
    (void)hipFree(d_soup); (void)hipFree(d_soup_idx);
    for (int l = 0; l < 4; ++l) { (void)hipFree(d_v[l]); (void)hipFree(d_i[l]); }
    trgl_destroy(ctx);
    if (!ok) {
        std::fprintf(stderr, "demo_lod: a level is not smaller than the one before, or differs from the shim's: %s\n", gl_last_error_message());
        return 3;
    }
    return 0;
}
