// trgl_host.cpp — the part of the C ABI in include/trgl.h that runs on the host alone and includes no HIP header: mesh attributes and
// bounds in host memory, AABB / frustum / shadow-matrix maths, TGA and OBJ files, stats formatting, the global error string.
// Its arithmetic is pinned bit for bit to the reference (-ffp-contract=off; the sums are chains of `sum += ...`, in the reference's order).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/trgl.h"
#include "box_core.h"
#include "clip_core.h"
#include "mip_core.h"
#include "occlusion_core.h"
#include "scene_core.h"
#include "triorder_core.h"
#include "sprite_core.h"
#include "skin_core.h"
#include "edge_core.h"
#include "subdiv_core.h"
#include "weld_core.h"
#include "lod_core.h"
#include "../shim/trgl_image.h"
#include "../shim/trgl_obj.h"

namespace trgl {
static thread_local std::string g_error;
void set_global_error(const std::string& msg) { g_error = msg; }
const char* global_error() { return g_error.c_str(); }
int fail(trgl_ctx* c, int code, const std::string& msg);       // trgl_api.cpp; called with c == nullptr here

// ---- the box filter (include/trgl.h, trgl_image_downsample; box_core.h) ------------------------------------------------------------
void host_box_filter(const uint8_t* src, int w, int h, int bpp, int f, uint8_t* dst) {
    const int w2 = w / f, h2 = h / f;
    const size_t row = (size_t)w * bpp;
    if (f == 1) { std::memcpy(dst, src, row * h); return; }
    const uint32_t half = (uint32_t)(f * f) / 2, magic = box_magic(f);
    for (int y = 0; y < h2; ++y)
        for (int x = 0; x < w2; ++x)
            for (int c = 0; c < bpp; ++c) {
                uint32_t sum = 0;
                for (int j = 0; j < f; ++j) {
                    const uint8_t* p = src + ((size_t)y * f + j) * row + (size_t)x * f * bpp + c;
                    for (int i = 0; i < f; ++i) sum += p[(size_t)i * bpp];
                }
                *dst++ = (uint8_t)box_round(sum, half, magic);
            }
}

// ---- mip chains, filtered samples and the LOD stage over host arrays (include/trgl.h, "Mipmapped textures"; mip_core.h) ---------------
// levels 1 .. L-1 of src into dst, in the packed layout; only the levels' bytes are written
void host_mipmaps(const uint8_t* src, int w, int h, int bpp, uint8_t* dst) {
    const int L = mip_levels(w, h);
    const uint8_t* prev = src;
    for (int l = 1; l < L; ++l) {
        const int pw = mip_side(w, l - 1), ph = mip_side(h, l - 1), cw = mip_side(w, l), ch = mip_side(h, l);
        const int fx = pw >= 2 ? 2 : 1, fy = ph >= 2 ? 2 : 1;
        const size_t prow = (size_t)pw * bpp;
        uint8_t* out = dst + mip_packed_offset(w, h, bpp, l);
        uint8_t* o = out;
        for (int y = 0; y < ch; ++y)
            for (int x = 0; x < cw; ++x)
                for (int c = 0; c < bpp; ++c) {
                    uint32_t sum = 0;
                    for (int j = 0; j < fy; ++j)
                        for (int i = 0; i < fx; ++i) sum += prev[((size_t)y * fy + j) * prow + ((size_t)x * fx + i) * bpp + c];
                    *o++ = (uint8_t)mip_round(sum, (uint32_t)(fx * fy));
                }
        prev = out;
    }
}

void host_lod_stage(const double viewport[16], const double* clip, double* vary, uint64_t n, int K, int uv_offset, int out_offset) {
    for (uint64_t t = 0; t < n; ++t) {
        double* row = vary + t * (uint64_t)K;
        double out[4];
        mip_lod_constants(viewport, clip + t * 12, row + uv_offset, out);
        for (int i = 0; i < 4; ++i) row[out_offset + i] = out[i];
    }
}

// ---- scene logic around the draws (model.cpp:15-40, geometry.h:264-266,297-327, our_gl.cpp:212-280) ------------------------------
// keep_min / keep_max (the running std::min / std::max) and dot3_from_zero, AABB::transform and Frustum::intersects: scene_core.h

void host_mesh_bounds(const double* vertices, int stride, uint64_t n, double out_min[3], double out_max[3]) {
    double lo[3] = { 1e9, 1e9, 1e9 }, hi[3] = { -1e9, -1e9, -1e9 };         // model.cpp:21-22
    for (uint64_t i = 0; i < n; ++i) {
        const double* p = vertices + i * (uint64_t)stride;
        for (int a = 0; a < 3; ++a) lo[a] = keep_min(lo[a], p[a]);          // :25-27
        for (int a = 0; a < 3; ++a) hi[a] = keep_max(hi[a], p[a]);          // :29-31
    }
    for (int a = 0; a < 3; ++a) {
        const double margin = (hi[a] - lo[a]) * 0.01;                       // :35
        out_min[a] = lo[a] - margin; out_max[a] = hi[a] + margin;           // :36
    }
}

// ---- Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388) ----------------------
// norm (geometry.h:130-133) of three consecutive doubles
static inline double norm3_from_zero(const double* v) { return std::sqrt(dot3_from_zero(v, v[0], v[1], v[2])); }
// normalized (geometry.h:136-140): a zero vector comes back unchanged
static inline void normalize3(double* v) {
    const double length = norm3_from_zero(v);
    if (length == 0) return;
    for (int a = 0; a < 3; ++a) v[a] = v[a] / length;
}

static void host_mesh_normals(double* vertices, uint64_t stride, uint64_t n, const uint32_t* indices, uint64_t nfaces) {
    for (uint64_t i = 0; i < n; ++i) { double* nrm = vertices + i * stride + 3; nrm[0] = nrm[1] = nrm[2] = 0.0; }     // :283-285
    for (uint64_t f = 0; f < nfaces; ++f) {                                                                          // :288-305
        const double* v0 = vertices + indices[3 * f] * stride; const double* v1 = vertices + indices[3 * f + 1] * stride;
        const double* v2 = vertices + indices[3 * f + 2] * stride;
        double e1[3], e2[3];
        for (int a = 0; a < 3; ++a) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
        const double fn[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        for (int k = 0; k < 3; ++k) {
            double* nrm = vertices + indices[3 * f + k] * stride + 3;
            for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] + fn[a];
        }
    }
    for (uint64_t i = 0; i < n; ++i) {                                                                               // :308-315
        double* nrm = vertices + i * stride + 3;
        const double length = norm3_from_zero(nrm);
        if (length > 0.001) { for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] / length; }
        else { nrm[0] = 0; nrm[1] = 0; nrm[2] = 1; }
    }
}

static void host_mesh_tangents(double* vertices, uint64_t stride, uint64_t n, const uint32_t* indices, uint64_t nfaces) {
    for (uint64_t i = 0; i < n; ++i) { double* t = vertices + i * stride + 8; for (int a = 0; a < 6; ++a) t[a] = 0.0; }   // :332-335
    for (uint64_t f = 0; f < nfaces; ++f) {                                                                          // :338-368
        const double* v0 = vertices + indices[3 * f] * stride; const double* v1 = vertices + indices[3 * f + 1] * stride;
        const double* v2 = vertices + indices[3 * f + 2] * stride;
        double dp1[3], dp2[3];
        for (int a = 0; a < 3; ++a) { dp1[a] = v1[a] - v0[a]; dp2[a] = v2[a] - v0[a]; }
        const double duv1x = v1[6] - v0[6], duv1y = v1[7] - v0[7], duv2x = v2[6] - v0[6], duv2y = v2[7] - v0[7];
        const double r = duv1x * duv2y - duv2x * duv1y;                                                              // :353
        if (std::fabs(r) < 1e-8) continue;
        const double invr = 1.0 / r;
        double tangent[3], bitangent[3];
        for (int a = 0; a < 3; ++a) {
            tangent[a] = (dp1[a] * duv2y - dp2[a] * duv1y) * invr;                                                   // :358
            bitangent[a] = (dp2[a] * duv1x - dp1[a] * duv2x) * invr;                                                 // :359
        }
        for (int k = 0; k < 3; ++k) { double* t = vertices + indices[3 * f + k] * stride + 8; for (int a = 0; a < 3; ++a) t[a] = t[a] + tangent[a]; }
        for (int k = 0; k < 3; ++k) { double* b = vertices + indices[3 * f + k] * stride + 11; for (int a = 0; a < 3; ++a) b[a] = b[a] + bitangent[a]; }
    }
    for (uint64_t i = 0; i < n; ++i) {                                                                               // :371-387
        double* rec = vertices + i * stride;
        double* t = rec + 8; double* b = rec + 11;
        if (norm3_from_zero(t) > 0.001 && norm3_from_zero(rec + 3) > 0.001) {
            double nn[3] = { rec[3], rec[4], rec[5] };
            normalize3(nn);                                                                                          // :374
            normalize3(t);                                                                                           // :375
            const double d = dot3_from_zero(nn, t[0], t[1], t[2]);
            for (int a = 0; a < 3; ++a) t[a] = t[a] - nn[a] * d;                                                     // :378
            normalize3(t);
            b[0] = rec[4] * t[2] - rec[5] * t[1]; b[1] = rec[5] * t[0] - rec[3] * t[2]; b[2] = rec[3] * t[1] - rec[4] * t[0];   // :381
        } else {
            t[0] = 1; t[1] = 0; t[2] = 0; b[0] = 0; b[1] = 1; b[2] = 0;                                              // :384-385
        }
    }
}

int host_mesh_attr(bool tangents, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces) {
    for (uint64_t k = 0; k < 3 * nfaces; ++k)
        if (indices[k] >= n) return -1;
    bool need = false;                                                      // :270-276 / :319-325
    for (uint64_t i = 0; i < n && !need; ++i) need = norm3_from_zero(vertices + i * (uint64_t)stride + (tangents ? 8 : 3)) < 0.001;
    if (!need) return 0;
    if (tangents) host_mesh_tangents(vertices, (uint64_t)stride, n, indices, nfaces);
    else host_mesh_normals(vertices, (uint64_t)stride, n, indices, nfaces);
    return 1;
}

// ---- the clip stage in host memory (include/trgl.h, trgl_clip_stage; the arithmetic is clip_core.h's) -------------------------------
uint64_t host_clip_stage(const double plane[4], const ClipTable& tab, int K, const double* clip, const double* vary, const uint32_t* colors,
                         uint64_t n, double* clip_out, double* vary_out, uint32_t* colors_out) {
    uint64_t o = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const double* tri = clip + i * 12;
        const double* vin = K ? vary + i * (uint64_t)K : nullptr;
        double t[2];
        const int code = clip_classify(tri, plane, t);
        for (int which = 0; which < clip_outputs(code); ++which, ++o) {
            clip_emit_clip(tri, code, which, t, clip_out + o * 12);
            for (int c = 0; c < K; ++c) vary_out[o * (uint64_t)K + c] = clip_emit_vary(vin, c, tab.slot[c], code, which, t);
            if (colors) colors_out[o] = colors[i];
        }
    }
    return o;
}

// ---- occlusion culling of boxes against a depth image in host memory (include/trgl.h, trgl_occlusion_boxes_image; steps 1-6 are
// occlusion_core.h's, step 7 a scan of the rectangle) -----------------------------------------------------------------------------------
void host_occlusion_boxes(const double* depth, int w, int h, const double viewport[16], const double view_proj[16],
                          const double* boxes, uint64_t n, uint8_t* codes) {
    for (uint64_t i = 0; i < n; ++i) {
        const double* box = boxes + 6 * i;
        OcclFold f = occl_corner(view_proj, viewport, box, 0);
        for (int k = 1; k < 8; ++k) f = occl_merge(f, occl_corner(view_proj, viewport, box, k));
        OcclRect r;
        int code = occl_decide(f, w, h, &r);
        if (code < 0) {
            code = TRGL_OCCL_HIDDEN;
            for (int y = r.y0; y <= r.y1 && code == TRGL_OCCL_HIDDEN; ++y) {
                const double* row = depth + (size_t)y * (size_t)w;
                for (int x = r.x0; x <= r.x1; ++x)
                    if (r.zq < row[x]) { code = TRGL_OCCL_VISIBLE; break; }                          // a NaN never, +inf always
            }
        }
        codes[i] = (uint8_t)code;
    }
}

// ---- depths of instances and their order in host memory (include/trgl.h, trgl_instance_depths / trgl_depth_order) -------------------
// dot<4> (geometry.h:122-127) with the four right-hand values apart: summed left to right from 0
static inline double dot4_from_zero(const double* a, double x, double y, double z, double w) {
    double sum = 0; sum += a[0] * x; sum += a[1] * y; sum += a[2] * z; sum += a[3] * w; return sum;
}

void host_instance_depths(const double model_view[16], const double point[3], const double* instances, int stride, uint64_t n, double* depths) {
    for (uint64_t i = 0; i < n; ++i) {
        const double* M = instances + i * (uint64_t)stride;
        double r[4];
        for (int c = 0; c < 4; ++c) r[c] = dot4_from_zero(model_view + 8, M[c], M[4 + c], M[8 + c], M[12 + c]);      // geometry.h:196-205, row 2
        depths[i] = dot4_from_zero(r, point[0], point[1], point[2], 1.0);
    }
}

// false: out of memory
bool host_depth_order(const double* depths, uint64_t n, bool front_to_back, uint32_t* order) {
    try {
        std::vector<uint64_t> keys(n);
        const uint64_t flip = front_to_back ? ~0ull : 0ull;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t b; std::memcpy(&b, depths + i, sizeof(b));
            keys[i] = (b ^ ((b >> 63) ? ~0ull : 1ull << 63)) ^ flip;
            order[i] = (uint32_t)i;
        }
        std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    } catch (const std::bad_alloc&) { return false; }                         // (std::stable_sort falls back to merging in place)
    return true;
}

// ---- a depth per group of triangles and the gather of rows in host memory (include/trgl.h, trgl_triangle_depths / trgl_order_stage;
// the depth expressions are triorder_core.h's) -------------------------------------------------------------------------------------
void host_triangle_depths(const double* clip, uint64_t G, uint32_t g, int mode, double* depths) {
    for (uint64_t q = 0; q < G; ++q) {
        const double* w = clip + q * (uint64_t)g * 12 + 3;
        double acc = tri_depth_first(mode, w[0]);
        for (uint64_t v = 1; v < 3 * (uint64_t)g; ++v) acc = tri_depth_step(mode, acc, w[4 * v]);
        const uint64_t bits = tri_depth_bits(acc);
        std::memcpy(depths + q, &bits, sizeof(bits));
    }
}

// every entry of the list is below G (checked by the caller)
void host_order_stage(int K, const double* clip, const double* vary, const uint32_t* colors, const uint32_t* order, uint64_t n_order, uint32_t g,
                      double* clip_out, double* vary_out, uint32_t* colors_out) {
    for (uint64_t p = 0; p < n_order; ++p) {
        const uint64_t src = (uint64_t)order[p] * g, dst = p * g;
        std::memcpy(clip_out + dst * 12, clip + src * 12, (size_t)g * 12 * sizeof(double));
        if (K) std::memcpy(vary_out + dst * (uint64_t)K, vary + src * (uint64_t)K, (size_t)g * (size_t)K * sizeof(double));
        if (colors) std::memcpy(colors_out + dst, colors + src, (size_t)g * sizeof(uint32_t));
    }
}

// ---- point sprites and wide lines in host memory (include/trgl.h, trgl_sprite_stage / trgl_line_stage; the arithmetic and the tables
// of the two output rows are sprite_core.h's) -------------------------------------------------------------------------------------------
// rows 2 i and 2 i + 1 of the outputs from quad q; attr: the n_attr doubles behind the pairs (vary_out null: no varyings)
static void host_quad_rows(const SpriteQuad& q, uint64_t i, uint32_t color, const double* attr, int n_attr,
                           double* clip_out, double* vary_out, uint32_t* colors_out) {
    for (int r = 0; r < 24; ++r) clip_out[i * 24 + r] = q.k[quad_clip_index(r)];
    const uint64_t K = 6 + (uint64_t)n_attr;
    for (int tri = 0; vary_out && tri < 2; ++tri) {
        double* row = vary_out + (2 * i + tri) * K;
        for (int c = 0; c < 6; ++c) row[c] = quad_vary(q.ta, q.tb, q.one, quad_vary_sel(tri, c));
        if (n_attr) std::memcpy(row + 6, attr, (size_t)n_attr * sizeof(double));
    }
    if (colors_out) colors_out[2 * i] = colors_out[2 * i + 1] = color;
}

void host_sprite_stage(const trgl_sprite_params& P, const double* points, int stride, const uint32_t* colors, uint64_t n,
                       double* clip_out, double* vary_out, uint32_t* colors_out) {
    for (uint64_t i = 0; i < n; ++i) {
        const double* row = points + i * (uint64_t)stride;
        SpriteQuad q;
        sprite_quad(P, row[0], row[1], row[2], P.size_offset >= 0 ? row[P.size_offset] : P.size, &q);
        host_quad_rows(q, i, colors ? colors[i] : 0u, row + P.attr_offset, P.n_attr, clip_out, vary_out, colors ? colors_out : nullptr);
    }
}

// every index is below n_points (checked by the caller)
void host_line_stage(const trgl_line_params& P, const double* points, int stride, const uint32_t* indices, const uint32_t* colors, uint64_t n,
                     double* clip_out, double* vary_out, uint32_t* colors_out) {
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t ia = indices ? indices[2 * j] : 2 * j, ib = indices ? indices[2 * j + 1] : 2 * j + 1;
        SpriteQuad q;
        const double* a = points + ia * (uint64_t)stride; const double* b = points + ib * (uint64_t)stride;
        line_quad(P, a[0], a[1], a[2], b[0], b[1], b[2], &q);
        host_quad_rows(q, j, (colors && q.one != 0.0) ? colors[j] : 0u, nullptr, 0, clip_out, vary_out, colors ? colors_out : nullptr);
    }
}

// ---- skeletal animation in host memory (include/trgl.h, trgl_skin_stage / trgl_pose_palette; the arithmetic is skin_core.h's) ------
void host_skin_stage(const trgl_skin_params& P, const double* vertices, uint64_t n, const uint16_t* joints, const double* weights,
                     const double* palette, double* out) {
    const uint64_t S = (uint64_t)P.vertex_stride, ni = (uint64_t)P.n_influences;
    for (uint64_t q = 0; q < P.n_poses; ++q) {
        const double* pal = palette + q * P.palette_stride;
        for (uint64_t v = 0; v < n; ++v) {
            const double* in = vertices + v * S;
            double* o = out + (q * n + v) * S;
            std::memcpy(o, in, S * sizeof(double));
            double B[12];
            skin_blend_zero(B);
            for (uint64_t k = 0; k < ni; ++k) skin_blend_add(B, weights[v * ni + k], pal + 16 * (uint64_t)joints[v * ni + k]);
            skin_position(B, in[0], in[1], in[2], o);
            for (int d = 0; d < 3; ++d)
                if (P.flags & (1u << d)) { const int at = skin_dir_offset(d); skin_direction(B, in[at], in[at + 1], in[at + 2], o + at); }
        }
    }
}

void host_pose_palette(const int32_t* parents, const double* inverse_bind, uint32_t n_joints, const double* local, uint64_t local_stride,
                       uint64_t n_poses, double* palette, uint64_t palette_stride) {
    std::vector<double> world((size_t)n_joints * 16);
    for (uint64_t q = 0; q < n_poses; ++q) {
        const double* loc = local + q * local_stride;
        double* pal = palette + q * palette_stride;
        for (uint32_t j = 0; j < n_joints; ++j) {
            double* w = world.data() + 16 * (size_t)j;
            if (parents[j] < 0) std::memcpy(w, loc + 16 * (size_t)j, 16 * sizeof(double));
            else mat4_mul(world.data() + 16 * (size_t)parents[j], loc + 16 * (size_t)j, w);
            double t[16];
            if (inverse_bind) mat4_mul(w, inverse_bind + 16 * (size_t)j, t); else std::memcpy(t, w, sizeof(t));
            for (int e = 0; e < 16; ++e) pal[16 * (size_t)j + e] = skin_canon(t[e]);
        }
    }
}

// ---- mesh edges in host memory (include/trgl.h, trgl_mesh_edges / trgl_edge_select; the key and the arithmetic are edge_core.h's) ----
// every index is below n_vertices (checked by the caller); returns the number of edges
uint64_t host_mesh_edges(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, uint32_t* edges_out) {
    const int bits = edge_index_bits(n_vertices);
    const uint64_t none = edge_key_none(bits), nh = 3 * n_faces;
    std::vector<std::pair<uint64_t, uint32_t>> he;      // (key, half-edge): pairs are distinct, so their order is the stable sort's by key
    he.reserve((size_t)nh);
    for (uint64_t h = 0; h < nh; ++h) {
        const uint64_t f = h / 3, k = h - 3 * f;
        const uint64_t key = edge_key(indices[h], indices[3 * f + (k == 2 ? 0 : k + 1)], n_vertices, bits);
        if (key != none) he.emplace_back(key, (uint32_t)h);
    }
    std::sort(he.begin(), he.end());
    uint64_t e = 0;
    for (size_t i = 0; i < he.size(); ++i) {
        if (i && he[i - 1].first == he[i].first) continue;
        uint32_t* rec = edges_out + 4 * e++;
        rec[0] = edge_key_lo(he[i].first, bits); rec[1] = edge_key_hi(he[i].first, bits); rec[2] = he[i].second / 3;
        rec[3] = (i + 1 < he.size() && he[i + 1].first == he[i].first) ? he[i + 1].second / 3 : EDGE_NONE;
    }
    for (uint64_t w = 4 * e; w < 4 * nh; ++w) edges_out[w] = EDGE_NONE;
    return e;
}

// false, and nothing written, when a record names a face >= n_faces or a face of it a vertex >= n_vertices
bool host_edge_select(const trgl_edge_params& P, const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                      const uint32_t* edges, uint64_t n_edges, uint8_t* codes_out, uint32_t* segments_out, uint32_t* colors_out, uint64_t* n_selected) {
    std::vector<uint8_t> codes((size_t)n_edges);
    const auto face = [&](uint32_t f, EdgeFace* out) {
        const uint32_t* ix = indices + 3 * (uint64_t)f;
        if (f >= n_faces || ix[0] >= n_vertices || ix[1] >= n_vertices || ix[2] >= n_vertices) return false;
        *out = edge_face(vertices + ix[0] * (uint64_t)stride, vertices + ix[1] * (uint64_t)stride, vertices + ix[2] * (uint64_t)stride, P.eye);
        return true;
    };
    for (uint64_t i = 0; i < n_edges; ++i) {
        const uint32_t f0 = edges[4 * i + 2], f1 = edges[4 * i + 3];
        if (f0 == EDGE_NONE) { codes[i] = 0; continue; }
        EdgeFace A, B{};
        const bool has1 = f1 != EDGE_NONE;
        if (!face(f0, &A) || (has1 && !face(f1, &B))) return false;
        codes[i] = edge_code(A, has1, B, P.crease_cos);
    }
    uint64_t slot = 0;
    for (uint64_t i = 0; i < n_edges; ++i) {
        const uint32_t sel = codes[i] & P.select;
        if (codes_out) codes_out[i] = codes[i];
        if (P.compact && !sel) continue;
        const uint64_t at = P.compact ? slot : i;
        if (sel) ++slot;
        if (segments_out) { segments_out[2 * at] = sel ? edges[4 * i] : EDGE_NONE; segments_out[2 * at + 1] = sel ? edges[4 * i + 1] : EDGE_NONE; }
        if (colors_out) colors_out[at] = sel ? edge_color(P.class_color, sel) : 0u;
    }
    if (P.compact)
        for (uint64_t at = slot; at < n_edges; ++at) {
            if (segments_out) { segments_out[2 * at] = EDGE_NONE; segments_out[2 * at + 1] = EDGE_NONE; }
            if (colors_out) colors_out[at] = 0u;
        }
    if (n_selected) *n_selected = slot;
    return true;
}

// ---- mesh welding in host memory (include/trgl.h, trgl_mesh_weld; the key, the comparison and the hash are weld_core.h's) ----
// Every index is below n_vertices (checked by the caller), 0 < n_vertices < 2^31; returns the number of distinct vertices.  A table of
// representatives with open addressing: vertex v, in ascending v, probes from its hash for the first representative identical to it and
// takes an empty slot when there is none - a key with a NaN is identical to nothing, itself included, and is never entered.
uint64_t host_mesh_weld(const trgl_weld_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out) {
    const uint64_t S = (uint64_t)P.vertex_stride;
    uint64_t slots = 16;
    while (slots < 2 * n_vertices) slots *= 2;
    std::vector<uint32_t> table(slots, WELD_NONE), remap((size_t)n_vertices), firsts;
    for (uint64_t v = 0; v < n_vertices; ++v) {
        const double* r = vertices + v * S;
        bool has_nan = false;
        for (int a = 0; a < P.key_count; ++a) { const double q = weld_q(r[P.key_offset + a], P.cell); has_nan = has_nan || q != q; }
        uint32_t rep = (uint32_t)v;
        if (!has_nan) {
            uint64_t at = weld_hash(r, P.key_offset, P.key_count, P.cell) & (slots - 1);
            while (table[at] != WELD_NONE && !weld_identical(vertices + table[at] * S, r, P.key_offset, P.key_count, P.cell)) at = (at + 1) & (slots - 1);
            if (table[at] == WELD_NONE) table[at] = (uint32_t)v;
            rep = table[at];
        }
        if (rep == v) { remap[v] = (uint32_t)firsts.size(); firsts.push_back((uint32_t)v); }
        else remap[v] = remap[rep];
    }
    const uint64_t U = firsts.size();
    if (remap_out) std::memcpy(remap_out, remap.data(), n_vertices * sizeof(uint32_t));
    if (firsts_out) {
        std::memcpy(firsts_out, firsts.data(), U * sizeof(uint32_t));
        for (uint64_t j = U; j < n_vertices; ++j) firsts_out[j] = WELD_NONE;
    }
    if (vertices_out) {
        for (uint64_t j = 0; j < U; ++j) std::memcpy(vertices_out + j * S, vertices + firsts[j] * S, S * sizeof(double));
        std::memset(vertices_out + U * S, 0, (n_vertices - U) * S * sizeof(double));
    }
    if (indices_out) for (uint64_t i = 0; i < 3 * n_faces; ++i) indices_out[i] = remap[indices[i]];
    return U;
}

// ---- mesh levels of detail in host memory (include/trgl.h, trgl_mesh_clean / trgl_mesh_simplify; the definitions are lod_core.h's) ----
// Every index is below n_vertices (checked by the caller).  Duplicates: a table of canonical triples with open addressing, faces entered
// in ascending number - a face that finds its triple is a duplicate of an earlier candidate.
void host_mesh_clean(const trgl_clean_params& P, const uint32_t* indices, uint64_t n_faces, const double* vertices, uint64_t n_vertices,
                     uint32_t* indices_out, uint32_t* face_firsts_out, uint32_t* vremap_out, uint32_t* vfirsts_out, double* vertices_out,
                     uint64_t counts[2]) {
    const bool duplicates = (P.flags & TRGL_CLEAN_DUPLICATES) != 0, with_vertices = (P.flags & TRGL_CLEAN_VERTICES) != 0;
    std::vector<uint32_t> kept;
    uint64_t slots = 16;
    while (duplicates && slots < 2 * n_faces) slots *= 2;
    std::vector<uint32_t> table(duplicates ? slots : 0, LOD_NONE);
    for (uint64_t f = 0; f < n_faces; ++f) {
        const uint32_t a = indices[3 * f], b = indices[3 * f + 1], c = indices[3 * f + 2];
        if (lod_face_class(a, b, c, (uint32_t)n_vertices) != LOD_FACE_CANDIDATE) continue;
        if (duplicates) {
            const LodTriple t = lod_canonical(a, b, c);
            uint64_t at = lod_face_hash(t) & (slots - 1);
            for (; table[at] != LOD_NONE; at = (at + 1) & (slots - 1)) {
                const uint32_t* g = indices + 3 * (uint64_t)table[at];
                if (lod_same_triple(lod_canonical(g[0], g[1], g[2]), t)) break;
            }
            if (table[at] != LOD_NONE) continue;
            table[at] = (uint32_t)f;
        }
        kept.push_back((uint32_t)f);
    }
    const uint64_t K = kept.size();
    std::vector<uint32_t> vremap;
    uint64_t U = n_vertices;
    if (with_vertices) {
        vremap.assign((size_t)n_vertices, 0u);
        for (uint32_t f : kept) for (int k = 0; k < 3; ++k) vremap[indices[3 * (uint64_t)f + k]] = 1u;
        U = 0;
        for (uint64_t v = 0; v < n_vertices; ++v) {
            if (!vremap[v]) { vremap[v] = LOD_NONE; continue; }
            if (vfirsts_out) vfirsts_out[U] = (uint32_t)v;
            if (vertices_out) std::memcpy(vertices_out + U * (uint64_t)P.vertex_stride, vertices + v * (uint64_t)P.vertex_stride, (size_t)P.vertex_stride * sizeof(double));
            vremap[v] = (uint32_t)U++;
        }
        if (vfirsts_out) for (uint64_t j = U; j < n_vertices; ++j) vfirsts_out[j] = LOD_NONE;
        if (vertices_out) std::memset(vertices_out + U * (uint64_t)P.vertex_stride, 0, (size_t)((n_vertices - U) * (uint64_t)P.vertex_stride) * sizeof(double));
        if (vremap_out) std::memcpy(vremap_out, vremap.data(), (size_t)n_vertices * sizeof(uint32_t));
    }
    const uint32_t fill = P.fill == TRGL_CLEAN_FILL_ZERO ? 0u : LOD_NONE;
    if (indices_out) {
        for (uint64_t j = 0; j < K; ++j)
            for (int k = 0; k < 3; ++k) { const uint32_t i = indices[3 * (uint64_t)kept[j] + k]; indices_out[3 * j + k] = with_vertices ? vremap[i] : i; }
        for (uint64_t i = 3 * K; i < 3 * n_faces; ++i) indices_out[i] = fill;
    }
    if (face_firsts_out) {
        for (uint64_t j = 0; j < K; ++j) face_firsts_out[j] = kept[j];
        for (uint64_t j = K; j < n_faces; ++j) face_firsts_out[j] = LOD_NONE;
    }
    counts[0] = K; counts[1] = U;
}

// The composition the header writes down: (a) the weld by position, (b) the means of the referenced members in ascending old number,
// (c) the clean with both flags; then the two maps put together.
void host_mesh_simplify(const trgl_simplify_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out, uint32_t* face_firsts_out,
                        uint64_t counts[2]) {
    const uint64_t S = (uint64_t)P.vertex_stride, M = (uint64_t)P.mean_count;
    trgl_weld_params W{};
    W.vertex_stride = P.vertex_stride; W.key_offset = 0; W.key_count = 3; W.cell = P.cell;
    std::vector<uint32_t> remap((size_t)n_vertices), firsts((size_t)n_vertices), welded_indices((size_t)(3 * n_faces));
    std::vector<double> records(vertices_out ? (size_t)(n_vertices * S) : 0);
    const uint64_t U = host_mesh_weld(W, vertices, n_vertices, n_faces ? indices : nullptr, n_faces, remap.data(), firsts.data(),
                                      vertices_out ? records.data() : nullptr, n_faces ? welded_indices.data() : nullptr);
    if (M && vertices_out) {
        std::vector<uint8_t> referenced((size_t)n_vertices, 0);
        for (uint64_t i = 0; i < 3 * n_faces; ++i) referenced[indices[i]] = 1;
        std::vector<uint32_t> count((size_t)U, 0u), first((size_t)U, 0u);
        std::vector<double> sum((size_t)(U * M));
        for (uint64_t v = 0; v < n_vertices; ++v) {                      // ascending old number
            if (!referenced[v]) continue;
            const uint64_t j = remap[v];
            const double* r = vertices + v * S;
            if (count[j] == 0) { first[j] = (uint32_t)v; for (uint64_t a = 0; a < M; ++a) sum[j * M + a] = r[a]; }
            else for (uint64_t a = 0; a < M; ++a) sum[j * M + a] = lod_mean_add(sum[j * M + a], r[a]);
            ++count[j];
        }
        for (uint64_t j = 0; j < U; ++j) {
            if (count[j] == 1) std::memcpy(records.data() + j * S, vertices + (uint64_t)first[j] * S, (size_t)M * sizeof(double));
            else if (count[j] > 1) for (uint64_t a = 0; a < M; ++a) records[j * S + a] = lod_mean_div(sum[j * M + a], count[j]);
        }
    }
    trgl_clean_params C{};
    C.vertex_stride = P.vertex_stride; C.flags = TRGL_CLEAN_DUPLICATES | TRGL_CLEAN_VERTICES; C.fill = P.fill;
    std::vector<uint32_t> vremap(remap_out ? (size_t)n_vertices : 0), vfirsts(firsts_out ? (size_t)n_vertices : 0);
    host_mesh_clean(C, welded_indices.data(), n_faces, records.data(), n_vertices, indices_out, face_firsts_out, remap_out ? vremap.data() : nullptr,
                    firsts_out ? vfirsts.data() : nullptr, vertices_out, counts);
    if (remap_out) for (uint64_t v = 0; v < n_vertices; ++v) remap_out[v] = vremap[remap[v]];
    if (firsts_out) for (uint64_t j = 0; j < n_vertices; ++j) firsts_out[j] = vfirsts[j] == LOD_NONE ? LOD_NONE : firsts[vfirsts[j]];
}

// ---- mesh subdivision in host memory (include/trgl.h, trgl_subdiv_topology / trgl_subdiv_vertices; the rules are subdiv_core.h's) ----
// false, and nothing written, for an index or a record out of range, an inconsistent record or a pair that no record names
bool host_subdiv_topology(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t* edges, uint64_t n_edges,
                          uint32_t* indices_out, uint32_t* stencils_out) {
    const uint64_t E = n_edges, V = n_vertices;
    std::vector<uint32_t> st((size_t)(6 * E + 4 * V), SUBDIV_NONE), refined((size_t)(12 * n_faces), 0u);
    uint32_t* odd = st.data();
    uint32_t* even = st.data() + 4 * E;
    uint32_t* ring = even + 4 * V;
    for (uint64_t k = 0; k < 3 * n_faces; ++k) if (indices[k] >= V) return false;
    std::vector<uint32_t> count((size_t)V, 0u), begin((size_t)V, 0u), fill((size_t)V, 0u);
    for (uint64_t e = 0; e < E; ++e) {
        const int kind = subdiv_odd_stencil(indices, n_faces, V, edges + 4 * e, odd + 4 * e);
        if (kind == SUBDIV_REC_BAD) return false;
        if (kind == SUBDIV_REC_EDGE) { ++count[odd[4 * e]]; ++count[odd[4 * e + 1]]; }
    }
    uint32_t at = 0;
    for (uint64_t v = 0; v < V; ++v) { begin[v] = count[v] ? at : 0u; at += count[v]; }
    for (uint64_t e = 0; e < E; ++e) {      // ascending e: every vertex's entries in ascending edge number
        const uint32_t lo = odd[4 * e], hi = odd[4 * e + 1];
        if (lo == SUBDIV_NONE) continue;
        ring[begin[lo] + fill[lo]++] = hi;
        ring[begin[hi] + fill[hi]++] = lo;
    }
    // (which ring entry belongs to a boundary edge: the edges again, in the same order)
    std::vector<uint32_t> nb((size_t)V, 0u), first((size_t)V, 0u), second((size_t)V, 0u);
    for (uint64_t e = 0; e < E; ++e) {
        const uint32_t ends[2] = { odd[4 * e], odd[4 * e + 1] };
        if (ends[0] == SUBDIV_NONE || odd[4 * e + 2] != SUBDIV_NONE) continue;
        for (int s = 0; s < 2; ++s) {
            const uint32_t v = ends[s], other = ends[1 - s];
            if (nb[v] == 0) first[v] = other; else if (nb[v] == 1) second[v] = other;
            ++nb[v];
        }
    }
    for (uint64_t v = 0; v < V; ++v) {
        uint32_t* rec = even + 4 * v;
        rec[0] = begin[v]; rec[1] = count[v];
        subdiv_boundary_pair((uint32_t)v, nb[v], first[v], second[v], rec + 2, rec + 3);
    }
    for (uint64_t f = 0; f < n_faces; ++f) {
        const uint32_t a = indices[3 * f], b = indices[3 * f + 1], c = indices[3 * f + 2];
        if (a == b || b == c || c == a) continue;      // a half-edge that makes no edge: four faces (0, 0, 0)
        const uint64_t ab = subdiv_find_edge(edges, E, a, b), bc = subdiv_find_edge(edges, E, b, c), ca = subdiv_find_edge(edges, E, c, a);
        if (ab >= E || bc >= E || ca >= E || odd[4 * ab] == SUBDIV_NONE || odd[4 * bc] == SUBDIV_NONE || odd[4 * ca] == SUBDIV_NONE) return false;
        const uint32_t m_ab = (uint32_t)(V + ab), m_bc = (uint32_t)(V + bc), m_ca = (uint32_t)(V + ca);
        const uint32_t four[12] = { a, m_ab, m_ca, b, m_bc, m_ab, c, m_ca, m_bc, m_ab, m_bc, m_ca };
        std::memcpy(refined.data() + 12 * f, four, sizeof(four));
    }
    if (!refined.empty()) std::memcpy(indices_out, refined.data(), refined.size() * sizeof(uint32_t));
    if (!st.empty()) std::memcpy(stencils_out, st.data(), st.size() * sizeof(uint32_t));
    return true;
}

// false, and nothing written, for a stencil word that names no vertex
bool host_subdiv_vertices(const trgl_subdiv_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* stencils, uint64_t n_edges,
                          double* out) {
    const uint64_t E = n_edges, V = n_vertices, S = (uint64_t)P.vertex_stride;
    const uint64_t smooth = P.mode == TRGL_SUBDIV_LOOP ? (uint64_t)P.smooth : 0;
    const uint32_t* odd = stencils;
    const uint32_t* even = stencils + 4 * E;
    const uint32_t* ring = even + 4 * V;
    for (uint64_t e = 0; e < E; ++e) if (subdiv_odd_class(odd + 4 * e, V) == SUBDIV_ODD_BAD) return false;
    for (uint64_t v = 0; v < V; ++v) {
        const int kind = subdiv_even_class(even + 4 * v, (uint32_t)v, V, E);
        if (kind == SUBDIV_EVEN_BAD) return false;
        if (kind == SUBDIV_EVEN_RING)
            for (uint64_t k = 0; k < even[4 * v + 1]; ++k) if (ring[even[4 * v] + k] >= V) return false;
    }
    for (uint64_t v = 0; v < V; ++v) {
        const uint32_t* st = even + 4 * v;
        const int kind = subdiv_even_class(st, (uint32_t)v, V, E);
        const double* x = vertices + v * S;
        double* o = out + v * S;
        for (uint64_t d = 0; d < S; ++d) {
            if (d >= smooth || kind == SUBDIV_EVEN_COPY) { o[d] = x[d]; continue; }
            if (kind == SUBDIV_EVEN_EDGE) { o[d] = subdiv_even_boundary(x[d], vertices[st[2] * S + d], vertices[st[3] * S + d]); continue; }
            double sum = 0.0;
            for (uint64_t k = 0; k < st[1]; ++k) sum += vertices[ring[st[0] + k] * S + d];
            o[d] = subdiv_even_interior(st[1], x[d], sum);
        }
    }
    for (uint64_t e = 0; e < E; ++e) {
        const uint32_t* st = odd + 4 * e;
        const int kind = subdiv_odd_class(st, V);
        double* o = out + (V + e) * S;
        for (uint64_t d = 0; d < S; ++d) {
            if (kind == SUBDIV_ODD_ZERO) { o[d] = 0.0; continue; }
            const double xl = vertices[st[0] * S + d], xh = vertices[st[1] * S + d];
            o[d] = (kind == SUBDIV_ODD_FULL && d < smooth) ? subdiv_odd_interior(xl, xh, vertices[st[2] * S + d], vertices[st[3] * S + d])
                                                           : subdiv_midpoint(xl, xh);
        }
    }
    return true;
}

// ---- world boxes of instances and frustum codes of boxes in host memory (include/trgl.h, trgl_instance_boxes / trgl_frustum_boxes;
// the arithmetic is scene_core.h's) --------------------------------------------------------------------------------------------------
void host_instance_boxes(const double* local_boxes, int local_stride, const double* instances, int stride, uint64_t n, double* boxes_out) {
    for (uint64_t i = 0; i < n; ++i)
        aabb_transform_core(local_boxes + i * (uint64_t)local_stride, instances + i * (uint64_t)stride, boxes_out + 6 * i);
}

void host_frustum_boxes(const double planes[24], const double* boxes, uint64_t n, bool merge, uint8_t* codes) {
    for (uint64_t i = 0; i < n; ++i) {
        if (!frustum_intersects_core(planes, boxes + 6 * i)) codes[i] = TRGL_OCCL_OUTSIDE;
        else if (!merge) codes[i] = TRGL_OCCL_VISIBLE;
    }
}
}  // namespace trgl
using namespace trgl;

extern "C" {

void trgl_ssao_defaults(trgl_ssao_params* p) {      // main.cpp:317-321
    if (!p) return;
    p->num_directions = 8; p->steps_per_direction = 8; p->sample_radius = 16.0; p->occlusion_threshold = 1e-3; p->intensity = 0.35;
}

int trgl_format_stats(const trgl_stats* s, char* buf, size_t buflen) {   // our_gl.cpp:205-209
    if (!s || !buf) return TRGL_E_INVALID;
    char lo[400], hi[400];      // "%f" of a double needs up to 317 characters
    if (std::isfinite(s->min_z)) std::snprintf(lo, sizeof lo, "%f", s->min_z); else std::snprintf(lo, sizeof lo, "inf");
    if (std::isfinite(s->max_z)) std::snprintf(hi, sizeof hi, "%f", s->max_z); else std::snprintf(hi, sizeof hi, "-inf");
    int n = std::snprintf(buf, buflen, "DEBUG: triangles=%llu fragments_drawn=%llu bbox=[%d,%d] - [%d,%d] z-range=[%s,%s]\n",
                          (unsigned long long)s->triangles_rasterized, (unsigned long long)s->fragments_drawn,
                          s->min_x, s->min_y, s->max_x, s->max_y, lo, hi);
    return (n < 0 || (size_t)n >= buflen) ? TRGL_E_INVALID : TRGL_OK;
}

int trgl_aabb_transform(const double bmin[3], const double bmax[3], const double m[16], double out_min[3], double out_max[3]) {
    if (!bmin || !bmax || !m || !out_min || !out_max) return TRGL_E_INVALID;
    const double box[6] = { bmin[0], bmin[1], bmin[2], bmax[0], bmax[1], bmax[2] };
    double out[6];
    aabb_transform_core(box, m, out);                                           // geometry.h:297-327
    for (int a = 0; a < 3; ++a) { out_min[a] = out[a]; out_max[a] = out[3 + a]; }
    return TRGL_OK;
}

int trgl_frustum_from_matrix(const double m[16], double planes[24]) {
    if (!m || !planes) return TRGL_E_INVALID;
    for (int pair = 0; pair < 3; ++pair)                                        // our_gl.cpp:217-250: LEFT/RIGHT with k = 0, BOTTOM/TOP 1, NEAR/FAR 2
        for (int side = 0; side < 2; ++side) {
            double* pl = planes + 4 * (2 * pair + side);
            for (int row = 0; row < 4; ++row)                                   // rows 0..2 give the normal, row 3 gives d
                pl[row] = side == 0 ? m[4 * row + 3] + m[4 * row + pair] : m[4 * row + 3] - m[4 * row + pair];
        }
    for (int i = 0; i < 6; ++i) {                                               // :253-259
        double* pl = planes + 4 * i;
        const double length = std::sqrt(dot3_from_zero(pl, pl[0], pl[1], pl[2]));
        if (length > 0.0) { pl[0] = pl[0] / length; pl[1] = pl[1] / length; pl[2] = pl[2] / length; pl[3] /= length; }
    }
    return TRGL_OK;
}

int trgl_frustum_intersects(const double planes[24], const double bmin[3], const double bmax[3]) {
    if (!planes || !bmin || !bmax) return TRGL_E_INVALID;
    const double box[6] = { bmin[0], bmin[1], bmin[2], bmax[0], bmax[1], bmax[2] };
    return frustum_intersects_core(planes, box) ? 1 : 0;                        // our_gl.cpp:264-280
}

int trgl_clip_layout(int kind, trgl_clip_attr* attrs, int* n_attrs) {
    static const trgl_clip_attr gouraud[] = { { 0, 1 } };
    static const trgl_clip_attr phong[] = { { 0, 2 }, { 6, 3 }, { 15, 3 } };      // uv[3], position_eye[3], normal_eye[3] (main.cpp:47-49)
    if (!n_attrs) return fail(nullptr, TRGL_E_INVALID, "trgl_clip_layout: n_attrs is null");
    const trgl_clip_attr* src = nullptr; int n = 0;
    switch (kind) {
    case TRGL_SHADER_FLAT: case TRGL_SHADER_CHECKER: break;
    case TRGL_SHADER_GOURAUD: src = gouraud; n = 1; break;
    case TRGL_SHADER_PHONG: case TRGL_SHADER_EYE: src = phong; n = 3; break;
    default: return fail(nullptr, TRGL_E_INVALID, "trgl_clip_layout: not a built-in shader kind");
    }
    for (int a = 0; attrs && a < n; ++a) attrs[a] = src[a];
    *n_attrs = n;
    return TRGL_OK;
}

int trgl_mip_layout(int w, int h, int bpp, int* levels, int widths[TRGL_MAX_MIP_LEVELS], int heights[TRGL_MAX_MIP_LEVELS],
                    size_t offsets[TRGL_MAX_MIP_LEVELS], size_t* total) {
    if (w < 1 || h < 1 || !(bpp == 1 || bpp == 3 || bpp == 4)) return fail(nullptr, TRGL_E_INVALID, "trgl_mip_layout: need w, h >= 1 and bpp in {1, 3, 4}");
    if (w > 65535 || h > 65535) return fail(nullptr, TRGL_E_UNSUPPORTED, "trgl_mip_layout: a side above 65535");
    if ((int64_t)w * h * bpp > 0x7fffffff) return fail(nullptr, TRGL_E_UNSUPPORTED, "trgl_mip_layout: w * h * bpp above INT_MAX");
    const int L = mip_levels(w, h);
    if (levels) *levels = L;
    for (int l = 0; l < TRGL_MAX_MIP_LEVELS; ++l) {
        if (widths) widths[l] = l < L ? mip_side(w, l) : 0;
        if (heights) heights[l] = l < L ? mip_side(h, l) : 0;
        if (offsets) offsets[l] = (l >= 1 && l < L) ? mip_packed_offset(w, h, bpp, l) : 0;
    }
    if (total) *total = mip_packed_offset(w, h, bpp, L);
    return TRGL_OK;
}

int trgl_image_sample(const uint8_t* level0, const uint8_t* chain, int w, int h, int bpp, int levels,
                      const double* uv, const double* lod, int mode, uint64_t n, uint8_t* out) {
    if (int r = trgl_mip_layout(w, h, bpp, nullptr, nullptr, nullptr, nullptr, nullptr)) return r;
    if (mode < 0 || mode > 2 || levels < 1) return fail(nullptr, TRGL_E_INVALID, "trgl_image_sample: need mode in 0..2 and levels >= 1");
    if (n == 0) return TRGL_OK;
    if (!level0 || !uv || !lod || !out) return fail(nullptr, TRGL_E_INVALID, "trgl_image_sample: null argument");
    const int L = std::min(levels, mip_levels(w, h));
    if (L > 1 && !chain) return fail(nullptr, TRGL_E_INVALID, "trgl_image_sample: chain is null");
    const MipView v{ level0, chain, w, h, bpp, L, false };
    for (uint64_t i = 0; i < n; ++i) {
        const MipTexel c = mip_sample_mode(v, uv + 2 * i, lod[i], mode);
        for (int k = 0; k < 4; ++k) out[5 * i + k] = (uint8_t)(c.bgra >> (8 * k));
        out[5 * i + 4] = (uint8_t)c.bytespp;
    }
    return TRGL_OK;
}

int trgl_selftest_mip_lod(const double* bar, const double* k, int tex_w, int tex_h, uint64_t n, double* out) {
    if (n && (!bar || !k || !out)) return fail(nullptr, TRGL_E_INVALID, "trgl_selftest_mip_lod: null argument");
    for (uint64_t i = 0; i < n; ++i) out[i] = mip_lod(bar + 3 * i, k + 4 * i, tex_w, tex_h);
    return TRGL_OK;
}

int trgl_gaussian_kernel(int radius, float* weights) {      // TGAImage::gaussian_blur's weights (tgaimage.cpp:271-324)
    if (radius <= 0 || !weights) return fail(nullptr, TRGL_E_INVALID, "trgl_gaussian_kernel: need radius >= 1 and room for 2 * radius + 1 weights");
    if (radius > TRGL_MAX_BLUR_RADIUS) return fail(nullptr, TRGL_E_UNSUPPORTED, "trgl_gaussian_kernel: radius above 46340 (i * i overflows the reference's int)");
    trgl_image::gaussian_weights(radius, weights);
    return TRGL_OK;
}

int trgl_shadow_matrix(const double light_mv[16], const double light_proj[16], const double light_vp[16],
                       const double cam_mv[16], const double cam_proj[16], const double cam_vp[16], double out[16]) {
    if (!light_mv || !light_proj || !light_vp || !cam_mv || !cam_proj || !cam_vp || !out)
        return fail(nullptr, TRGL_E_INVALID, "trgl_shadow_matrix: null matrix");
    auto mul = [](const double* a, const double* b, double* r) { mat4_mul(a, b, r); };      // geometry.h:196-205 (skin_core.h)
    double t[16], L[16], Cm[16], inv[16];
    mul(light_vp, light_proj, t); mul(t, light_mv, L);                               // Viewport * Perspective * ModelView, left to right
    mul(cam_vp, cam_proj, t); mul(t, cam_mv, Cm);
    // Gauss-Jordan with partial pivoting on [Cm | I]
    for (int i = 0; i < 16; ++i) inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(Cm[4 * r + col]) > std::fabs(Cm[4 * piv + col])) piv = r;
        const double pv = Cm[4 * piv + col];
        if (pv == 0.0 || !std::isfinite(pv)) return fail(nullptr, TRGL_E_INVALID, "trgl_shadow_matrix: the camera's matrix is singular (a pivot is 0 or not finite)");
        if (piv != col)
            for (int k = 0; k < 4; ++k) { std::swap(Cm[4 * piv + k], Cm[4 * col + k]); std::swap(inv[4 * piv + k], inv[4 * col + k]); }
        for (int k = 0; k < 4; ++k) { Cm[4 * col + k] /= pv; inv[4 * col + k] /= pv; }
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = Cm[4 * r + col];
            for (int k = 0; k < 4; ++k) { Cm[4 * r + k] -= f * Cm[4 * col + k]; inv[4 * r + k] -= f * inv[4 * col + k]; }
        }
    }
    mul(L, inv, t);
    std::memcpy(out, t, sizeof(t));
    return TRGL_OK;
}

int trgl_obj_load(const char* path, double** vertices, uint64_t* n_vertices, uint32_t** indices, uint64_t* n_faces) {
    if (!path || !vertices || !n_vertices || !indices || !n_faces) return TRGL_E_INVALID;
    trgl_obj::Mesh m;
    try {
        if (!trgl_obj::load(path, m)) return fail(nullptr, TRGL_E_INVALID, m.error);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, TRGL_E_NOMEM, "trgl_obj_load: out of memory");
    }
    *n_vertices = m.vertices.size() / 14; *n_faces = m.indices.size() / 3;
    *vertices = (double*)std::malloc(m.vertices.size() * sizeof(double) + 8);
    *indices = (uint32_t*)std::malloc(m.indices.size() * sizeof(uint32_t) + 8);
    if (!*vertices || !*indices) { std::free(*vertices); std::free(*indices); return TRGL_E_NOMEM; }
    std::memcpy(*vertices, m.vertices.data(), m.vertices.size() * sizeof(double));
    std::memcpy(*indices, m.indices.data(), m.indices.size() * sizeof(uint32_t));
    return TRGL_OK;
}
void trgl_obj_free(double* vertices, uint32_t* indices) { std::free(vertices); std::free(indices); }

size_t trgl_tga_max_size(int w, int h, int bpp) {
    if (w <= 0 || h <= 0 || bpp <= 0) return 18;
    return size_t(18) + size_t(w) * h * bpp + size_t(w) * h;      // every pixel its own literal packet
}

int trgl_tga_encode(const uint8_t* pixels, int w, int h, int bpp, int vflip, int rle, uint8_t* out, size_t* out_len) {
    if (!pixels || !out || !out_len || w <= 0 || h <= 0 || w > 65535 || h > 65535 || !(bpp == 1 || bpp == 3 || bpp == 4)) return TRGL_E_INVALID;
    try {
        TGAImage img(w, h, bpp);
        std::memcpy(img.buffer(), pixels, size_t(w) * h * bpp);
        std::vector<uint8_t> bytes = img.encode_tga(vflip != 0, rle != 0);
        std::memcpy(out, bytes.data(), bytes.size());
        *out_len = bytes.size();
    } catch (const std::bad_alloc&) {
        return TRGL_E_NOMEM;
    }
    return TRGL_OK;
}

int trgl_tga_info(const uint8_t* file, size_t size, int* width, int* height, int* bpp) {
    if (!file || !width || !height || !bpp || size < 18) return TRGL_E_INVALID;            // tgaimage.cpp:85-90
    const int w = file[12] | (file[13] << 8), h = file[14] | (file[15] << 8), b = file[16] >> 3;
    if (w <= 0 || h <= 0 || (b != 1 && b != 3 && b != 4)) return TRGL_E_INVALID;           // :96-99
    if (!(file[2] == 2 || file[2] == 3 || file[2] == 10 || file[2] == 11)) return TRGL_E_INVALID;   // :113-116
    *width = w; *height = h; *bpp = b;
    return TRGL_OK;
}

int trgl_tga_decode(const uint8_t* file, size_t size, uint8_t* pixels) {
    if (!file || !pixels) return TRGL_E_INVALID;
    try {                                          // a header may claim 65535 x 65535 x 4 bytes: nothing throws across the C ABI
        TGAImage img;
        if (!img.decode_tga(file, size)) return TRGL_E_INVALID;
        std::memcpy(pixels, img.buffer(), size_t(img.width()) * img.height() * img.bytespp());
    } catch (const std::bad_alloc&) {
        return TRGL_E_NOMEM;
    }
    return TRGL_OK;
}

}  // extern "C"
