// edge_core.h — the definitions of trgl_mesh_edges and trgl_edge_select (include/trgl.h, "mesh edges") as the functions that the host
// loops (trgl_host.cpp) and the kernels (kernels_edge.hip) both compile: the sort key of a half-edge, the facing and the unit normal
// of a face, the code byte of an edge and the colour of a selected one.
// fp64, every operation rounded, contraction off.  No double computed here is stored: only comparisons leave, so NaN payloads do not matter.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_EDGE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_EDGE_HD inline
#endif

namespace trgl {

constexpr uint32_t EDGE_NONE = 0xFFFFFFFFu;      // every word of a "no edge" record, f1 of a boundary edge, both words of a "no edge" segment

// bits of the largest vertex number (at least 1, at most 32: an index has no more)
TRGL_EDGE_HD int edge_index_bits(uint64_t n_vertices) {
    const uint64_t top = n_vertices < 2 ? 1 : (n_vertices - 1 > 0xFFFFFFFFull ? 0xFFFFFFFFull : n_vertices - 1);
    int bits = 1;
    while (bits < 32 && (top >> bits)) ++bits;
    return bits;
}
// The sort key of a half-edge (a, b) over `bits` = edge_index_bits(n_vertices): lo in the upper `bits` bits, hi in the lower ones, so
// keys ascend with (lo, hi) and a sort over 2 * bits bits orders them.  "No edge" (a == b, or an index >= n_vertices) is all ones in
// those 2 * bits bits: lo == hi is no edge's key, and every key of an edge is smaller.
TRGL_EDGE_HD uint64_t edge_key_none(int bits) { return bits == 32 ? ~0ull : (1ull << (2 * bits)) - 1ull; }
TRGL_EDGE_HD uint64_t edge_key(uint32_t a, uint32_t b, uint64_t n_vertices, int bits) {
    if (a == b || a >= n_vertices || b >= n_vertices) return edge_key_none(bits);
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return ((uint64_t)lo << bits) | (uint64_t)hi;
}
TRGL_EDGE_HD uint32_t edge_key_lo(uint64_t key, int bits) { return (uint32_t)(key >> bits); }
TRGL_EDGE_HD uint32_t edge_key_hi(uint64_t key, int bits) { return (uint32_t)(key & (bits == 32 ? 0xFFFFFFFFull : (1ull << bits) - 1ull)); }

// What trgl_edge_select needs of a face: whether it faces the eye, and its unit normal
struct EdgeFace { bool front; double u[3]; };

// p0, p1, p2: the positions of the face's vertices in index order
TRGL_EDGE_HD EdgeFace edge_face(const double* p0, const double* p1, const double* p2, const double eye[4]) {
    double e1[3], e2[3], n[3], d[3];
    for (int a = 0; a < 3; ++a) { e1[a] = p1[a] - p0[a]; e2[a] = p2[a] - p0[a]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];                                   // geometry.h:143-149, as model.cpp:293-299 calls it
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    for (int a = 0; a < 3; ++a) { const double t = eye[3] * p0[a]; d[a] = eye[a] - t; }
    double s = 0.0;
    s += n[0] * d[0]; s += n[1] * d[1]; s += n[2] * d[2];
    EdgeFace f;
    f.front = s > 0.0;                                                      // (a NaN is not front)
    double sum = 0.0;
    sum += n[0] * n[0]; sum += n[1] * n[1]; sum += n[2] * n[2];
    const double length = sqrt(sum);                                        // normalized(), geometry.h:136-140
    const bool zero = length == 0.0;
    for (int a = 0; a < 3; ++a) f.u[a] = zero ? n[a] : n[a] / length;
    return f;
}

// the code byte of an edge between faces f0 and (has1) f1
TRGL_EDGE_HD uint8_t edge_code(const EdgeFace& f0, bool has1, const EdgeFace& f1, double crease_cos) {
    uint32_t code = TRGL_EDGE_ANY;
    if (!has1) return (uint8_t)(code | TRGL_EDGE_BOUNDARY);
    if (f0.front != f1.front) code |= TRGL_EDGE_SILHOUETTE;
    double dot = 0.0;
    dot += f0.u[0] * f1.u[0]; dot += f0.u[1] * f1.u[1]; dot += f0.u[2] * f1.u[2];
    if (dot < crease_cos) code |= TRGL_EDGE_CREASE;                         // (a NaN is no crease)
    return (uint8_t)code;
}

// class_color of the lowest set bit of code & select (sel != 0)
TRGL_EDGE_HD uint32_t edge_color(const uint32_t class_color[4], uint32_t sel) {
    return class_color[(sel & 1u) ? 0 : (sel & 2u) ? 1 : (sel & 4u) ? 2 : 3];
}

}  // namespace trgl
