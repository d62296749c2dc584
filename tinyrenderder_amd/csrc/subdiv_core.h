// subdiv_core.h — the definitions of trgl_subdiv_topology and trgl_subdiv_vertices (include/trgl.h, "mesh subdivision") as the functions
// that the host loops (trgl_host.cpp) and the kernels (kernels_subdiv.hip) both compile: the lookup of an edge by its pair, the corner of a
// face opposite an edge, what makes a record or a stencil word usable, Warren's beta and the four vertex rules.
// fp64, every operation rounded, contraction off.  A computed double that is a NaN is stored canonical; a copied one keeps its bits.
#pragma once
#include <stdint.h>

#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_SUBDIV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_SUBDIV_HD inline
#endif

namespace trgl {

constexpr uint32_t SUBDIV_NONE = 0xFFFFFFFFu;

// ---- the table (trgl_subdiv_topology) ----
// (lo, hi) of a pair or of a record as one number: records ascend in it, and the all-ones words of a "no edge" record lie behind every edge
TRGL_SUBDIV_HD uint64_t subdiv_pair_key(uint32_t lo, uint32_t hi) { return ((uint64_t)lo << 32) | (uint64_t)hi; }

// The number of the first of n_edges records whose (lo, hi) is not below `key`, by halving [0, n_edges) - n_edges when there is none.
// The header states this search: over records that do not ascend it still ends, at the record the halving reaches.
TRGL_SUBDIV_HD uint64_t subdiv_lower_bound(const uint32_t* edges, uint64_t n_edges, uint64_t key) {
    uint64_t first = 0, last = n_edges;
    while (first < last) {
        const uint64_t mid = (first + last) >> 1;
        if (subdiv_pair_key(edges[4 * mid], edges[4 * mid + 1]) < key) first = mid + 1; else last = mid;
    }
    return first;
}
// e(a, b): the record that names the pair of a and b (a != b), or n_edges
TRGL_SUBDIV_HD uint64_t subdiv_find_edge(const uint32_t* edges, uint64_t n_edges, uint32_t a, uint32_t b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const uint64_t e = subdiv_lower_bound(edges, n_edges, subdiv_pair_key(lo, hi));
    return (e < n_edges && edges[4 * e] == lo && edges[4 * e + 1] == hi) ? e : n_edges;
}

// The corner of the face (i0, i1, i2) opposite the edge (lo, hi): the index behind the lowest half-edge that joins the two.  false: the
// face does not hold the pair, or names a vertex >= n_vertices
TRGL_SUBDIV_HD bool subdiv_opposite(const uint32_t* face, uint32_t lo, uint32_t hi, uint64_t n_vertices, uint32_t* corner) {
    const uint32_t i[3] = { face[0], face[1], face[2] };
    if (i[0] >= n_vertices || i[1] >= n_vertices || i[2] >= n_vertices) return false;
    for (int k = 0; k < 3; ++k) {
        const uint32_t a = i[k], b = i[k == 2 ? 0 : k + 1];
        if ((a == lo && b == hi) || (a == hi && b == lo)) { *corner = i[k == 0 ? 2 : k - 1]; return true; }
    }
    return false;
}

// The odd stencil {lo, hi, o0, o1} of the record rec = {lo, hi, f0, f1}.  SUBDIV_REC_NONE: a "no edge" record (f0 is none), four NONE
// words; SUBDIV_REC_BAD: an inconsistent one - the host refuses it, the device writes four NONE words as well.
enum { SUBDIV_REC_EDGE = 0, SUBDIV_REC_NONE = 1, SUBDIV_REC_BAD = 2 };
TRGL_SUBDIV_HD int subdiv_odd_stencil(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t rec[4], uint32_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = SUBDIV_NONE;
    const uint32_t lo = rec[0], hi = rec[1], f0 = rec[2], f1 = rec[3];
    if (f0 == SUBDIV_NONE) return SUBDIV_REC_NONE;
    if (lo >= hi || hi >= n_vertices || f0 >= n_faces || (f1 != SUBDIV_NONE && f1 >= n_faces)) return SUBDIV_REC_BAD;
    uint32_t o0 = SUBDIV_NONE, o1 = SUBDIV_NONE;
    if (!subdiv_opposite(indices + 3 * (uint64_t)f0, lo, hi, n_vertices, &o0)) return SUBDIV_REC_BAD;
    if (f1 != SUBDIV_NONE && !subdiv_opposite(indices + 3 * (uint64_t)f1, lo, hi, n_vertices, &o1)) return SUBDIV_REC_BAD;
    const bool boundary = f1 == SUBDIV_NONE || f1 == f0;
    out[0] = lo; out[1] = hi; out[2] = boundary ? SUBDIV_NONE : o0; out[3] = boundary ? SUBDIV_NONE : o1;
    return SUBDIV_REC_EDGE;
}

// (b0, b1) of an even record from the number of boundary edges at the vertex and the first two of them in ring order
TRGL_SUBDIV_HD void subdiv_boundary_pair(uint32_t v, uint32_t n_boundary, uint32_t first, uint32_t second, uint32_t* b0, uint32_t* b1) {
    if (n_boundary == 0) { *b0 = SUBDIV_NONE; *b1 = SUBDIV_NONE; }
    else if (n_boundary == 2) { *b0 = first; *b1 = second; }
    else { *b0 = v; *b1 = v; }
}

// ---- the stencil words (trgl_subdiv_vertices) ----
// What an odd stencil asks for.  ZERO: the record of a "no edge" stencil; BAD: a word names no vertex (the host refuses, the device
// writes the zero record); MID: the midpoint of lo and hi in every double; FULL: the four-point rule in the smooth doubles
enum { SUBDIV_ODD_ZERO = 0, SUBDIV_ODD_BAD = 1, SUBDIV_ODD_MID = 2, SUBDIV_ODD_FULL = 3 };
TRGL_SUBDIV_HD int subdiv_odd_class(const uint32_t st[4], uint64_t n_vertices) {
    if (st[0] == SUBDIV_NONE && st[1] == SUBDIV_NONE && st[2] == SUBDIV_NONE && st[3] == SUBDIV_NONE) return SUBDIV_ODD_ZERO;
    if (st[0] >= n_vertices || st[1] >= n_vertices) return SUBDIV_ODD_BAD;
    if (st[2] == SUBDIV_NONE && st[3] == SUBDIV_NONE) return SUBDIV_ODD_MID;
    if (st[2] >= n_vertices || st[3] >= n_vertices) return SUBDIV_ODD_BAD;
    return SUBDIV_ODD_FULL;
}
// What the even stencil {begin, count, b0, b1} of vertex v asks for, ring entries apart.  COPY: an isolated vertex or a corner; BAD: a
// word out of range (the host refuses, the device copies); RING: the interior rule over ring[begin .. begin + count), whose entries must
// name vertices; EDGE: the boundary rule with b0 and b1
enum { SUBDIV_EVEN_COPY = 0, SUBDIV_EVEN_BAD = 1, SUBDIV_EVEN_RING = 2, SUBDIV_EVEN_EDGE = 3 };
TRGL_SUBDIV_HD int subdiv_even_class(const uint32_t st[4], uint32_t v, uint64_t n_vertices, uint64_t n_edges) {
    const uint64_t begin = st[0], count = st[1];
    if (begin + count > 2 * n_edges) return SUBDIV_EVEN_BAD;
    if (st[2] == SUBDIV_NONE && st[3] == SUBDIV_NONE) return count ? SUBDIV_EVEN_RING : SUBDIV_EVEN_COPY;
    if (st[2] >= n_vertices || st[3] >= n_vertices) return SUBDIV_EVEN_BAD;
    return (st[2] == v && st[3] == v) ? SUBDIV_EVEN_COPY : SUBDIV_EVEN_EDGE;
}

// ---- the arithmetic ----
TRGL_SUBDIV_HD double subdiv_canon(double x) {
    if (x == x) return x;
    const uint64_t b = 0x7FF8000000000000ull;
    double r; __builtin_memcpy(&r, &b, sizeof(r));
    return r;
}
// Warren's weight of a ring entry at an interior vertex of valence `count`
TRGL_SUBDIV_HD double subdiv_beta(uint32_t count) { return count <= 3 ? 0.1875 : 3.0 / (8.0 * (double)count); }
TRGL_SUBDIV_HD double subdiv_midpoint(double x_lo, double x_hi) { return subdiv_canon(0.5 * (x_lo + x_hi)); }
TRGL_SUBDIV_HD double subdiv_odd_interior(double x_lo, double x_hi, double x_o0, double x_o1) {
    const double s = x_lo + x_hi, t = x_o0 + x_o1;
    const double p = 0.375 * s, q = 0.125 * t;
    return subdiv_canon(p + q);
}
// ring_sum: +0.0 plus x of every ring entry in ring order
TRGL_SUBDIV_HD double subdiv_even_interior(uint32_t count, double x_v, double ring_sum) {
    const double beta = subdiv_beta(count);
    const double a = 1.0 - (double)count * beta;
    const double p = a * x_v, q = beta * ring_sum;
    return subdiv_canon(p + q);
}
TRGL_SUBDIV_HD double subdiv_even_boundary(double x_v, double x_b0, double x_b1) {
    const double p = 0.75 * x_v, q = 0.125 * (x_b0 + x_b1);
    return subdiv_canon(p + q);
}

}  // namespace trgl
