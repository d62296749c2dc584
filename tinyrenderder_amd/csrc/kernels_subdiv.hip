// kernels_subdiv.hip — one level of triangle-mesh subdivision, Loop and linear (include/trgl.h: trgl_subdiv_topology,
// trgl_subdiv_vertices and trgl_draw_subdivided), gfx950.  The table's rules and the arithmetic are subdiv_core.h's.
//
// trgl_subdiv_topology, once per mesh:
//   k_subdiv_odd     : one lane per edge record: its odd stencil {lo, hi, o0, o1} from the two faces' indices (subdiv_odd_stencil), and
//                      two sort entries, keys lo and hi with values 2 e and 2 e + 1 - key n_vertices, behind every vertex, for a record
//                      that is no edge.
//   the sort         : hipcub::DeviceRadixSort::SortPairs over the bits of n_vertices - stable, so a vertex's entries stay in ascending e
//                      and its first entry's position is already `begin`: no scan.
//   k_subdiv_ring    : one lane per sorted entry: the other endpoint of its edge, NONE behind the last used one.
//   k_subdiv_even    : one lane per vertex: the ends of its run by two halvings of the sorted keys, then a walk of the run for the
//                      boundary pair (the longest walk is the mesh's largest valence; once per mesh).
//   k_subdiv_indices : one lane per face: e(a, b) by halving the records (subdiv_find_edge), which serves fan edges as f0 / f1 cannot; a
//                      record counts only where its odd stencil was written as an edge.
// trgl_subdiv_vertices, every frame:
//   k_subdiv_vertices: one launch over the (n_vertices + n_edges) * stride doubles of the output, even records first.  Consecutive lanes
//                      take consecutive doubles, so a record's lanes read the same stencil (one request) and consecutive doubles of each
//                      neighbour's record, and a wave stores 512 contiguous bytes.  A ring is walked in order by every lane of its record:
//                      parallel over doubles and vertices, never over the ring.  A lane divides once, for its first double.
// No atomic anywhere.  Every index, face number and stencil word is compared with its count before it becomes an address.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "launch.h"
#include "edge_core.h"
#include "subdiv_core.h"

namespace {

using namespace trgl;

__host__ __device__ inline bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }
// four words at a 4-byte aligned address; wide: the array is 16-byte aligned (the same for every lane)
__device__ __forceinline__ void store_words4(uint32_t* p, bool wide, const uint32_t w[4]) {
    if (wide) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else { p[0] = w[0]; p[1] = w[1]; p[2] = w[2]; p[3] = w[3]; }
}
__device__ __forceinline__ void load_words4(const uint32_t* p, bool wide, uint32_t w[4]) {
    if (wide) { const uint4 v = *reinterpret_cast<const uint4*>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else { w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; w[3] = p[3]; }
}

__global__ __launch_bounds__(SUBDIV_BLOCK) void k_subdiv_odd(const uint32_t* __restrict__ indices, uint64_t n_faces, uint64_t n_vertices,
                                                             const uint32_t* __restrict__ edges, uint32_t n_edges, uint32_t* __restrict__ odd,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ values) {
    const uint32_t e = blockIdx.x * SUBDIV_BLOCK + threadIdx.x;
    if (e >= n_edges) return;
    uint32_t rec[4], st[4];
    load_words4(edges + 4 * (size_t)e, aligned_to(edges, 16), rec);
    const bool edge = subdiv_odd_stencil(indices, n_faces, n_vertices, rec, st) == SUBDIV_REC_EDGE;
    store_words4(odd + 4 * (size_t)e, aligned_to(odd, 16), st);
    keys[2 * (size_t)e] = edge ? st[0] : (uint32_t)n_vertices;
    keys[2 * (size_t)e + 1] = edge ? st[1] : (uint32_t)n_vertices;
    values[2 * (size_t)e] = 2u * e;
    values[2 * (size_t)e + 1] = 2u * e + 1u;
}

__global__ __launch_bounds__(SUBDIV_BLOCK) void k_subdiv_ring(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ values, uint32_t n,
                                                              uint64_t n_vertices, const uint32_t* __restrict__ odd, uint32_t* __restrict__ ring) {
    const uint32_t i = blockIdx.x * SUBDIV_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t other = SUBDIV_NONE;
    if (keys[i] < n_vertices) { const uint32_t val = values[i]; other = odd[4 * (size_t)(val >> 1) + (1u - (val & 1u))]; }      // (val < n: made by k_subdiv_odd)
    ring[i] = other;
}

// the first of n ascending keys that is not below `key`
__device__ __forceinline__ uint32_t first_not_below(const uint32_t* __restrict__ keys, uint32_t n, uint64_t key) {
    uint32_t first = 0, last = n;
    while (first < last) {
        const uint32_t mid = first + ((last - first) >> 1);
        if (keys[mid] < key) first = mid + 1; else last = mid;
    }
    return first;
}

__global__ __launch_bounds__(SUBDIV_BLOCK) void k_subdiv_even(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ values, uint32_t n,
                                                              uint32_t n_vertices, const uint32_t* __restrict__ odd, uint32_t* __restrict__ even) {
    const uint32_t v = blockIdx.x * SUBDIV_BLOCK + threadIdx.x;
    if (v >= n_vertices) return;
    const uint32_t lb = first_not_below(keys, n, v), ub = first_not_below(keys, n, (uint64_t)v + 1);
    uint32_t nb = 0, first = 0, second = 0;
    for (uint32_t i = lb; i < ub; ++i) {
        const uint32_t val = values[i];
        const uint32_t* st = odd + 4 * (size_t)(val >> 1);
        if (st[2] != SUBDIV_NONE) continue;
        const uint32_t other = st[1u - (val & 1u)];
        if (nb == 0) first = other; else if (nb == 1) second = other;
        ++nb;
    }
    uint32_t rec[4] = { ub > lb ? lb : 0u, ub - lb, 0u, 0u };
    subdiv_boundary_pair(v, nb, first, second, rec + 2, rec + 3);
    store_words4(even + 4 * (size_t)v, aligned_to(even, 16), rec);
}

__global__ __launch_bounds__(SUBDIV_BLOCK) void k_subdiv_indices(const uint32_t* __restrict__ indices, uint32_t n_faces, uint64_t n_vertices,
                                                                 const uint32_t* __restrict__ edges, uint32_t n_edges,
                                                                 const uint32_t* __restrict__ odd, uint32_t* __restrict__ out) {
    const uint32_t f = blockIdx.x * SUBDIV_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t a = indices[3 * (size_t)f], b = indices[3 * (size_t)f + 1], c = indices[3 * (size_t)f + 2];
    uint32_t w[12] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    if (a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a) {
        const uint64_t ab = subdiv_find_edge(edges, n_edges, a, b), bc = subdiv_find_edge(edges, n_edges, b, c),
                       ca = subdiv_find_edge(edges, n_edges, c, a);
        // (a record that k_subdiv_odd found inconsistent names no pair)
        if (ab < n_edges && bc < n_edges && ca < n_edges && odd[4 * ab] != SUBDIV_NONE && odd[4 * bc] != SUBDIV_NONE && odd[4 * ca] != SUBDIV_NONE) {
            const uint32_t m_ab = (uint32_t)(n_vertices + ab), m_bc = (uint32_t)(n_vertices + bc), m_ca = (uint32_t)(n_vertices + ca);
            w[0] = a; w[1] = m_ab; w[2] = m_ca;  w[3] = b; w[4] = m_bc; w[5] = m_ab;  w[6] = c; w[7] = m_ca; w[8] = m_bc;
            w[9] = m_ab; w[10] = m_bc; w[11] = m_ca;
        }
    }
    uint32_t* o = out + 12 * (size_t)f;
    const bool wide = aligned_to(out, 16);      // (48 bytes per face: every face is as aligned as the array)
    store_words4(o, wide, w); store_words4(o + 4, wide, w + 4); store_words4(o + 8, wide, w + 8);
}

// One double of the output: record `rec`, double `d` of it
__device__ __forceinline__ double subdiv_value(const SubdivVertexArgs& a, uint64_t rec, uint32_t d, bool wide) {
    const uint64_t V = a.n_vertices, S = a.stride;
    const double* __restrict__ x = a.vertices;
    uint32_t st[4];
    if (rec < V) {
        const double xv = x[rec * S + d];
        if (d >= a.smooth) return xv;
        load_words4(a.stencils + 4 * (size_t)(a.n_edges + rec), wide, st);
        const int kind = subdiv_even_class(st, (uint32_t)rec, V, a.n_edges);
        if (kind == SUBDIV_EVEN_EDGE) return subdiv_even_boundary(xv, x[(uint64_t)st[2] * S + d], x[(uint64_t)st[3] * S + d]);
        if (kind != SUBDIV_EVEN_RING) return xv;
        const uint32_t* __restrict__ ring = a.stencils + 4 * (size_t)(a.n_edges + V) + st[0];
        double sum = 0.0;
        bool named = true;
        for (uint32_t k = 0; k < st[1]; ++k) {
            const uint32_t n = ring[k];
            if (n < V) sum += x[(uint64_t)n * S + d]; else named = false;
        }
        return named ? subdiv_even_interior(st[1], xv, sum) : xv;
    }
    load_words4(a.stencils + 4 * (size_t)(rec - V), wide, st);
    const int kind = subdiv_odd_class(st, V);
    if (kind == SUBDIV_ODD_ZERO || kind == SUBDIV_ODD_BAD) return 0.0;
    const double xl = x[(uint64_t)st[0] * S + d], xh = x[(uint64_t)st[1] * S + d];
    if (kind == SUBDIV_ODD_FULL && d < a.smooth) return subdiv_odd_interior(xl, xh, x[(uint64_t)st[2] * S + d], x[(uint64_t)st[3] * S + d]);
    return subdiv_midpoint(xl, xh);
}

__global__ __launch_bounds__(SUBDIV_BLOCK) void k_subdiv_vertices(const SubdivVertexArgs a) {
    const uint64_t total = (a.n_vertices + a.n_edges) * (uint64_t)a.stride;
    uint64_t g = (uint64_t)blockIdx.x * (SUBDIV_BLOCK * SUBDIV_ITEMS) + threadIdx.x;
    if (g >= total) return;
    uint64_t rec = g / a.stride;
    uint32_t d = (uint32_t)(g - rec * a.stride);
    const bool wide = aligned_to(a.stencils, 16);
#pragma unroll
    for (int k = 0; k < SUBDIV_ITEMS; ++k) {
        if (g < total) a.out[g] = subdiv_value(a, rec, d, wide);
        g += SUBDIV_BLOCK; rec += a.step_q; d += a.step_r;      // SUBDIV_BLOCK = step_q * stride + step_r
        if (d >= a.stride) { d -= a.stride; ++rec; }
    }
}

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
unsigned num_blocks(uint64_t n) { return (unsigned)((n + SUBDIV_BLOCK - 1) / SUBDIV_BLOCK); }

struct Carve { uint32_t* keys; uint32_t* sorted_keys; uint32_t* values; uint32_t* sorted_values; size_t sort_off; };
Carve carve(void* scratch, uint64_t n_edges) {
    char* p = (char*)scratch;
    const size_t words = align256(2 * (size_t)n_edges * sizeof(uint32_t));
    Carve c;
    c.keys = (uint32_t*)p; c.sorted_keys = (uint32_t*)(p + words); c.values = (uint32_t*)(p + 2 * words); c.sorted_values = (uint32_t*)(p + 3 * words);
    c.sort_off = 4 * words;
    return c;
}
// the bits of the largest key, n_vertices itself
int key_bits(uint64_t n_vertices) { return edge_index_bits(n_vertices + 1); }
hipError_t sort_entries(void* tmp, size_t& tmp_bytes, const Carve& c, uint64_t n_edges, uint64_t n_vertices, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t*)c.keys, c.sorted_keys, (const uint32_t*)c.values, c.sorted_values,
                                              2 * (size_t)n_edges, 0, key_bits(n_vertices), s);
}

}  // namespace

namespace trgl {

hipError_t subdiv_topology_scratch_bytes(uint64_t n_edges, uint64_t n_vertices, size_t* bytes) {
    const Carve c = carve(nullptr, n_edges);
    size_t tmp = 0;
    if (n_edges) { const hipError_t e = sort_entries(nullptr, tmp, c, n_edges, n_vertices, nullptr); if (e != hipSuccess) return e; }
    *bytes = c.sort_off + align256(tmp) + 256;
    return hipSuccess;
}

hipError_t launch_subdiv_topology(hipStream_t s, const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t* edges,
                                  uint64_t n_edges, void* scratch, size_t scratch_bytes, uint32_t* indices_out, uint32_t* stencils_out) {
    const Carve c = carve(scratch, n_edges);
    if (scratch_bytes < c.sort_off) return hipErrorInvalidValue;
    uint32_t* odd = stencils_out;
    uint32_t* even = stencils_out + 4 * n_edges;
    uint32_t* ring = even + 4 * n_vertices;
    hipError_t e;
    if (n_edges) {
        hipLaunchKernelGGL(k_subdiv_odd, dim3(num_blocks(n_edges)), dim3(SUBDIV_BLOCK), 0, s, indices, n_faces, n_vertices, edges, (uint32_t)n_edges,
                           odd, c.keys, c.values);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t tmp = scratch_bytes - c.sort_off;
        if ((e = sort_entries((char*)scratch + c.sort_off, tmp, c, n_edges, n_vertices, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_subdiv_ring, dim3(num_blocks(2 * n_edges)), dim3(SUBDIV_BLOCK), 0, s, c.sorted_keys, c.sorted_values,
                           (uint32_t)(2 * n_edges), n_vertices, odd, ring);
    }
    hipLaunchKernelGGL(k_subdiv_even, dim3(num_blocks(n_vertices)), dim3(SUBDIV_BLOCK), 0, s, c.sorted_keys, c.sorted_values, (uint32_t)(2 * n_edges),
                       (uint32_t)n_vertices, odd, even);
    hipLaunchKernelGGL(k_subdiv_indices, dim3(num_blocks(n_faces)), dim3(SUBDIV_BLOCK), 0, s, indices, (uint32_t)n_faces, n_vertices, edges,
                       (uint32_t)n_edges, odd, indices_out);
    return hipGetLastError();
}

hipError_t launch_subdiv_topology_sort(hipStream_t s, uint64_t n_edges, uint64_t n_vertices, void* scratch, size_t scratch_bytes) {
    const Carve c = carve(scratch, n_edges);
    if (scratch_bytes < c.sort_off || !n_edges) return hipErrorInvalidValue;
    size_t tmp = scratch_bytes - c.sort_off;
    return sort_entries((char*)scratch + c.sort_off, tmp, c, n_edges, n_vertices, s);
}

hipError_t launch_subdiv_vertices(hipStream_t s, SubdivVertexArgs a) {
    const uint64_t total = (a.n_vertices + a.n_edges) * (uint64_t)a.stride, per_block = (uint64_t)SUBDIV_BLOCK * SUBDIV_ITEMS;
    a.step_q = (uint32_t)SUBDIV_BLOCK / a.stride; a.step_r = (uint32_t)SUBDIV_BLOCK % a.stride;
    hipLaunchKernelGGL(k_subdiv_vertices, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(SUBDIV_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace trgl
