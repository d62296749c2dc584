// kernels_edge.hip — the edge list of an indexed mesh and its classes per view (include/trgl.h: trgl_mesh_edges, trgl_edge_select and
// trgl_draw_outline), gfx950.  The arithmetic and the sort key are edge_core.h's.
//
// trgl_mesh_edges:
//   k_edge_keys     : one thread per half-edge h: its key (edge_key: lo above hi in 2 * bits bits, all ones for "no edge") and h itself.
//   the sort        : hipcub::DeviceRadixSort::SortPairs over those 2 * bits bits - least significant digit first, stable, so the
//                     half-edges of one edge stay in ascending h and the "no edge" keys end up behind every edge.
//   k_edge_count    : a block takes EDGE_BLOCK sorted entries, one per lane; an entry is a run head when its key is an edge's and differs
//                     from the key in front of it.  One ballot per wave; the block leaves its number of heads in blk[block].
//   the scan        : launch_block_count_scan (kernels_instance.hip), two levels; *total = the number of edges.
//   k_edge_write    : the blocks of k_edge_count make their ballots again; head i is edge e = chunk[block / INST_SCAN_CHUNK] + blk[block]
//                     + its rank in the block, and its lane writes {lo, hi, h / 3, the next entry's h / 3 when that has the same key}.
//                     Lane i >= *total also writes record i as "no edge": e <= i and e < *total, so the two never meet.
// trgl_edge_select:
//   k_edge_classify : one thread per record: both faces from their six vertices (edge_face), the code byte (edge_code); plain: the
//                     segment pair and the colour per record; compacted: the byte code & select to scratch and the block's count.
//   k_edge_scatter  : (compacted) the ranks again from the scratch bytes; selected record i goes to slot <= i, and lane i >= *total
//                     writes the tail.
// No atomic decides a position anywhere.  fp64 in edge_core.h's operation order, contraction off.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "launch.h"
#include "edge_core.h"

namespace {

using namespace trgl;

static_assert(EDGE_BLOCK == 256 && EDGE_BLOCK == INST_BLOCK, "four waves per block, and the scan of kernels_instance.hip over the block counts");

// The rank of this lane among the lanes of its block with `mine` set, and the block's count of them (every lane).  s_w: 4 words of LDS.
__device__ __forceinline__ uint32_t block_rank(bool mine, uint32_t* s_w, uint32_t* count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(mine);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_w[w];
    *count = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return rank;
}

// four words at a 4-byte aligned address; wide: the array is 16-byte aligned (the same for every lane)
__device__ __forceinline__ void store_words4(uint32_t* p, bool wide, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    if (wide) *reinterpret_cast<uint4*>(p) = make_uint4(x, y, z, w);
    else { p[0] = x; p[1] = y; p[2] = z; p[3] = w; }
}
__device__ __forceinline__ uint4 load_words4(const uint32_t* p, bool wide) {
    if (wide) return *reinterpret_cast<const uint4*>(p);
    return make_uint4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void store_words2(uint32_t* p, bool wide, uint32_t x, uint32_t y) {
    if (wide) *reinterpret_cast<uint2*>(p) = make_uint2(x, y);
    else { p[0] = x; p[1] = y; }
}
__host__ __device__ inline bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_keys(const uint32_t* __restrict__ indices, uint32_t nh, uint64_t n_vertices, int bits,
                                                          unsigned long long* __restrict__ keys, uint32_t* __restrict__ numbers) {
    const uint32_t h = blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (h >= nh) return;
    const uint32_t f = h / 3, k = h - 3 * f;
    const uint32_t a = indices[h], b = indices[3 * f + (k == 2 ? 0 : k + 1)];
    keys[h] = edge_key(a, b, n_vertices, bits);
    numbers[h] = h;
}

// this lane's sorted entry is the first of an edge's run
__device__ __forceinline__ bool run_head(const unsigned long long* __restrict__ keys, uint32_t i, uint32_t nh, unsigned long long none,
                                         unsigned long long* key) {
    if (i >= nh) { *key = none; return false; }
    const unsigned long long k = keys[i];
    *key = k;
    return k != none && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_count(const unsigned long long* __restrict__ keys, uint32_t nh, unsigned long long none,
                                                           uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    unsigned long long key;
    const bool head = run_head(keys, blockIdx.x * EDGE_BLOCK + threadIdx.x, nh, none, &key);
    uint32_t count;
    (void)block_rank(head, s_w, &count);
    if (threadIdx.x == 0) blk[blockIdx.x] = count;
}

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_write(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ numbers,
                                                           uint32_t nh, unsigned long long none, int bits, const uint32_t* __restrict__ blk,
                                                           const uint32_t* __restrict__ chunk, const unsigned long long* __restrict__ total,
                                                           uint32_t* __restrict__ edges_out, bool wide) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * EDGE_BLOCK + threadIdx.x;
    unsigned long long key;
    const bool head = run_head(keys, i, nh, none, &key);
    uint32_t count;
    const uint32_t rank = block_rank(head, s_w, &count);
    if (i >= nh) return;
    if (head) {
        const uint32_t e = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x] + rank;
        const uint32_t f1 = (i + 1 < nh && keys[i + 1] == key) ? numbers[i + 1] / 3 : EDGE_NONE;
        store_words4(edges_out + 4 * (size_t)e, wide, edge_key_lo(key, bits), edge_key_hi(key, bits), numbers[i] / 3, f1);
    }
    if ((unsigned long long)i >= *total) store_words4(edges_out + 4 * (size_t)i, wide, EDGE_NONE, EDGE_NONE, EDGE_NONE, EDGE_NONE);
}

// The face `f` of the mesh (f < n_faces): false when one of its indices names no vertex
__device__ __forceinline__ bool load_face(const EdgeSelectArgs& a, uint32_t f, EdgeFace* out) {
    const uint32_t i0 = a.indices[3 * (size_t)f], i1 = a.indices[3 * (size_t)f + 1], i2 = a.indices[3 * (size_t)f + 2];
    if (i0 >= a.n_vertices || i1 >= a.n_vertices || i2 >= a.n_vertices) return false;
    const double* r0 = a.vertices + (size_t)i0 * (size_t)a.stride;
    const double* r1 = a.vertices + (size_t)i1 * (size_t)a.stride;
    const double* r2 = a.vertices + (size_t)i2 * (size_t)a.stride;
    const double p0[3] = { r0[0], r0[1], r0[2] }, p1[3] = { r1[0], r1[1], r1[2] }, p2[3] = { r2[0], r2[1], r2[2] };
    *out = edge_face(p0, p1, p2, a.P.eye);
    return true;
}

template <bool COMPACT>
__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_classify(EdgeSelectArgs a, uint8_t* __restrict__ tmp_sel, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * EDGE_BLOCK + threadIdx.x;
    uint32_t sel = 0;
    if (i < a.n_edges) {
        const uint4 rec = load_words4(a.edges + 4 * (size_t)i, aligned_to(a.edges, 16));
        const uint32_t f0 = rec.z, f1 = rec.w;
        uint32_t code = 0;
        if (f0 < a.n_faces && (f1 == EDGE_NONE || f1 < a.n_faces)) {       // (EDGE_NONE is no face: 3 * n_faces < 2^31)
            EdgeFace A, B;
            B.front = false; B.u[0] = B.u[1] = B.u[2] = 0.0;
            const bool has1 = f1 != EDGE_NONE;
            if (load_face(a, f0, &A) && (!has1 || load_face(a, f1, &B))) code = edge_code(A, has1, B, a.P.crease_cos);
        }
        sel = code & a.P.select;
        if (a.codes) a.codes[i] = (uint8_t)code;
        if (COMPACT) tmp_sel[i] = (uint8_t)sel;
        else {
            if (a.segments) store_words2(a.segments + 2 * (size_t)i, aligned_to(a.segments, 8), sel ? rec.x : EDGE_NONE, sel ? rec.y : EDGE_NONE);
            if (a.colors) a.colors[i] = sel ? edge_color(a.P.class_color, sel) : 0u;
        }
    }
    if (COMPACT) {
        uint32_t count;
        (void)block_rank(sel != 0, s_w, &count);
        if (threadIdx.x == 0) blk[blockIdx.x] = count;
    }
}

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_scatter(EdgeSelectArgs a, const uint8_t* __restrict__ tmp_sel, const uint32_t* __restrict__ blk,
                                                             const uint32_t* __restrict__ chunk, const unsigned long long* __restrict__ total) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * EDGE_BLOCK + threadIdx.x;
    const uint32_t sel = i < a.n_edges ? tmp_sel[i] : 0u;
    uint32_t count;
    const uint32_t rank = block_rank(sel != 0, s_w, &count);
    if (i >= a.n_edges) return;
    const bool wide = aligned_to(a.segments, 8);
    if (sel) {
        const uint32_t slot = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x] + rank;
        if (a.segments) store_words2(a.segments + 2 * (size_t)slot, wide, a.edges[4 * (size_t)i], a.edges[4 * (size_t)i + 1]);
        if (a.colors) a.colors[slot] = edge_color(a.P.class_color, sel);
    }
    if ((unsigned long long)i >= *total) {
        if (a.segments) store_words2(a.segments + 2 * (size_t)i, wide, EDGE_NONE, EDGE_NONE);
        if (a.colors) a.colors[i] = 0u;
    }
}

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
uint32_t num_blocks(uint32_t n) { return (n + EDGE_BLOCK - 1) / EDGE_BLOCK; }
uint32_t num_chunks(uint32_t nblk) { return (nblk + INST_SCAN_CHUNK - 1) / INST_SCAN_CHUNK; }

struct Carve { unsigned long long* total; unsigned long long* keys; unsigned long long* sorted_keys; uint32_t* numbers; uint32_t* sorted_numbers;
               uint32_t* blk; uint32_t* chunk; size_t sort_off; };
Carve carve(void* scratch, uint32_t nh) {
    char* p = (char*)scratch;
    const uint32_t nblk = num_blocks(nh);
    Carve c;
    size_t off = 0;
    c.total = (unsigned long long*)(p + off); off += 256;
    c.keys = (unsigned long long*)(p + off); off += align256((size_t)nh * sizeof(unsigned long long));
    c.sorted_keys = (unsigned long long*)(p + off); off += align256((size_t)nh * sizeof(unsigned long long));
    c.numbers = (uint32_t*)(p + off); off += align256((size_t)nh * sizeof(uint32_t));
    c.sorted_numbers = (uint32_t*)(p + off); off += align256((size_t)nh * sizeof(uint32_t));
    c.blk = (uint32_t*)(p + off); off += align256((size_t)nblk * sizeof(uint32_t));
    c.chunk = (uint32_t*)(p + off); off += align256((size_t)num_chunks(nblk) * sizeof(uint32_t));
    c.sort_off = off;
    return c;
}

hipError_t sort_half_edges(void* tmp, size_t& tmp_bytes, const Carve& c, uint32_t nh, int bits, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const unsigned long long*)c.keys, c.sorted_keys, (const uint32_t*)c.numbers,
                                              c.sorted_numbers, (size_t)nh, 0, 2 * bits, s);
}

struct SelectCarve { unsigned long long* total; uint8_t* sel; uint32_t* blk; uint32_t* chunk; size_t bytes; };
SelectCarve select_carve(void* scratch, uint32_t n) {
    char* p = (char*)scratch;
    const uint32_t nblk = num_blocks(n);
    SelectCarve c;
    size_t off = 0;
    c.total = (unsigned long long*)(p + off); off += 256;
    c.sel = (uint8_t*)(p + off); off += align256(n);
    c.blk = (uint32_t*)(p + off); off += align256((size_t)nblk * sizeof(uint32_t));
    c.chunk = (uint32_t*)(p + off); off += align256((size_t)num_chunks(nblk) * sizeof(uint32_t));
    c.bytes = off;
    return c;
}

}  // namespace

namespace trgl {

hipError_t mesh_edges_scratch_bytes(uint32_t nh, uint64_t n_vertices, size_t* bytes) {
    const Carve c = carve(nullptr, nh);
    size_t tmp = 0;
    const hipError_t e = sort_half_edges(nullptr, tmp, c, nh, edge_index_bits(n_vertices), nullptr);
    if (e != hipSuccess) return e;
    *bytes = c.sort_off + align256(tmp);
    return hipSuccess;
}

hipError_t launch_mesh_edges(hipStream_t s, const uint32_t* indices, uint32_t nh, uint64_t n_vertices, void* scratch, size_t scratch_bytes,
                             uint32_t* edges_out, const unsigned long long** total) {
    const Carve c = carve(scratch, nh);
    if (scratch_bytes < c.sort_off) return hipErrorInvalidValue;
    *total = c.total;
    const int bits = edge_index_bits(n_vertices);
    const unsigned long long none = edge_key_none(bits);
    const uint32_t nblk = num_blocks(nh);
    hipLaunchKernelGGL(k_edge_keys, dim3(nblk), dim3(EDGE_BLOCK), 0, s, indices, nh, n_vertices, bits, c.keys, c.numbers);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tmp = scratch_bytes - c.sort_off;
    if ((e = sort_half_edges((char*)scratch + c.sort_off, tmp, c, nh, bits, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_edge_count, dim3(nblk), dim3(EDGE_BLOCK), 0, s, c.sorted_keys, nh, none, c.blk);
    launch_block_count_scan(s, c.blk, nblk, c.chunk, c.total);
    hipLaunchKernelGGL(k_edge_write, dim3(nblk), dim3(EDGE_BLOCK), 0, s, c.sorted_keys, c.sorted_numbers, nh, none, bits, c.blk, c.chunk, c.total,
                       edges_out, aligned_to(edges_out, 16));
    return hipGetLastError();
}

hipError_t launch_mesh_edges_sort(hipStream_t s, uint32_t nh, uint64_t n_vertices, void* scratch, size_t scratch_bytes) {
    const Carve c = carve(scratch, nh);
    if (scratch_bytes < c.sort_off) return hipErrorInvalidValue;
    size_t tmp = scratch_bytes - c.sort_off;
    return sort_half_edges((char*)scratch + c.sort_off, tmp, c, nh, edge_index_bits(n_vertices), s);
}

size_t edge_select_scratch_bytes(uint32_t n) { return select_carve(nullptr, n).bytes; }

hipError_t launch_edge_select(hipStream_t s, const EdgeSelectArgs& a, void* scratch, const unsigned long long** total) {
    const uint32_t nblk = num_blocks(a.n_edges);
    if (!a.P.compact) {
        *total = nullptr;
        hipLaunchKernelGGL(k_edge_classify<false>, dim3(nblk), dim3(EDGE_BLOCK), 0, s, a, nullptr, nullptr);
        return hipGetLastError();
    }
    const SelectCarve c = select_carve(scratch, a.n_edges);
    *total = c.total;
    hipLaunchKernelGGL(k_edge_classify<true>, dim3(nblk), dim3(EDGE_BLOCK), 0, s, a, c.sel, c.blk);
    launch_block_count_scan(s, c.blk, nblk, c.chunk, c.total);
    hipLaunchKernelGGL(k_edge_scatter, dim3(nblk), dim3(EDGE_BLOCK), 0, s, a, c.sel, c.blk, c.chunk, c.total);
    return hipGetLastError();
}

}  // namespace trgl
