// kernels_weld.hip — identical vertices joined (include/trgl.h: trgl_mesh_weld), gfx950.  The compared value, the comparison and the
// hash are weld_core.h's.
//
//   k_weld_keys    : one thread per vertex v: the low hash_bits bits of the hash of its key, and v itself.
//   the sort       : hipcub::DeviceRadixSort::SortPairs over those bits - stable, so a run of equal hashes is in ascending v.  With
//                    hash_bits == 0 there is nothing to sort: the pairs as written are one run in ascending v.
//   k_weld_resolve : one thread per sorted entry i.  The first entry of its run: itself when the hash in front differs, else a
//                    lower_bound over the sorted hashes.  Its key equals the run head's - every duplicate of a mesh, unless two keys
//                    collide: rep = the head's vertex.  It does not: the run is walked from its head to the first entry in front of i
//                    whose key is identical - the lowest-numbered one, the run ascends in v -; none (a NaN finds none): rep = v.
//   k_weld_count   : a block takes WELD_BLOCK vertices in old order; the flag is rep[v] == v; one ballot per wave, the block's count.
//   the scan       : launch_block_count_scan (kernels_instance.hip), two levels; *total = the number of distinct vertices.
//   k_weld_write   : the ballots again.  Representative v gets newnum[v] = chunk[..] + blk[block] + its rank and writes firsts_out
//                    there.  The block's representatives have consecutive new numbers, so their records are one contiguous piece of
//                    vertices_out: the lanes store it 16 bytes each (8 at a head or tail that is only 8-byte aligned), each 8 bytes
//                    loaded from the record they come from - duplicates' records are never read.  Lane i >= *total writes the
//                    firsts_out fill, and the block the zero records of its vertices >= *total, contiguous again.  A slot below *total
//                    is written by its representative alone and a slot at or above it by its own number's block alone.
//   k_weld_remap   : remap[v] = newnum[rep[v]] (into scratch when remap_out is null and indices_out is not).
//   k_weld_indices : indices_out[i] = remap[indices[i]], NONE for an index >= n - compared before it becomes an address.
// No atomic decides a number or a position.  Records move as 64-bit words: every bit is kept.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "compact_device.h"
#include "launch.h"
#include "weld_core.h"

namespace {

using namespace trgl;
using namespace trgl_dev;            // block_rank, store_run, move_kept_records (compact_device.h)

static_assert(WELD_BLOCK == 256 && WELD_BLOCK == INST_BLOCK && WELD_BLOCK == COMPACT_BLOCK, "four waves per block, and the scan of kernels_instance.hip over the block counts");

typedef unsigned long long u64;

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_keys(WeldArgs a, u64* __restrict__ hashes, uint32_t* __restrict__ numbers) {
    const uint32_t v = blockIdx.x * WELD_BLOCK + threadIdx.x;
    if (v >= a.n) return;
    const double* r = a.vertices + (size_t)v * (size_t)a.P.vertex_stride;
    hashes[v] = weld_hash_low(weld_hash(r, a.P.key_offset, a.P.key_count, a.P.cell), a.hash_bits);
    numbers[v] = v;
}

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_resolve(WeldArgs a, const u64* __restrict__ sh, const uint32_t* __restrict__ sn,
                                                             uint32_t* __restrict__ rep) {
    const uint32_t i = blockIdx.x * WELD_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const u64 h = sh[i];
    const uint32_t v = sn[i];                                             // (a permutation of 0 .. n-1: the sort's values)
    uint32_t first = i;
    if (i > 0 && sh[i - 1] == h) {                                        // lower_bound of h in sh[0 .. i)
        uint32_t lo = 0, hi = i;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (sh[mid] < h) lo = mid + 1; else hi = mid; }
        first = lo;
    }
    const size_t S = (size_t)a.P.vertex_stride;
    const double* rv = a.vertices + (size_t)v * S;
    uint32_t r = v;
    for (uint32_t j = first; j < i; ++j) {                                // (the head first: one step for every duplicate without a collision)
        const uint32_t u = sn[j];
        if (weld_identical(a.vertices + (size_t)u * S, rv, a.P.key_offset, a.P.key_count, a.P.cell)) { r = u; break; }
    }
    rep[v] = r;
}

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_count(const uint32_t* __restrict__ rep, uint32_t n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    const uint32_t v = blockIdx.x * WELD_BLOCK + threadIdx.x;
    uint32_t count;
    (void)block_rank(v < n && rep[v] == v, s_w, &count);
    if (threadIdx.x == 0) blk[blockIdx.x] = count;
}

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_write(WeldArgs a, const uint32_t* __restrict__ rep, const uint32_t* __restrict__ blk,
                                                           const uint32_t* __restrict__ chunk, const u64* __restrict__ total,
                                                           uint32_t* __restrict__ newnum) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_src[WELD_BLOCK];                                // the block's representatives by rank, as lane numbers
    const uint32_t v0 = blockIdx.x * WELD_BLOCK, v = v0 + threadIdx.x;
    const bool is_rep = v < a.n && rep[v] == v;
    uint32_t count;
    const uint32_t rank = block_rank(is_rep, s_w, &count);
    const uint32_t base = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x];      // base + count <= *total <= n
    const u64 U = *total;
    if (is_rep) {
        newnum[v] = base + rank;
        s_src[rank] = threadIdx.x;
        if (a.firsts_out) a.firsts_out[base + rank] = v;
    }
    if (v < a.n && (u64)v >= U && a.firsts_out) a.firsts_out[v] = WELD_NONE;
    if (!a.vertices_out) return;
    __syncthreads();
    move_kept_records(reinterpret_cast<const u64*>(a.vertices), reinterpret_cast<u64*>(a.vertices_out), (u64)a.P.vertex_stride, s_src, count, base,
                      v0, a.n, U);
}

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_remap(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ newnum, uint32_t n,
                                                           uint32_t* __restrict__ remap) {
    const uint32_t v = blockIdx.x * WELD_BLOCK + threadIdx.x;
    if (v < n) remap[v] = newnum[rep[v]];                                 // (rep[v] < n: a vertex number of the sort's values)
}

__global__ __launch_bounds__(WELD_BLOCK) void k_weld_indices(const uint32_t* __restrict__ indices, uint32_t n_idx, const uint32_t* __restrict__ remap,
                                                             uint32_t n, uint32_t* __restrict__ indices_out) {
    const uint32_t i = blockIdx.x * WELD_BLOCK + threadIdx.x;
    if (i >= n_idx) return;
    const uint32_t idx = indices[i];
    indices_out[i] = idx < n ? remap[idx] : WELD_NONE;
}

uint32_t num_blocks(uint32_t n) { return (n + WELD_BLOCK - 1) / WELD_BLOCK; }
uint32_t num_chunks(uint32_t nblk) { return (nblk + INST_SCAN_CHUNK - 1) / INST_SCAN_CHUNK; }

struct Carve { u64* total; u64* hashes; u64* sorted_hashes; uint32_t* numbers; uint32_t* sorted_numbers; uint32_t* rep; uint32_t* newnum;
               uint32_t* remap; uint32_t* blk; uint32_t* chunk; size_t sort_off; };
Carve carve(void* scratch, uint32_t n) {
    char* p = (char*)scratch;
    const uint32_t nblk = num_blocks(n);
    Carve c;
    size_t off = 0;
    c.total = (u64*)(p + off); off += 256;
    c.hashes = (u64*)(p + off); off += scratch_align256((size_t)n * sizeof(u64));
    c.sorted_hashes = (u64*)(p + off); off += scratch_align256((size_t)n * sizeof(u64));
    c.numbers = (uint32_t*)(p + off); off += scratch_align256((size_t)n * sizeof(uint32_t));
    c.sorted_numbers = (uint32_t*)(p + off); off += scratch_align256((size_t)n * sizeof(uint32_t));
    c.rep = (uint32_t*)(p + off); off += scratch_align256((size_t)n * sizeof(uint32_t));
    c.newnum = (uint32_t*)(p + off); off += scratch_align256((size_t)n * sizeof(uint32_t));
    c.remap = (uint32_t*)(p + off); off += scratch_align256((size_t)n * sizeof(uint32_t));
    c.blk = (uint32_t*)(p + off); off += scratch_align256((size_t)nblk * sizeof(uint32_t));
    c.chunk = (uint32_t*)(p + off); off += scratch_align256((size_t)num_chunks(nblk) * sizeof(uint32_t));
    c.sort_off = off;
    return c;
}

// hash_bits > 0
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const Carve& c, uint32_t n, int hash_bits, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const u64*)c.hashes, c.sorted_hashes, (const uint32_t*)c.numbers, c.sorted_numbers,
                                              (size_t)n, 0, hash_bits, s);
}

}  // namespace

namespace trgl {

hipError_t mesh_weld_scratch_bytes(uint32_t n, int hash_bits, size_t* bytes) {
    const Carve c = carve(nullptr, n);
    size_t tmp = 0;
    if (hash_bits > 0) {
        const hipError_t e = sort_pairs(nullptr, tmp, c, n, hash_bits, nullptr);
        if (e != hipSuccess) return e;
    }
    *bytes = c.sort_off + scratch_align256(tmp);
    return hipSuccess;
}

hipError_t launch_mesh_weld(hipStream_t s, const WeldArgs& a, void* scratch, size_t scratch_bytes, const unsigned long long** total) {
    const Carve c = carve(scratch, a.n);
    if (scratch_bytes < c.sort_off || a.hash_bits < 0 || a.hash_bits > 64) return hipErrorInvalidValue;
    *total = c.total;
    const uint32_t nblk = num_blocks(a.n);
    hipLaunchKernelGGL(k_weld_keys, dim3(nblk), dim3(WELD_BLOCK), 0, s, a, c.hashes, c.numbers);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const u64* sh = c.hashes; const uint32_t* sn = c.numbers;
    if (a.hash_bits > 0) {
        size_t tmp = scratch_bytes - c.sort_off;
        if ((e = sort_pairs((char*)scratch + c.sort_off, tmp, c, a.n, a.hash_bits, s)) != hipSuccess) return e;
        sh = c.sorted_hashes; sn = c.sorted_numbers;
    }
    hipLaunchKernelGGL(k_weld_resolve, dim3(nblk), dim3(WELD_BLOCK), 0, s, a, sh, sn, c.rep);
    hipLaunchKernelGGL(k_weld_count, dim3(nblk), dim3(WELD_BLOCK), 0, s, c.rep, a.n, c.blk);
    launch_block_count_scan(s, c.blk, nblk, c.chunk, c.total);
    hipLaunchKernelGGL(k_weld_write, dim3(nblk), dim3(WELD_BLOCK), 0, s, a, c.rep, c.blk, c.chunk, c.total, c.newnum);
    if (a.remap_out || a.indices_out) {
        uint32_t* remap = a.remap_out ? a.remap_out : c.remap;
        hipLaunchKernelGGL(k_weld_remap, dim3(nblk), dim3(WELD_BLOCK), 0, s, c.rep, c.newnum, a.n, remap);
        if (a.indices_out && a.n_idx)
            hipLaunchKernelGGL(k_weld_indices, dim3(num_blocks(a.n_idx)), dim3(WELD_BLOCK), 0, s, a.indices, a.n_idx, remap, a.n, a.indices_out);
    }
    return hipGetLastError();
}

WeldPairs mesh_weld_pairs(const void* scratch, uint32_t n, int hash_bits) {
    const Carve c = carve(const_cast<void*>(scratch), n);
    return hash_bits > 0 ? WeldPairs{ c.sorted_hashes, c.sorted_numbers, c.rep, c.newnum } : WeldPairs{ c.hashes, c.numbers, c.rep, c.newnum };
}

hipError_t launch_mesh_weld_sort(hipStream_t s, uint32_t n, int hash_bits, void* scratch, size_t scratch_bytes) {
    const Carve c = carve(scratch, n);
    if (scratch_bytes < c.sort_off || hash_bits < 1 || hash_bits > 64) return hipErrorInvalidValue;
    size_t tmp = scratch_bytes - c.sort_off;
    return sort_pairs((char*)scratch + c.sort_off, tmp, c, n, hash_bits, s);
}

}  // namespace trgl
