// kernels_lod.hip — faces that draw nothing removed and the cells of a vertex clustering averaged (include/trgl.h: trgl_mesh_clean,
// trgl_mesh_simplify), gfx950.  The class of a face, the canonical triple, its hash and the mean's arithmetic are lod_core.h's.
//
//   k_clean_keys    : one thread per face f: the low hash_bits bits of the hash of its canonical triple - of its own number when it is
//                     invalid or degenerate: such a face is identical to nothing -, and f itself.
//   the sort        : hipcub::DeviceRadixSort::SortPairs over those bits - stable, so a run of equal hashes is in ascending f.  With
//                     hash_bits == 0 there is nothing to sort: the pairs as written are one run in ascending f.
//   k_clean_resolve : one thread per sorted entry i, a candidate face f.  The first entry of its run: itself when the hash in front
//                     differs, else a lower_bound over the sorted hashes.  The run is walked from its head to i: the first candidate with
//                     f's triple makes f a duplicate (the head, unless two triples collide); none: f is kept.  keep[f], one byte.
//   k_clean_classify: without TRGL_CLEAN_DUPLICATES, instead of the three above: keep[f] = f is a candidate.
//   k_clean_fcount  : a block takes LOD_BLOCK faces in old order; one ballot per wave over keep[], the block's count.
//   the scan        : launch_block_count_scan (kernels_instance.hip), two levels; totals[0] = the number of kept faces.
//   k_clean_mark    : with TRGL_CLEAN_VERTICES, every kept face stores 1 to the words of its three vertices (zeroed before): plain stores of
//                     the same word by every face that names the vertex.
//   k_clean_vcount, the scan again: totals[1] = the number of referenced vertices.
//   k_clean_vwrite  : the ballots again.  vremap[v] = chunk[..] + blk[block] + rank, or NONE; vfirsts_out; the block's referenced records
//                     are one contiguous piece of vertices_out (move_kept_records, compact_device.h), the zero records behind the count.
//   k_clean_fwrite  : the ballots over keep[] again.  A kept face puts its three indices - through vremap with TRGL_CLEAN_VERTICES - and
//                     its number into LDS at its rank; the block's kept faces have consecutive new numbers, so their 12-byte triples are one
//                     contiguous piece of indices_out: the lanes store it 16 bytes each from LDS (4 per word in front of the first and
//                     behind the last 16-byte boundary), not as three strided 4-byte stores per face.  The fill words of the block's own
//                     faces at or above totals[0] leave the same way.  A slot below the count is written by its keeper's block alone and
//                     one at or above it by its own number's block alone.
//   k_lod_mark_words: (simplify) every word of `indices` below n stores 1 to its vertex's word.
//   k_lod_mean      : (simplify) one thread per sorted entry of the weld's pairs; the head of a cluster (rep[v] == v) walks its run of equal
//                     hashes from its own place on - the run ascends in vertex number - and sums the referenced members of its cluster
//                     in that order, four doubles of the record per walk.  Long and serial when a mesh collapses into a few cells.
//   k_lod_compose   : (simplify) remap_out and firsts_out through the weld's map and the clean's.
// No atomic decides a number or a position.  Records move as 64-bit words: every bit is kept.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "compact_device.h"
#include "launch.h"
#include "lod_core.h"

namespace {

using namespace trgl;
using namespace trgl_dev;            // block_rank, store_run32, move_kept_records (compact_device.h)

static_assert(LOD_BLOCK == 256 && LOD_BLOCK == INST_BLOCK && LOD_BLOCK == COMPACT_BLOCK, "four waves per block, and the scan of kernels_instance.hip over the block counts");

typedef unsigned long long u64;

struct Face { uint32_t a, b, c; };
__device__ __forceinline__ Face load_face(const uint32_t* __restrict__ indices, uint32_t f) {
    const uint32_t* p = indices + (size_t)f * 3;
    return Face{ p[0], p[1], p[2] };
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_keys(CleanArgs a, u64* __restrict__ hashes, uint32_t* __restrict__ numbers) {
    const uint32_t f = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (f >= a.n_faces) return;
    const Face t = load_face(a.indices, f);
    const u64 h = lod_face_class(t.a, t.b, t.c, a.n_vertices) == LOD_FACE_CANDIDATE ? lod_face_hash(lod_canonical(t.a, t.b, t.c)) : lod_dropped_hash(f);
    hashes[f] = weld_hash_low(h, a.hash_bits);
    numbers[f] = f;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_resolve(CleanArgs a, const u64* __restrict__ sh, const uint32_t* __restrict__ sn,
                                                             uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (i >= a.n_faces) return;
    const uint32_t f = sn[i];                                             // (a permutation of 0 .. n_faces-1: the sort's values)
    const Face t = load_face(a.indices, f);
    if (lod_face_class(t.a, t.b, t.c, a.n_vertices) != LOD_FACE_CANDIDATE) { keep[f] = 0; return; }
    const u64 h = sh[i];
    uint32_t first = i;
    if (i > 0 && sh[i - 1] == h) {                                        // lower_bound of h in sh[0 .. i)
        uint32_t lo = 0, hi = i;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (sh[mid] < h) lo = mid + 1; else hi = mid; }
        first = lo;
    }
    const LodTriple mine = lod_canonical(t.a, t.b, t.c);
    uint8_t kept = 1;
    for (uint32_t j = first; j < i; ++j) {                                // (the head first: one step for every duplicate without a collision)
        const Face g = load_face(a.indices, sn[j]);
        if (lod_face_class(g.a, g.b, g.c, a.n_vertices) == LOD_FACE_CANDIDATE && lod_same_triple(lod_canonical(g.a, g.b, g.c), mine)) { kept = 0; break; }
    }
    keep[f] = kept;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_classify(CleanArgs a, uint8_t* __restrict__ keep) {
    const uint32_t f = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (f >= a.n_faces) return;
    const Face t = load_face(a.indices, f);
    keep[f] = lod_face_class(t.a, t.b, t.c, a.n_vertices) == LOD_FACE_CANDIDATE ? 1 : 0;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_fcount(const uint8_t* __restrict__ keep, uint32_t n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    const uint32_t f = blockIdx.x * LOD_BLOCK + threadIdx.x;
    uint32_t count;
    (void)block_rank(f < n && keep[f] != 0, s_w, &count);
    if (threadIdx.x == 0) blk[blockIdx.x] = count;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_mark(CleanArgs a, const uint8_t* __restrict__ keep, uint32_t* __restrict__ referenced) {
    const uint32_t f = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (f >= a.n_faces || !keep[f]) return;
    const Face t = load_face(a.indices, f);                               // (a kept face: its three indices are below n_vertices)
    referenced[t.a] = 1u; referenced[t.b] = 1u; referenced[t.c] = 1u;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_vcount(const uint32_t* __restrict__ referenced, uint32_t n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    const uint32_t v = blockIdx.x * LOD_BLOCK + threadIdx.x;
    uint32_t count;
    (void)block_rank(v < n && referenced[v] != 0u, s_w, &count);
    if (threadIdx.x == 0) blk[blockIdx.x] = count;
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_vwrite(CleanArgs a, const uint32_t* __restrict__ referenced, const uint32_t* __restrict__ blk,
                                                            const uint32_t* __restrict__ chunk, const u64* __restrict__ total,
                                                            uint32_t* __restrict__ vremap) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_src[LOD_BLOCK];                                 // the block's referenced vertices by rank, as lane numbers
    const uint32_t v0 = blockIdx.x * LOD_BLOCK, v = v0 + threadIdx.x;
    const bool kept = v < a.n_vertices && referenced[v] != 0u;
    uint32_t count;
    const uint32_t rank = block_rank(kept, s_w, &count);
    const uint32_t base = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x];      // base + count <= *total <= n_vertices
    const u64 U = *total;
    if (kept) {
        s_src[rank] = threadIdx.x;
        if (a.vfirsts_out) a.vfirsts_out[base + rank] = v;
    }
    if (v < a.n_vertices) {
        vremap[v] = kept ? base + rank : LOD_NONE;
        if ((u64)v >= U && a.vfirsts_out) a.vfirsts_out[v] = LOD_NONE;
    }
    if (!a.vertices_out) return;
    __syncthreads();
    move_kept_records(reinterpret_cast<const u64*>(a.vertices), reinterpret_cast<u64*>(a.vertices_out), (u64)a.P.vertex_stride, s_src, count, base,
                      v0, a.n_vertices, U);
}

__global__ __launch_bounds__(LOD_BLOCK) void k_clean_fwrite(CleanArgs a, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ blk,
                                                            const uint32_t* __restrict__ chunk, const u64* __restrict__ total,
                                                            const uint32_t* __restrict__ vremap) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_words[3 * LOD_BLOCK];                           // the block's kept triples by rank
    __shared__ uint32_t s_first[LOD_BLOCK];                               // ... and their old numbers
    const uint32_t f0 = blockIdx.x * LOD_BLOCK, f = f0 + threadIdx.x;
    const bool kept = f < a.n_faces && keep[f] != 0;
    uint32_t count;
    const uint32_t rank = block_rank(kept, s_w, &count);
    const uint32_t base = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x];      // base + count <= *total <= n_faces
    const u64 K = *total;
    if (kept) {
        Face t = load_face(a.indices, f);
        if (vremap) { t.a = vremap[t.a]; t.b = vremap[t.b]; t.c = vremap[t.c]; }       // (a kept face: its indices are below n_vertices, and referenced)
        s_words[3 * rank] = t.a; s_words[3 * rank + 1] = t.b; s_words[3 * rank + 2] = t.c;
        s_first[rank] = f;
    }
    __syncthreads();
    const uint32_t end = f0 + LOD_BLOCK < a.n_faces ? f0 + LOD_BLOCK : a.n_faces;     // (f0 < n_faces < 2^31 / 3)
    const uint32_t z0 = K > (u64)f0 ? (uint32_t)K : f0;                               // (K <= n_faces)
    if (a.indices_out) {
        if (count) store_run32(a.indices_out + (size_t)base * 3, 3 * count, [&](uint32_t d) { return s_words[d]; });
        const uint32_t fill = a.P.fill == TRGL_CLEAN_FILL_ZERO ? 0u : LOD_NONE;
        if (z0 < end) store_run32(a.indices_out + (size_t)z0 * 3, 3 * (end - z0), [fill](uint32_t) { return fill; });
    }
    if (a.face_firsts_out) {
        if (threadIdx.x < count) a.face_firsts_out[base + threadIdx.x] = s_first[threadIdx.x];
        if (f < a.n_faces && (u64)f >= K) a.face_firsts_out[f] = LOD_NONE;
    }
}

__global__ __launch_bounds__(LOD_BLOCK) void k_lod_mark_words(const uint32_t* __restrict__ indices, uint32_t n_idx, uint32_t n, uint32_t* __restrict__ referenced) {
    const uint32_t i = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (i >= n_idx) return;
    const uint32_t idx = indices[i];
    if (idx < n) referenced[idx] = 1u;                                    // compared before it becomes an address
}

__global__ __launch_bounds__(LOD_BLOCK) void k_lod_mean(WeldPairs w, const double* __restrict__ vertices, uint32_t S, uint32_t mean_count, uint32_t n,
                                                        const uint32_t* __restrict__ referenced, double* __restrict__ records) {
    const uint32_t i = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = w.numbers[i];
    if (w.rep[v] != v) return;                                            // the lowest number of its cluster: the first of it in the run
    const u64 h = w.hashes[i];
    double* out = records + (size_t)w.newnum[v] * S;
    for (uint32_t a0 = 0; a0 < mean_count; a0 += 4) {
        const uint32_t na = mean_count - a0 < 4 ? mean_count - a0 : 4;
        double s[4] = { 0.0, 0.0, 0.0, 0.0 };
        uint32_t count = 0, first = 0;
        for (uint32_t k = i; k < n && w.hashes[k] == h; ++k) {
            const uint32_t u = w.numbers[k];
            if (w.rep[u] != v || !referenced[u]) continue;
            const double* r = vertices + (size_t)u * S + a0;
            if (count == 0) { first = u; for (uint32_t a = 0; a < na; ++a) s[a] = r[a]; }
            else for (uint32_t a = 0; a < na; ++a) s[a] = lod_mean_add(s[a], r[a]);
            ++count;
        }
        if (count == 0) return;                                           // the representative's record stays
        if (count == 1) {                                                 // that member's bits
            const u64* r = reinterpret_cast<const u64*>(vertices) + (size_t)first * S + a0;
            for (uint32_t a = 0; a < na; ++a) reinterpret_cast<u64*>(out)[a0 + a] = r[a];
        } else {
            for (uint32_t a = 0; a < na; ++a) out[a0 + a] = lod_mean_div(s[a], count);
        }
    }
}

__global__ __launch_bounds__(LOD_BLOCK) void k_lod_compose(uint32_t n, const uint32_t* __restrict__ weld_remap, const uint32_t* __restrict__ vremap,
                                                           uint32_t* __restrict__ remap_out, const uint32_t* __restrict__ weld_firsts,
                                                           const uint32_t* __restrict__ vfirsts, uint32_t* __restrict__ firsts_out) {
    const uint32_t v = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (v >= n) return;
    if (remap_out) remap_out[v] = vremap[weld_remap[v]];                  // (weld_remap[v] < n: a new number of the weld)
    if (firsts_out) { const uint32_t j = vfirsts[v]; firsts_out[v] = j < n ? weld_firsts[j] : LOD_NONE; }
}

uint32_t num_blocks(uint32_t n) { return (n + LOD_BLOCK - 1) / LOD_BLOCK; }
uint32_t num_chunks(uint32_t nblk) { return (nblk + INST_SCAN_CHUNK - 1) / INST_SCAN_CHUNK; }

struct Carve { u64* totals; u64* hashes; u64* sorted_hashes; uint32_t* numbers; uint32_t* sorted_numbers; uint8_t* keep; uint32_t* fblk; uint32_t* fchunk;
               uint32_t* referenced; uint32_t* vremap; uint32_t* vblk; uint32_t* vchunk; size_t sort_off; };
Carve carve(void* scratch, uint32_t F, uint32_t V) {
    char* p = (char*)scratch;
    const uint32_t fb = num_blocks(F), vb = num_blocks(V);
    Carve c;
    size_t off = 0;
    c.totals = (u64*)(p + off); off += 256;
    c.hashes = (u64*)(p + off); off += scratch_align256((size_t)F * sizeof(u64));
    c.sorted_hashes = (u64*)(p + off); off += scratch_align256((size_t)F * sizeof(u64));
    c.numbers = (uint32_t*)(p + off); off += scratch_align256((size_t)F * sizeof(uint32_t));
    c.sorted_numbers = (uint32_t*)(p + off); off += scratch_align256((size_t)F * sizeof(uint32_t));
    c.keep = (uint8_t*)(p + off); off += scratch_align256((size_t)F);
    c.fblk = (uint32_t*)(p + off); off += scratch_align256((size_t)fb * sizeof(uint32_t));
    c.fchunk = (uint32_t*)(p + off); off += scratch_align256((size_t)num_chunks(fb) * sizeof(uint32_t));
    c.referenced = (uint32_t*)(p + off); off += scratch_align256((size_t)V * sizeof(uint32_t));
    c.vremap = (uint32_t*)(p + off); off += scratch_align256((size_t)V * sizeof(uint32_t));
    c.vblk = (uint32_t*)(p + off); off += scratch_align256((size_t)vb * sizeof(uint32_t));
    c.vchunk = (uint32_t*)(p + off); off += scratch_align256((size_t)num_chunks(vb) * sizeof(uint32_t));
    c.sort_off = off;
    return c;
}

// hash_bits > 0, F > 0
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const Carve& c, uint32_t F, int hash_bits, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const u64*)c.hashes, c.sorted_hashes, (const uint32_t*)c.numbers, c.sorted_numbers,
                                              (size_t)F, 0, hash_bits, s);
}

}  // namespace

namespace trgl {

hipError_t mesh_clean_scratch_bytes(uint32_t n_faces, uint32_t n_vertices, int hash_bits, size_t* bytes) {
    const Carve c = carve(nullptr, n_faces, n_vertices);
    size_t tmp = 0;
    if (hash_bits > 0 && n_faces) {
        const hipError_t e = sort_pairs(nullptr, tmp, c, n_faces, hash_bits, nullptr);
        if (e != hipSuccess) return e;
    }
    *bytes = c.sort_off + scratch_align256(tmp);
    return hipSuccess;
}

hipError_t launch_mesh_clean(hipStream_t s, const CleanArgs& a, void* scratch, size_t scratch_bytes, const unsigned long long** totals) {
    const Carve c = carve(scratch, a.n_faces, a.n_vertices);
    const bool with_vertices = (a.P.flags & TRGL_CLEAN_VERTICES) != 0;
    if (scratch_bytes < c.sort_off || a.hash_bits < 0 || a.hash_bits > 64 || a.n_vertices == 0 || (a.n_faces == 0 && !with_vertices))
        return hipErrorInvalidValue;
    if (!with_vertices && (a.vremap_out || a.vfirsts_out || a.vertices_out)) return hipErrorInvalidValue;
    *totals = c.totals;
    const uint32_t fb = num_blocks(a.n_faces), vb = num_blocks(a.n_vertices);
    hipError_t e = hipMemsetAsync(c.totals, 0, 2 * sizeof(u64), s);
    if (e != hipSuccess) return e;
    if (a.n_faces) {
        if (a.P.flags & TRGL_CLEAN_DUPLICATES) {
            hipLaunchKernelGGL(k_clean_keys, dim3(fb), dim3(LOD_BLOCK), 0, s, a, c.hashes, c.numbers);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            const u64* sh = c.hashes; const uint32_t* sn = c.numbers;
            if (a.hash_bits > 0) {
                size_t tmp = scratch_bytes - c.sort_off;
                if ((e = sort_pairs((char*)scratch + c.sort_off, tmp, c, a.n_faces, a.hash_bits, s)) != hipSuccess) return e;
                sh = c.sorted_hashes; sn = c.sorted_numbers;
            }
            hipLaunchKernelGGL(k_clean_resolve, dim3(fb), dim3(LOD_BLOCK), 0, s, a, sh, sn, c.keep);
        } else {
            hipLaunchKernelGGL(k_clean_classify, dim3(fb), dim3(LOD_BLOCK), 0, s, a, c.keep);
        }
        hipLaunchKernelGGL(k_clean_fcount, dim3(fb), dim3(LOD_BLOCK), 0, s, c.keep, a.n_faces, c.fblk);
        launch_block_count_scan(s, c.fblk, fb, c.fchunk, c.totals);
    }
    uint32_t* vremap = nullptr;
    if (with_vertices) {
        vremap = a.vremap_out ? a.vremap_out : c.vremap;
        if ((e = hipMemsetAsync(c.referenced, 0, (size_t)a.n_vertices * sizeof(uint32_t), s)) != hipSuccess) return e;
        if (a.n_faces) hipLaunchKernelGGL(k_clean_mark, dim3(fb), dim3(LOD_BLOCK), 0, s, a, c.keep, c.referenced);
        hipLaunchKernelGGL(k_clean_vcount, dim3(vb), dim3(LOD_BLOCK), 0, s, c.referenced, a.n_vertices, c.vblk);
        launch_block_count_scan(s, c.vblk, vb, c.vchunk, c.totals + 1);
        hipLaunchKernelGGL(k_clean_vwrite, dim3(vb), dim3(LOD_BLOCK), 0, s, a, c.referenced, c.vblk, c.vchunk, c.totals + 1, vremap);
    }
    if (a.n_faces && (a.indices_out || a.face_firsts_out))
        hipLaunchKernelGGL(k_clean_fwrite, dim3(fb), dim3(LOD_BLOCK), 0, s, a, c.keep, c.fblk, c.fchunk, c.totals, vremap);
    return hipGetLastError();
}

hipError_t launch_mesh_clean_sort(hipStream_t s, uint32_t n_faces, uint32_t n_vertices, int hash_bits, void* scratch, size_t scratch_bytes) {
    const Carve c = carve(scratch, n_faces, n_vertices);
    if (scratch_bytes < c.sort_off || hash_bits < 1 || hash_bits > 64 || n_faces == 0) return hipErrorInvalidValue;
    size_t tmp = scratch_bytes - c.sort_off;
    return sort_pairs((char*)scratch + c.sort_off, tmp, c, n_faces, hash_bits, s);
}

hipError_t launch_lod_mean(hipStream_t s, const double* vertices, int stride, int mean_count, uint32_t n, const uint32_t* indices, uint32_t n_idx,
                           const void* weld_scratch, int hash_bits, uint32_t* referenced, double* records) {
    if (n == 0 || stride < 1 || mean_count < 1 || mean_count > stride) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(referenced, 0, (size_t)n * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (n_idx) hipLaunchKernelGGL(k_lod_mark_words, dim3(num_blocks(n_idx)), dim3(LOD_BLOCK), 0, s, indices, n_idx, n, referenced);
    hipLaunchKernelGGL(k_lod_mean, dim3(num_blocks(n)), dim3(LOD_BLOCK), 0, s, mesh_weld_pairs(weld_scratch, n, hash_bits), vertices, (uint32_t)stride,
                       (uint32_t)mean_count, n, (const uint32_t*)referenced, records);
    return hipGetLastError();
}

hipError_t launch_lod_compose(hipStream_t s, uint32_t n, const uint32_t* weld_remap, const uint32_t* vremap, uint32_t* remap_out,
                              const uint32_t* weld_firsts, const uint32_t* vfirsts, uint32_t* firsts_out) {
    if (n == 0 || (!remap_out && !firsts_out)) return hipSuccess;
    hipLaunchKernelGGL(k_lod_compose, dim3(num_blocks(n)), dim3(LOD_BLOCK), 0, s, n, weld_remap, vremap, remap_out, weld_firsts, vfirsts, firsts_out);
    return hipGetLastError();
}

}  // namespace trgl
