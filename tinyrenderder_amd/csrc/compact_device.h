// compact_device.h — device helpers of the kernels that keep some entries of an array and number them in their old order
// (kernels_weld.hip, kernels_lod.hip): the rank of a lane among the kept lanes of its block, contiguous stores of a block's piece of an
// output, and the move of the kept records of a block with the zero records behind the count.  Blocks of COMPACT_BLOCK lanes, four waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trgl_dev {

constexpr int COMPACT_BLOCK = 256;
typedef unsigned long long cu64;

// The rank of this lane among the lanes of its block with `mine` set, and the block's count of them (every lane).  s_w: 4 words of LDS.
__device__ __forceinline__ uint32_t block_rank(bool mine, uint32_t* s_w, uint32_t* count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const cu64 b = __ballot(mine);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_w[w];
    *count = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return rank;
}

// nd 64-bit words to g (8-byte aligned) as contiguous memory, word d = f(d): 16 bytes per lane, 8 at a head or tail
template <class F> __device__ __forceinline__ void store_run(cu64* g, cu64 nd, F f) {
    const cu64 head = (((uintptr_t)g & 15) != 0 && nd) ? 1u : 0u;
    if (head && threadIdx.x == 0) g[0] = f((cu64)0);
    const cu64 pairs = (nd - head) >> 1;
    for (cu64 p = threadIdx.x; p < pairs; p += COMPACT_BLOCK) {
        const cu64 d = head + 2 * p;
        *reinterpret_cast<ulonglong2*>(g + d) = make_ulonglong2(f(d), f(d + 1));
    }
    if (((nd - head) & 1u) && threadIdx.x == COMPACT_BLOCK - 1) g[nd - 1] = f(nd - 1);
}

// nw 32-bit words to g (4-byte aligned) as contiguous memory, word d = f(d): 16 bytes per lane, 4 per word of a head (up to 3 words in
// front of the first 16-byte boundary) and of a tail (up to 3 behind the last)
template <class F> __device__ __forceinline__ void store_run32(uint32_t* g, uint32_t nw, F f) {
    uint32_t head = (uint32_t)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;
    if (head > nw) head = nw;
    if (threadIdx.x < head) g[threadIdx.x] = f(threadIdx.x);
    const uint32_t quads = (nw - head) >> 2;
    for (uint32_t p = threadIdx.x; p < quads; p += COMPACT_BLOCK) {
        const uint32_t d = head + 4 * p;
        *reinterpret_cast<uint4*>(g + d) = make_uint4(f(d), f(d + 1), f(d + 2), f(d + 3));
    }
    const uint32_t tail0 = head + 4 * quads;
    if (threadIdx.x < nw - tail0) g[tail0 + threadIdx.x] = f(tail0 + threadIdx.x);
}

// The records a block keeps, as one contiguous piece of `out`: the block takes the entries v0 .. v0 + COMPACT_BLOCK of n, `count` of
// them are kept, s_src[r] is the lane of the kept one of rank r (LDS, written before a barrier), `base` its first new number and U the
// count of all kept entries (base + count <= U <= n).  Record base + r is the record of entry v0 + s_src[r] of `in`, S 64-bit words
// each, every 8 bytes loaded from the record they come from - a record that is not kept is never read.  Then the zero records of the
// block's own entries at or above U, contiguous again.  A record below U is written by its keeper's block alone and one at or above it
// by its own number's block alone.
__device__ __forceinline__ void move_kept_records(const cu64* in, cu64* out, cu64 S, const uint32_t* s_src, uint32_t count, uint32_t base,
                                                  uint32_t v0, uint32_t n, cu64 U) {
    const cu64* src = in + (cu64)v0 * S;
    if (count) {
        const cu64 nd = (cu64)count * S;
        if (nd <= 0xFFFFFFFFull) {
            const uint32_t S32 = (uint32_t)S;
            store_run(out + (cu64)base * S, nd, [&](cu64 d) { const uint32_t r = (uint32_t)d / S32; return src[(cu64)s_src[r] * S + ((uint32_t)d - r * S32)]; });
        } else {
            store_run(out + (cu64)base * S, nd, [&](cu64 d) { const cu64 r = d / S; return src[(cu64)s_src[r] * S + (d - r * S)]; });
        }
    }
    const cu64 end = (cu64)v0 + COMPACT_BLOCK < (cu64)n ? (cu64)v0 + COMPACT_BLOCK : (cu64)n;
    const cu64 z0 = U > (cu64)v0 ? U : (cu64)v0;
    if (z0 < end) store_run(out + z0 * S, (end - z0) * S, [](cu64) { return (cu64)0; });
}

}  // namespace trgl_dev
