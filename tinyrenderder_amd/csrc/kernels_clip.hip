// kernels_clip.hip — the clip stage on the device (include/trgl.h: trgl_clip_stage), gfx950.  The arithmetic is clip_core.h's, the very
// functions the host path compiles; what is written here is how the work is laid over the machine.
//
//   k_clip_count   : a block takes CLIP_BLOCK_TRIS consecutive triangles, one per lane, reads only their 12 clip doubles, classifies them
//                    and leaves the block's number of output triangles (0, 1 or 2 each) in blk[block].
//   k_clip_scan_chunks : the lower level of the scan - block c turns the CLIP_SCAN_CHUNK entries blk[c * CLIP_SCAN_CHUNK ..) into their
//                    exclusive prefix sums, in place, and leaves their total in chunk[c].
//   k_clip_scan_top: the upper level - one block turns chunk[] into its exclusive prefix sums, in place (CLIP_SCAN_CHUNK entries per
//                    round with the running total carried over), and leaves the grand total in *total.
//   k_clip_scatter : the blocks of k_clip_count classify again, scan their counts and write their outputs behind
//                    chunk[block / CLIP_SCAN_CHUNK] + blk[block]: input order is output order, and no atomic decides where anything goes.
//
// Both per-triangle kernels bring their block's clip coordinates into LDS with coalesced 8-byte loads (a lane's own triangle is 96 bytes
// away from its neighbour's: read directly, every load instruction would touch 48 cache lines).  8 bytes is all the alignment the inputs have.
// k_clip_scatter then treats a block's outputs as what they are in memory, three contiguous streams: (outputs * 12) clip doubles,
// (outputs * K) varying doubles and (outputs) colour words.  The whole block walks each stream element by element - thread e, e + 256, ... -
// so that stores are contiguous across the lanes of a wave and loads nearly so (a triangle that passes through unchanged, the common
// case, is a straight copy).  An element looks up its output's source triangle and class in LDS and is copied, or interpolated with the
// triangle's two parameters t, which the classifying lane left in LDS (one division per cut edge, not one per element).
#include <hip/hip_runtime.h>
#include "clip_core.h"
#include "launch.h"

namespace {

using namespace trgl;

constexpr int T = CLIP_BLOCK_TRIS;
static_assert(T == 256, "one triangle per lane of a 256-thread block");

// the sum of v over the block (valid in every thread) and, in *excl, the sum over the threads before this one; s_w: 4 words of LDS
// (an own copy, not device_util.h's block_excl_scan: written that way, all four kernels of this file get other instructions)
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_w, uint32_t* excl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();                                   // s_w may still be read from an earlier round
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const uint32_t x = s_w[w]; total += x; if (w < wave) before += x; }
    *excl = before + inc - v;
    return total;
}

// the clip doubles of triangles [first, first + m) into s_clip, m <= T
__device__ __forceinline__ void stage_clip(const double* __restrict__ clip, uint64_t first, uint32_t m, double* s_clip) {
    const double* src = clip + first * 12;
    for (uint32_t e = threadIdx.x; e < m * 12; e += T) s_clip[e] = src[e];
    __syncthreads();
}

__global__ __launch_bounds__(T) void k_clip_count(ClipArgs a, uint32_t* __restrict__ blk) {
    __shared__ double s_clip[T * 12];
    __shared__ uint32_t s_w[4];
    const uint64_t first = (uint64_t)blockIdx.x * T;
    const uint32_t m = a.n - first < T ? (uint32_t)(a.n - first) : T;
    stage_clip(a.clip, first, m, s_clip);
    uint32_t cnt = 0;
    if (threadIdx.x < m) {
        double t[2];
        cnt = (uint32_t)clip_outputs(clip_classify(s_clip + threadIdx.x * 12, a.plane, t));
    }
    uint32_t excl;
    const uint32_t total = block_scan(cnt, s_w, &excl);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

static_assert(CLIP_SCAN_CHUNK == 256, "block_scan is written for four waves");

__global__ __launch_bounds__(CLIP_SCAN_CHUNK) void k_clip_scan_chunks(uint32_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ chunk) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * CLIP_SCAN_CHUNK + threadIdx.x;
    const uint32_t v = i < nblk ? blk[i] : 0;
    uint32_t excl;
    const uint32_t sum = block_scan(v, s_w, &excl);
    if (i < nblk) blk[i] = excl;
    if (threadIdx.x == 0) chunk[blockIdx.x] = sum;
}

// (the outputs of a call are fewer than 2^32: n < 2^31)
__global__ __launch_bounds__(CLIP_SCAN_CHUNK) void k_clip_scan_top(uint32_t* __restrict__ chunk, uint32_t nchunks, unsigned long long* __restrict__ total) {
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nchunks; base += CLIP_SCAN_CHUNK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nchunks ? chunk[i] : 0;
        uint32_t excl;
        const uint32_t sum = block_scan(v, s_w, &excl);
        if (i < nchunks) chunk[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(T) void k_clip_scatter(ClipArgs a, const uint32_t* __restrict__ blk, const uint32_t* __restrict__ chunk) {
    __shared__ double s_clip[T * 12];
    __shared__ double s_t[T * 2];
    __shared__ uint16_t s_src[2 * T];                  // per output of the block: source triangle << 1 | which output of it
    __shared__ uint8_t s_code[T];
    __shared__ uint32_t s_w[4];
    const uint64_t first = (uint64_t)blockIdx.x * T;
    const uint32_t m = a.n - first < T ? (uint32_t)(a.n - first) : T;
    stage_clip(a.clip, first, m, s_clip);
    int code = CLIP_DROP;
    double t[2] = { 0.0, 0.0 };
    if (threadIdx.x < m) code = clip_classify(s_clip + threadIdx.x * 12, a.plane, t);
    const uint32_t cnt = (uint32_t)clip_outputs(code);
    uint32_t lo;
    const uint32_t outs = block_scan(cnt, s_w, &lo);
    s_code[threadIdx.x] = (uint8_t)code;
    s_t[2 * threadIdx.x] = t[0]; s_t[2 * threadIdx.x + 1] = t[1];
    for (uint32_t w = 0; w < cnt; ++w) s_src[lo + w] = (uint16_t)(threadIdx.x << 1 | w);
    __syncthreads();
    if (outs == 0) return;
    const uint64_t obase = (uint64_t)chunk[blockIdx.x / CLIP_SCAN_CHUNK] + blk[blockIdx.x];      // outputs before this block's

    double* co = a.clip_out + obase * 12;
    for (uint32_t e = threadIdx.x; e < outs * 12; e += T) {
        const uint32_t o = e / 12, c = e - o * 12, src = s_src[o], tl = src >> 1;
        const int cd = s_code[tl];
        const double* tri = s_clip + tl * 12;
        double v = tri[c];
        if (cd != CLIP_PASS) {
            int va, vb, ts;
            clip_slot(cd, (int)(src & 1), (int)(c >> 2), &va, &vb, &ts);
            const double xa = tri[4 * va + (c & 3)];
            v = va == vb ? xa : clip_lerp(xa, tri[4 * vb + (c & 3)], s_t[2 * tl + ts]);
        }
        co[e] = v;
    }
    if (a.K) {
        const uint32_t K = (uint32_t)a.K;
        double* vo = a.vary_out + obase * K;
        const double* vi = a.vary + first * K;
        for (uint32_t e = threadIdx.x; e < outs * K; e += T) {
            const uint32_t o = e / K, c = e - o * K, src = s_src[o], tl = src >> 1;
            vo[e] = clip_emit_vary(vi + (size_t)tl * K, (int)c, a.tab.slot[c], s_code[tl], (int)(src & 1), s_t + 2 * tl);
        }
    }
    if (a.colors)
        for (uint32_t o = threadIdx.x; o < outs; o += T) a.colors_out[obase + o] = a.colors[first + (s_src[o] >> 1)];
}

}  // namespace

namespace trgl {

uint32_t clip_num_blocks(uint64_t n) { return (uint32_t)((n + CLIP_BLOCK_TRIS - 1) / CLIP_BLOCK_TRIS); }
size_t clip_scratch_words(uint64_t n) { const size_t nblk = clip_num_blocks(n); return nblk + (nblk + CLIP_SCAN_CHUNK - 1) / CLIP_SCAN_CHUNK; }

void launch_clip_stage(hipStream_t s, const ClipArgs& a, uint32_t* scratch, unsigned long long* total) {
    const uint32_t nblk = clip_num_blocks(a.n), nchunks = (nblk + CLIP_SCAN_CHUNK - 1) / CLIP_SCAN_CHUNK;
    uint32_t* blk = scratch; uint32_t* chunk = scratch + nblk;
    if (nblk) {
        hipLaunchKernelGGL(k_clip_count, dim3(nblk), dim3(T), 0, s, a, blk);
        hipLaunchKernelGGL(k_clip_scan_chunks, dim3(nchunks), dim3(CLIP_SCAN_CHUNK), 0, s, blk, nblk, chunk);
    }
    hipLaunchKernelGGL(k_clip_scan_top, dim3(1), dim3(CLIP_SCAN_CHUNK), 0, s, chunk, nchunks, total);
    if (nblk) hipLaunchKernelGGL(k_clip_scatter, dim3(nblk), dim3(T), 0, s, a, blk, chunk);
}

}  // namespace trgl
