// kernels_triorder.hip — a depth per group of triangles and the gather of rows under an order list (include/trgl.h:
// trgl_triangle_depths, trgl_order_stage, trgl_draw_ordered), gfx950.
//
//   k_triangle_depths : one thread per group of g triangles: the fold of triorder_core.h over the 3 g clip w of the group, in memory
//                       order.  w sits at byte 24 of each 32-byte vertex, so the loads of a wave touch every 32-byte sector of its
//                       64 groups exactly once: the kernel reads the n * 96 bytes of the clip array and writes 8 bytes per group.
//   k_gather_rows     : out group p = in group order[p], a group being g consecutive rows (g * row bytes, contiguous on both sides).
//                       The output is cut into units of 16, 8 or 4 bytes; a thread moves GATHER_UNROLL units that lie a block's width
//                       apart, so every store instruction of a wave is contiguous and the lanes that read one group read it as a whole,
//                       in order.  All of a thread's loads are issued before its first store: GATHER_UNROLL groups in flight per lane.
//                       An entry >= G never becomes an address: its units are stored as zeros.  One launch per array; the unit (the
//                       widest that the pointers and the row length allow) changes how the bytes travel, not the bytes.
// No atomics, no LDS.
#include <hip/hip_runtime.h>
#include "launch.h"
#include "triorder_core.h"

namespace {

using namespace trgl;

template <int MODE>
__global__ __launch_bounds__(256) void k_triangle_depths(const double* __restrict__ clip, uint32_t G, uint32_t g,
                                                         unsigned long long* __restrict__ depth_bits) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= G) return;
    const double* w = clip + (size_t)q * (size_t)g * 12 + 3;      // w of vertex v: w[4 v]
    double w0 = w[0], w1 = w[4], w2 = w[8];
    double acc = tri_depth_first(MODE, w0);
    acc = tri_depth_step(MODE, acc, w1);
    acc = tri_depth_step(MODE, acc, w2);
    for (uint32_t t = 1; t < g; ++t) {
        w += 12;
        w0 = w[0]; w1 = w[4]; w2 = w[8];
        acc = tri_depth_step(MODE, acc, w0);
        acc = tri_depth_step(MODE, acc, w1);
        acc = tri_depth_step(MODE, acc, w2);
    }
    depth_bits[q] = tri_depth_bits(acc);
}

struct alignas(16) Unit16 { unsigned long long a, b; };

template <class U> __device__ inline U zero_unit();
template <> __device__ inline Unit16 zero_unit<Unit16>() { return Unit16{ 0ull, 0ull }; }
template <> __device__ inline unsigned long long zero_unit<unsigned long long>() { return 0ull; }
template <> __device__ inline uint32_t zero_unit<uint32_t>() { return 0u; }

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;
constexpr int GATHER_BLOCK_UNITS = GATHER_THREADS * GATHER_UNROLL;

// in / out in units of U; upg: units per group; total = n_order * upg units of output; G: groups of the input
template <class U>
__global__ __launch_bounds__(GATHER_THREADS) void k_gather_rows(const U* __restrict__ in, U* __restrict__ out, const uint32_t* __restrict__ order,
                                                                unsigned long long upg, unsigned long long total, uint32_t G) {
    const unsigned long long start = (unsigned long long)blockIdx.x * GATHER_BLOCK_UNITS;      // (uniform: one division per block)
    const unsigned long long p0 = start / upg, r0 = start % upg;
    const bool narrow = upg <= 0xffff0000ull;      // r0 + j then fits 32 bits: the per-unit division is a 32-bit one
    unsigned long long dst[GATHER_UNROLL], src[GATHER_UNROLL];
    uint32_t entry[GATHER_UNROLL];
    bool live[GATHER_UNROLL];
#pragma unroll
    for (int k = 0; k < GATHER_UNROLL; ++k) {
        const uint32_t j = threadIdx.x + k * GATHER_THREADS;
        dst[k] = start + j;
        live[k] = dst[k] < total;
        unsigned long long dp, off;
        if (narrow) { const uint32_t t = (uint32_t)r0 + j, u = (uint32_t)upg; dp = t / u; off = t % u; }
        else { const unsigned long long t = r0 + j; dp = t / upg; off = t % upg; }
        entry[k] = live[k] ? order[p0 + dp] : 0xffffffffu;
        src[k] = off;
    }
    U v[GATHER_UNROLL];
#pragma unroll
    for (int k = 0; k < GATHER_UNROLL; ++k)
        v[k] = entry[k] < G ? in[(unsigned long long)entry[k] * upg + src[k]] : zero_unit<U>();
#pragma unroll
    for (int k = 0; k < GATHER_UNROLL; ++k)
        if (live[k]) out[dst[k]] = v[k];
}

template <class U>
void gather(hipStream_t s, const void* in, void* out, const uint32_t* order, unsigned long long group_bytes, unsigned long long n_order, uint32_t G) {
    const unsigned long long upg = group_bytes / sizeof(U), total = n_order * upg;
    const unsigned long long blocks = (total + GATHER_BLOCK_UNITS - 1) / GATHER_BLOCK_UNITS;
    hipLaunchKernelGGL(k_gather_rows<U>, dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, s, (const U*)in, (U*)out, order, upg, total, G);
}

}  // namespace

namespace trgl {

void launch_triangle_depths(hipStream_t s, const double* clip, uint32_t G, uint32_t g, int mode, double* depths) {
    const dim3 grid((G + 255) / 256), block(256);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(depths);
    if (mode == 0) hipLaunchKernelGGL(k_triangle_depths<0>, grid, block, 0, s, clip, G, g, out);
    else if (mode == 1) hipLaunchKernelGGL(k_triangle_depths<1>, grid, block, 0, s, clip, G, g, out);
    else hipLaunchKernelGGL(k_triangle_depths<2>, grid, block, 0, s, clip, G, g, out);
}

void launch_gather_rows(hipStream_t s, const void* in, void* out, uint32_t row_bytes, const uint32_t* order, uint32_t n_order, uint32_t G, uint32_t g) {
    const unsigned long long group_bytes = (unsigned long long)row_bytes * g;
    const uintptr_t both = (uintptr_t)in | (uintptr_t)out;
    if (row_bytes % 16 == 0 && (both & 15) == 0) gather<Unit16>(s, in, out, order, group_bytes, n_order, G);
    else if (row_bytes % 8 == 0 && (both & 7) == 0) gather<unsigned long long>(s, in, out, order, group_bytes, n_order, G);
    else gather<uint32_t>(s, in, out, order, group_bytes, n_order, G);
}

}  // namespace trgl
