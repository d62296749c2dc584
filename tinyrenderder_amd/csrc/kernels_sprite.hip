// kernels_sprite.hip — point sprites and wide lines: one point or one segment becomes the two triangles of a quad (include/trgl.h:
// trgl_sprite_stage, trgl_line_stage and their draws), gfx950.
//
// The stage reads 24-40 bytes per primitive and writes about 300: it is a write stream, and a lane that stored its own two rows would
// make every store of a wave touch 64 lines 192 bytes apart.  So a block works in two steps over SPRITE_BLOCK primitives:
//   1. lane p computes quad p with sprite_core.h's functions (k_line_stage: both index loads, then both row loads, are issued before the
//      arithmetic) and leaves its 16 corner doubles in LDS, component-major with a pitch of SPRITE_BLOCK + 1 doubles: the writes of a
//      wave are conflict-free, and the reads below spread over the banks (bank = 2 (component + quad) mod 64).
//   2. the block's part of each output array is contiguous - 24 doubles of clip rows, 2 K of varyings, 2 colours per quad.  The lanes
//      walk it in units of 16 bytes (8 where the array is only 8-byte aligned; colours as dwords), a block's width apart, so every store
//      instruction of a wave covers contiguous memory.  A unit's doubles are looked up in LDS by sprite_core.h's tables; a sprite's
//      attribute doubles are read from the point's row again (they sit in L2: lane 1 fetched the row just before).
// One launch per call.  No atomics.  Every global index is compared with n (or n_points) before it becomes an address.
#include <hip/hip_runtime.h>
#include "launch.h"
#include "sprite_core.h"

namespace {

using namespace trgl;

constexpr int PITCH = SPRITE_BLOCK + 1;

// what step 1 leaves for step 2 (39 KiB: four blocks per CU)
struct QuadTile {
    double k[16][PITCH];
    double t[3][SPRITE_BLOCK];      // ta, tb, one (lines; a sprite's are constants)
    uint32_t col[SPRITE_BLOCK];
};

__device__ inline void tile_put(QuadTile& T, int p, const SpriteQuad& q, uint32_t col, bool with_t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) T.k[e][p] = q.k[e];
    if (with_t) { T.t[0][p] = q.ta; T.t[1][p] = q.tb; T.t[2][p] = q.one; }
    T.col[p] = col;
}

// double d of the block's clip rows
__device__ inline double tile_clip(const QuadTile& T, uint32_t d) {
    const uint32_t p = d / 24u;
    return T.k[quad_clip_index((int)(d - p * 24u))][p];
}

// Double d of the block's varyings rows, K doubles each.  LINES: the pairs come from T.t; else they are a sprite's constants and
// columns 6 .. K - 1 are the doubles at attr of the quad's point.
template <bool LINES>
__device__ inline double tile_vary(const QuadTile& T, uint32_t d, uint32_t K, const double* attr, uint32_t stride) {
    const uint32_t p = d / (2u * K), r = d - p * (2u * K), tri = r >= K ? 1u : 0u, c = r - tri * K;
    if (c >= 6u) return attr[(size_t)p * stride + (c - 6u)];
    const int sel = quad_vary_sel((int)tri, (int)c);
    if (LINES) return sel == 2 ? 0.0 : T.t[sel == 3 ? 2 : sel][p];
    return quad_vary(0.0, 1.0, 1.0, sel);
}

struct alignas(16) Pair { double a, b; };

// Step 2 for the nq quads of a block; the pointers are the block's own parts of the arrays.  The counts of doubles are even, so a
// 16-byte unit never crosses the end.
template <bool LINES>
__device__ inline void store_rows(const QuadTile& T, uint32_t nq, double* clip, double* vary, uint32_t K, const double* attr, uint32_t stride,
                                  uint32_t* colors) {
    const uint32_t tid = threadIdx.x;
    const uint32_t nclip = nq * 24u;
    if (((uintptr_t)clip & 15) == 0) {
#pragma unroll 4
        for (uint32_t d = 2u * tid; d < nclip; d += 2u * SPRITE_BLOCK)
            *reinterpret_cast<Pair*>(clip + d) = Pair{ tile_clip(T, d), tile_clip(T, d + 1u) };
    } else {
#pragma unroll 4
        for (uint32_t d = tid; d < nclip; d += SPRITE_BLOCK) clip[d] = tile_clip(T, d);
    }
    if (vary) {
        const uint32_t nvary = nq * 2u * K;
        if (((uintptr_t)vary & 15) == 0) {
#pragma unroll 2
            for (uint32_t d = 2u * tid; d < nvary; d += 2u * SPRITE_BLOCK)
                *reinterpret_cast<Pair*>(vary + d) = Pair{ tile_vary<LINES>(T, d, K, attr, stride), tile_vary<LINES>(T, d + 1u, K, attr, stride) };
        } else {
#pragma unroll 2
            for (uint32_t d = tid; d < nvary; d += SPRITE_BLOCK) vary[d] = tile_vary<LINES>(T, d, K, attr, stride);
        }
    }
    if (colors)
        for (uint32_t j = tid; j < 2u * nq; j += SPRITE_BLOCK) colors[j] = T.col[j >> 1];
}

__global__ __launch_bounds__(SPRITE_BLOCK) void k_sprite_stage(const SpriteArgs a) {
    __shared__ QuadTile T;
    const uint64_t base = (uint64_t)blockIdx.x * SPRITE_BLOCK;
    const uint32_t nq = (uint32_t)(a.n - base < (uint64_t)SPRITE_BLOCK ? a.n - base : (uint64_t)SPRITE_BLOCK);
    const uint32_t p = threadIdx.x;
    const double* rows = a.points + base * (uint64_t)a.stride;
    if (p < nq) {
        const double* row = rows + (size_t)p * a.stride;
        const double px = row[0], py = row[1], pz = row[2];
        const double s = a.P.size_offset >= 0 ? row[a.P.size_offset] : a.P.size;
        const uint32_t col = a.colors ? a.colors[base + p] : 0u;
        SpriteQuad q;
        sprite_quad(a.P, px, py, pz, s, &q);
        tile_put(T, (int)p, q, col, false);
    }
    __syncthreads();
    const uint32_t K = 6u + (uint32_t)a.P.n_attr;
    store_rows<false>(T, nq, a.clip_out + base * 24, a.vary_out ? a.vary_out + base * 2 * K : nullptr, K, rows + a.P.attr_offset, (uint32_t)a.stride,
                      a.colors ? a.colors_out + base * 2 : nullptr);
}

__global__ __launch_bounds__(SPRITE_BLOCK) void k_line_stage(const LineArgs a) {
    __shared__ QuadTile T;
    const uint64_t base = (uint64_t)blockIdx.x * SPRITE_BLOCK;
    const uint32_t nq = (uint32_t)(a.n - base < (uint64_t)SPRITE_BLOCK ? a.n - base : (uint64_t)SPRITE_BLOCK);
    const uint32_t p = threadIdx.x;
    if (p < nq) {
        const uint64_t j = base + p;
        uint64_t ia = 2 * j, ib = 2 * j + 1;
        if (a.indices) { const uint32_t i0 = a.indices[2 * j], i1 = a.indices[2 * j + 1]; ia = i0; ib = i1; }
        const bool ok = ia < a.n_points && ib < a.n_points;      // else neither is an address
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        uint32_t col = 0u;
        if (ok) {
            const double* ra = a.points + ia * (uint64_t)a.stride;
            const double* rb = a.points + ib * (uint64_t)a.stride;
            a0 = ra[0]; a1 = ra[1]; a2 = ra[2];
            b0 = rb[0]; b1 = rb[1]; b2 = rb[2];
            if (a.colors) col = a.colors[j];
        }
        SpriteQuad q;
        if (ok) line_quad(a.P, a0, a1, a2, b0, b1, b2, &q); else sprite_quad_zero(&q);
        if (q.one == 0.0) col = 0u;      // an all-zero quad has colour 0
        tile_put(T, (int)p, q, col, true);
    }
    __syncthreads();
    store_rows<true>(T, nq, a.clip_out + base * 24, a.vary_out ? a.vary_out + base * 12 : nullptr, 6u, nullptr, 0u,
                     a.colors ? a.colors_out + base * 2 : nullptr);
}

}  // namespace

namespace trgl {

void launch_sprite_stage(hipStream_t s, const SpriteArgs& a) {
    const uint64_t blocks = (a.n + SPRITE_BLOCK - 1) / SPRITE_BLOCK;
    hipLaunchKernelGGL(k_sprite_stage, dim3((unsigned)blocks), dim3(SPRITE_BLOCK), 0, s, a);
}

void launch_line_stage(hipStream_t s, const LineArgs& a) {
    const uint64_t blocks = (a.n + SPRITE_BLOCK - 1) / SPRITE_BLOCK;
    hipLaunchKernelGGL(k_line_stage, dim3((unsigned)blocks), dim3(SPRITE_BLOCK), 0, s, a);
}

}  // namespace trgl
