// kernels_image.hip — TGAImage::gaussian_blur (tgaimage.cpp:271-324) and TGAImage::scale (tgaimage.cpp:246-267) for an image in HBM,
// byte for byte.
//
// The blur is separable and every output byte is its own serial chain: a float sum from 0.0f over the taps k = -radius..radius, in that
// order, of byte(clamped neighbour) * weight[k] - one rounded multiply and one rounded add per tap (the reference is built without
// contraction) - truncated to a byte.  float addition is not associative, so the chain is never split, reordered or fused: one thread
// owns an output byte and walks its taps front to back.  What is shared is the DATA: neighbouring outputs read overlapping bytes, so a
// workgroup stages its tile plus a clamped halo of `radius` pixels in LDS once and every thread reads its taps from there.
//   k_blur_h   rows are w * bpp bytes and the taps of a byte lie bpp bytes apart, whatever the channel: a tile is BLUR_H_BYTES consecutive
//              bytes of BLUR_H_ROWS rows, thread t owns byte t of each row
//   k_blur_v   the taps of a byte lie one row apart: a tile is BLUR_V_BYTES consecutive bytes of BLUR_V_ROWS rows, a wave owns every fourth
//              row of it, a lane one byte column
//   k_blur_far radius > BLUR_LDS_RADIUS (the halo no longer fits the tile): one thread per output byte reads its clamped taps from global
//              memory; the same chain, the same bits
// Global accesses are single bytes at consecutive addresses across a wave - images are only 1-byte aligned (bpp = 3 gives nothing better
// from the second row on) - except inside the clamped halo, where lanes repeat the edge pixel.  The weights are read through a
// wave-uniform index.  The horizontal pass writes a scratch image that the vertical pass reads: the intermediate is quantised to bytes
// exactly as the reference's second copy is (tgaimage.cpp:306).
// The scale is an integer gather: a tile is SCALE_BYTES consecutive bytes of SCALE_ROWS output rows, the source column of a byte is
// computed once for all rows of the tile.
#include <hip/hip_runtime.h>
#include "launch.h"

namespace {

using namespace trgl;

// j / bpp for bpp in {1, 3, 4} and j < 65536 without a division
__device__ __forceinline__ uint32_t div_bpp(uint32_t j, int bpp) { return bpp == 1 ? j : bpp == 4 ? j >> 2 : (j * 0xAAABu) >> 17; }

__device__ __forceinline__ float tap(float acc, uint8_t byte, float weight) { return __fadd_rn(acc, __fmul_rn((float)(int)byte, weight)); }
__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

constexpr int BLUR_H_SPAN = BLUR_H_BYTES + 2 * BLUR_LDS_RADIUS * 4;        // a tile row with the widest halo (bpp = 4) on both sides
constexpr uint32_t MAX_GRID = 1u << 20;                                    // tiles beyond it are walked by a grid-stride loop

// tiles = bands * segs; tile t covers bytes [seg * BLUR_H_BYTES, +BLUR_H_BYTES) of rows [band * BLUR_H_ROWS, +BLUR_H_ROWS).
// radius <= BLUR_LDS_RADIUS, bpp <= 4.
__global__ __launch_bounds__(256) void k_blur_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int bpp, int radius,
                                                const float* __restrict__ weights, uint32_t segs, uint64_t tiles) {
    __shared__ uint8_t lds[BLUR_H_ROWS][BLUR_H_SPAN];
    const int64_t row_bytes = (int64_t)w * bpp;
    const int span = BLUR_H_BYTES + 2 * radius * bpp;
    const int tid = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t b0 = (uint32_t)(t % segs) * BLUR_H_BYTES;          // first byte of the tile in its row (row_bytes fits an int)
        const int64_t y0 = (int64_t)(t / segs) * BLUR_H_ROWS;
        const uint32_t px0 = b0 / (uint32_t)bpp, ch0 = b0 - px0 * (uint32_t)bpp;
        // lds[r][i] = the byte at b0 - radius * bpp + i of row y0 + r, pixels clamped to 0..w-1 (tgaimage.cpp:294); rows past the image repeat the last
        for (int i = tid; i < span; i += 256) {
            const uint32_t j = ch0 + (uint32_t)i, dp = div_bpp(j, bpp);
            const int64_t px = clamp64((int64_t)px0 - radius + dp, 0, w - 1);
            const int64_t off = px * bpp + (j - dp * (uint32_t)bpp);
#pragma unroll
            for (int r = 0; r < BLUR_H_ROWS; ++r) lds[r][i] = src[clamp64(y0 + r, 0, h - 1) * row_bytes + off];
        }
        __syncthreads();
        float acc[BLUR_H_ROWS];
#pragma unroll
        for (int r = 0; r < BLUR_H_ROWS; ++r) acc[r] = 0.0f;
        for (int k = 0; k <= 2 * radius; ++k) {                            // ascending k: the reference's order (tgaimage.cpp:293)
            const float weight = weights[k];
#pragma unroll
            for (int r = 0; r < BLUR_H_ROWS; ++r) acc[r] = tap(acc[r], lds[r][tid + k * bpp], weight);
        }
        const int64_t b = (int64_t)b0 + tid;
        if (b < row_bytes) {
#pragma unroll
            for (int r = 0; r < BLUR_H_ROWS; ++r)
                if (y0 + r < h) dst[(y0 + r) * row_bytes + b] = (uint8_t)(int)acc[r];
        }
        __syncthreads();
    }
}

constexpr int BLUR_V_PER_THREAD = BLUR_V_ROWS / 4;                         // four waves share the rows of a tile
// tiles = bands * cblocks; tile t covers bytes [cblock * BLUR_V_BYTES, +BLUR_V_BYTES) of rows [band * BLUR_V_ROWS, +BLUR_V_ROWS).
// radius <= BLUR_LDS_RADIUS.
__global__ __launch_bounds__(256) void k_blur_v(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t row_bytes, int h, int radius,
                                                const float* __restrict__ weights, uint32_t cblocks, uint64_t tiles) {
    static_assert(BLUR_V_BYTES == 64, "a wave stages and owns one 64-byte row segment at a time");
    __shared__ uint8_t lds[BLUR_V_ROWS + 2 * BLUR_LDS_RADIUS][BLUR_V_BYTES];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int span = BLUR_V_ROWS + 2 * radius;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t col = (int64_t)(t % cblocks) * BLUR_V_BYTES + cx;
        const int64_t y0 = (int64_t)(t / cblocks) * BLUR_V_ROWS;
        const int64_t colc = col < row_bytes ? col : row_bytes - 1;
        // lds[i] = row y0 - radius + i clamped to 0..h-1 (tgaimage.cpp:313)
        for (int i = ry; i < span; i += 4) lds[i][cx] = src[clamp64(y0 - radius + i, 0, h - 1) * row_bytes + colc];
        __syncthreads();
        float acc[BLUR_V_PER_THREAD];
#pragma unroll
        for (int e = 0; e < BLUR_V_PER_THREAD; ++e) acc[e] = 0.0f;
        for (int k = 0; k <= 2 * radius; ++k) {                            // ascending k (tgaimage.cpp:312)
            const float weight = weights[k];
#pragma unroll
            for (int e = 0; e < BLUR_V_PER_THREAD; ++e) acc[e] = tap(acc[e], lds[ry + 4 * e + k][cx], weight);
        }
        if (col < row_bytes) {
#pragma unroll
            for (int e = 0; e < BLUR_V_PER_THREAD; ++e) {
                const int64_t y = y0 + ry + 4 * e;
                if (y < h) dst[y * row_bytes + col] = (uint8_t)(int)acc[e];
            }
        }
        __syncthreads();
    }
}

// Any radius: one thread per output byte (grid-stride), its clamped taps read from global memory.
template <bool VERTICAL>
__global__ __launch_bounds__(256) void k_blur_far(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int bpp, int radius,
                                                  const float* __restrict__ weights, uint64_t nbytes) {
    const uint32_t row_bytes = (uint32_t)w * (uint32_t)bpp;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes; i += step) {
        const uint32_t y = (uint32_t)(i / row_bytes), b = (uint32_t)(i - (uint64_t)y * row_bytes);
        float acc = 0.0f;
        if (VERTICAL) {
            for (int k = 0; k <= 2 * radius; ++k)
                acc = tap(acc, src[clamp64((int64_t)y - radius + k, 0, h - 1) * row_bytes + b], weights[k]);
        } else {
            const uint32_t px = b / (uint32_t)bpp, ch = b - px * (uint32_t)bpp;
            const uint8_t* row = src + (uint64_t)y * row_bytes + ch;
            for (int k = 0; k <= 2 * radius; ++k)
                acc = tap(acc, row[clamp64((int64_t)px - radius + k, 0, w - 1) * bpp], weights[k]);
        }
        dst[i] = (uint8_t)(int)acc;
    }
}

// tiles = bands * segs; tile t covers bytes [seg * SCALE_BYTES, +SCALE_BYTES) of output rows [band * SCALE_ROWS, +SCALE_ROWS).
// (w2 - 1) * w and (h2 - 1) * h fit an int (the host checked), so the products below fit 32 bits.
__global__ __launch_bounds__(256) void k_scale(const uint8_t* __restrict__ src, int w, int h, int bpp, uint8_t* __restrict__ dst, int w2, int h2,
                                               uint32_t segs, uint64_t tiles) {
    const int64_t row2 = (int64_t)w2 * bpp, row = (int64_t)w * bpp;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t b0 = (uint32_t)(t % segs) * SCALE_BYTES;
        const int64_t y0 = (int64_t)(t / segs) * SCALE_ROWS;
        const uint32_t px0 = b0 / (uint32_t)bpp, j = b0 - px0 * (uint32_t)bpp + threadIdx.x, dp = div_bpp(j, bpp);
        const uint32_t x = px0 + dp, ch = j - dp * (uint32_t)bpp;
        const int64_t b = (int64_t)b0 + threadIdx.x;
        if (b >= row2) continue;
        const int64_t soff = (int64_t)(x * (uint32_t)w / (uint32_t)w2) * bpp + ch;            // tgaimage.cpp:253
#pragma unroll
        for (int r = 0; r < SCALE_ROWS; ++r) {
            const int64_t y = y0 + r;
            if (y < h2) dst[y * row2 + b] = src[(int64_t)((uint32_t)y * (uint32_t)h / (uint32_t)h2) * row + soff];   // :254
        }
    }
}

uint32_t grid_for(uint64_t tiles) { return (uint32_t)(tiles < MAX_GRID ? tiles : MAX_GRID); }

}  // namespace

namespace trgl {

void launch_image_blur(hipStream_t s, uint8_t* pixels, int w, int h, int bpp, int radius, const float* weights, uint8_t* tmp) {
    const uint64_t row_bytes = (uint64_t)w * bpp, nbytes = row_bytes * h;
    if (radius <= BLUR_LDS_RADIUS) {
        const uint32_t segs = (uint32_t)((row_bytes + BLUR_H_BYTES - 1) / BLUR_H_BYTES);
        const uint64_t htiles = (uint64_t)segs * (((uint64_t)h + BLUR_H_ROWS - 1) / BLUR_H_ROWS);
        hipLaunchKernelGGL(k_blur_h, dim3(grid_for(htiles)), dim3(256), 0, s, pixels, tmp, w, h, bpp, radius, weights, segs, htiles);
        const uint32_t cblocks = (uint32_t)((row_bytes + BLUR_V_BYTES - 1) / BLUR_V_BYTES);
        const uint64_t vtiles = (uint64_t)cblocks * (((uint64_t)h + BLUR_V_ROWS - 1) / BLUR_V_ROWS);
        hipLaunchKernelGGL(k_blur_v, dim3(grid_for(vtiles)), dim3(256), 0, s, tmp, pixels, (int64_t)row_bytes, h, radius, weights, cblocks, vtiles);
    } else {
        const dim3 grid(grid_for((nbytes + 255) / 256));
        hipLaunchKernelGGL(k_blur_far<false>, grid, dim3(256), 0, s, pixels, tmp, w, h, bpp, radius, weights, nbytes);
        hipLaunchKernelGGL(k_blur_far<true>, grid, dim3(256), 0, s, tmp, pixels, w, h, bpp, radius, weights, nbytes);
    }
}

void launch_image_scale(hipStream_t s, const uint8_t* src, int w, int h, int bpp, uint8_t* dst, int w2, int h2) {
    const uint64_t row2 = (uint64_t)w2 * bpp;
    const uint32_t segs = (uint32_t)((row2 + SCALE_BYTES - 1) / SCALE_BYTES);
    const uint64_t tiles = (uint64_t)segs * (((uint64_t)h2 + SCALE_ROWS - 1) / SCALE_ROWS);
    hipLaunchKernelGGL(k_scale, dim3(grid_for(tiles)), dim3(256), 0, s, src, w, h, bpp, dst, w2, h2, segs, tiles);
}

}  // namespace trgl
