// kernels_shadow.hip — the shadow post-pass (include/trgl.h: trgl_shadow_mask_image, trgl_image_modulate), gfx950.
//
//   k_shadow_mask : every camera pixel with a finite depth is carried into the light's screen space by the row-major M - the pixel centre
//                   (x + 0.5, y + 0.5, z, 1) of our_gl.cpp:149 through geometry.h's mat * vec, the guard on w of our_gl.cpp:94, a true
//                   division (geometry.h:117), the depth range test of our_gl.cpp:103 - and its depth there is compared with the
//                   (2r+1)^2 entries of the light's depth map around it; the byte is (unsigned char)(255.0 * (1.0 - occluded / total *
//                   darkness)), the shape of main.cpp:360-361,760.
//   k_modulate    : px[c] = (unsigned char)std::min(255.0, px[c] * (mask / 255.0)) (main.cpp:775-781) on an image in place.
// fp64 in the order include/trgl.h writes down, contraction off; the host paths (shim/trgl_image.h) are the same expressions.
//
// k_shadow_mask.  A thread owns four consecutive pixels of a row, a wave a tile of 32 x 8 pixels (8 lanes across, 8 rows) and a block four
// such tiles below one another: neighbouring camera pixels land close together in the light's map, so a compact tile keeps a wave's
// gathers within a few cache lines where a 256-pixel row would spread them along a line through the map.  The map itself is read from
// global memory: where a block's footprint in it lies depends on M, so nothing is staged.
// A row's groups of four start where the MASK is word aligned - the row is shifted left by (mask + y * w) & 3 pixels - so that every
// group that lies inside the row leaves as one 4-byte store whatever w and the base address are; only the groups cut by the row's ends
// store bytes.  With that shift the depths of every whole group sit at the same offset modulo 16: two 16-byte loads where that offset is
// 0 (always, when both base addresses are 16-byte aligned), else an 8-byte, a 16-byte and an 8-byte load.
// A block whose pixels are all background writes 255 and never reads M (it travels as a kernel argument).
//
// k_modulate.  The word-wise layout of k_composite, for every bpp: a thread owns four pixels = bpp words, read, multiplied and written
// back as words.  The groups start at the first pixel whose address is word aligned (for bpp = 4 there is none unless the base is: the
// groups then go byte by byte); the pixels before it and behind the last whole group are one thread's, byte by byte.
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "device_util.h"

namespace {

using namespace trgl;

using trgl_dev::dot4;

constexpr uint32_t MAX_GRID = 1u << 20;               // tiles beyond it are walked by a grid-stride loop

// tiles = tiles_x * tiles_y; tile t covers rows [ty * SHADOW_TILE_H, +SHADOW_TILE_H) and, in row y, the pixels
// [tx * SHADOW_TILE_W - shift(y), +SHADOW_TILE_W) with shift(y) = (mask + y * w) & 3; tiles_x = ceil((w + 3) / SHADOW_TILE_W).
// w * h and map_w * map_h fit an int.
__global__ __launch_bounds__(256) void k_shadow_mask(ShadowArgs a, uint32_t tiles_x, uint64_t tiles) {
    static_assert(SHADOW_TILE_W == 32 && SHADOW_TILE_H == 32, "a wave is 8 lanes x 4 pixels wide and 8 rows high, a block four waves high");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inf = __builtin_inf();
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t y = (int64_t)(t / tiles_x) * SHADOW_TILE_H + wave * 8 + (lane >> 3);
        const bool row_in = y < a.h;
        const int64_t row0 = y * a.w;                                                            // index of the row's first pixel
        const int shift = row_in ? (int)(((uintptr_t)a.mask + (uint64_t)row0) & 3) : 0;
        const int64_t x0 = (int64_t)(t % tiles_x) * SHADOW_TILE_W + 4 * (lane & 7) - shift;      // -3 .. w + 30
        const bool whole = row_in && x0 >= 0 && x0 + 4 <= a.w;
        double z[4] = { inf, inf, inf, inf };                                                    // a pixel outside the image stands as background
        if (whole) {
            const double* d = a.depth + row0 + x0;
            if (((uintptr_t)d & 15) == 0) {
                const double2 lo = *reinterpret_cast<const double2*>(d), hi = *reinterpret_cast<const double2*>(d + 2);
                z[0] = lo.x; z[1] = lo.y; z[2] = hi.x; z[3] = hi.y;
            } else {
                const double2 mid = *reinterpret_cast<const double2*>(d + 1);
                z[0] = d[0]; z[1] = mid.x; z[2] = mid.y; z[3] = d[3];
            }
        } else if (row_in) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j >= 0 && x0 + j < a.w) z[j] = a.depth[row0 + x0 + j];
        }
        const int any_finite = (__builtin_isfinite(z[0]) || __builtin_isfinite(z[1]) || __builtin_isfinite(z[2]) || __builtin_isfinite(z[3])) ? 1 : 0;
        uint32_t out = 0xffffffffu;                                                              // four lit pixels
        if (__syncthreads_or(any_finite)) {
            // where each pixel lands in the map, and the taps around it that lie inside the map (none for a pixel that stays lit)
            int x_lo[4], x_hi[4], y_lo[4], y_hi[4]; double limit[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x_lo[j] = 0; x_hi[j] = -1; y_lo[j] = 0; y_hi[j] = -1; limit[j] = 0.0;
                if (!__builtin_isfinite(z[j])) continue;                                         // step 1
                const double px = (double)(x0 + j) + 0.5, py = (double)y + 0.5;                  // step 2
                const double q3 = dot4(a.M + 12, px, py, z[j], 1.0);
                if (!(q3 > 1e-12)) continue;                                                     // step 3, our_gl.cpp:94
                const double s0 = dot4(a.M + 0, px, py, z[j], 1.0) / q3;                         // step 4, geometry.h:117
                const double s1 = dot4(a.M + 4, px, py, z[j], 1.0) / q3;
                const double s2 = dot4(a.M + 8, px, py, z[j], 1.0) / q3;
                if (!(__builtin_isfinite(s0) && __builtin_isfinite(s1) && __builtin_isfinite(s2))) continue;
                if (s2 < -1.0 || s2 > 1.0) continue;                                             // step 5, our_gl.cpp:103
                if (!(s0 >= 0.0 && s0 < (double)a.map_w && s1 >= 0.0 && s1 < (double)a.map_h)) continue;   // step 6
                const int ix = (int)s0, iy = (int)s1;                                            // step 7
                limit[j] = s2 - a.bias;
                x_lo[j] = max(ix - a.radius, 0); x_hi[j] = ix > a.map_w - 1 - a.radius ? a.map_w - 1 : ix + a.radius;   // (no sum above INT_MAX)
                y_lo[j] = max(iy - a.radius, 0); y_hi[j] = iy > a.map_h - 1 - a.radius ? a.map_h - 1 : iy + a.radius;
            }
            const double total = (double)((2 * a.radius + 1) * (2 * a.radius + 1));
            out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int occluded = 0;
                for (int ty = y_lo[j]; ty <= y_hi[j]; ++ty) {
                    const double* row = a.map + (size_t)ty * a.map_w;
                    for (int tx = x_lo[j]; tx <= x_hi[j]; ++tx) occluded += (row[tx] < limit[j]) ? 1 : 0;   // +inf and NaN never occlude
                }
                const double factor = 1.0 - ((double)occluded / total) * a.darkness;             // step 8, main.cpp:360-361
                out |= (uint32_t)(unsigned char)(255.0 * factor) << (8 * j);                     // main.cpp:760
            }
        }
        if (whole) {
            *reinterpret_cast<uint32_t*>(a.mask + row0 + x0) = out;                              // word aligned by the row's shift
        } else if (row_in) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j >= 0 && x0 + j < a.w) a.mask[row0 + x0 + j] = (uint8_t)(out >> (8 * j));
        }
    }
}

__device__ __forceinline__ uint8_t modulate_channel(uint32_t ch, double f) { return (unsigned char)dmin(255.0, (double)ch * f); }   // main.cpp:777-781

// pixels [i0, i1) byte by byte
__device__ void modulate_bytewise(uint8_t* px, int bpp, const uint8_t* mask, uint64_t i0, uint64_t i1) {
    const int nc = bpp < 3 ? bpp : 3;
    for (uint64_t i = i0; i < i1; ++i) {
        const double f = (double)mask[i] / 255.0;                                                // main.cpp:775
        for (int c = 0; c < nc; ++c) px[i * bpp + c] = modulate_channel(px[i * bpp + c], f);
    }
}

// Thread g < groups owns the pixels [head + 4 g, +4): BPP words at a word-aligned address when `wide`.  Thread `groups` owns the
// pixels before `head` and behind the last group.
template <int BPP>
__global__ __launch_bounds__(256) void k_modulate(uint8_t* __restrict__ px, const uint8_t* __restrict__ mask, uint64_t n, uint32_t head,
                                                  uint64_t groups, bool wide) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > groups) return;
    if (g == groups) {
        modulate_bytewise(px, BPP, mask, 0, head < n ? head : n);
        modulate_bytewise(px, BPP, mask, head + 4 * groups < n ? head + 4 * groups : n, n);
        return;
    }
    const uint64_t i0 = head + 4 * g;
    if (!wide) { modulate_bytewise(px, BPP, mask, i0, i0 + 4); return; }
    uint32_t* words = reinterpret_cast<uint32_t*>(px + i0 * BPP);
    uint32_t w[BPP];
#pragma unroll
    for (int k = 0; k < BPP; ++k) w[k] = words[k];
    const uint8_t* m = mask + i0;
    uint32_t mw;
    if (((uintptr_t)m & 3) == 0) mw = *reinterpret_cast<const uint32_t*>(m);
    else mw = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
    uint32_t o[BPP];
#pragma unroll
    for (int k = 0; k < BPP; ++k) o[k] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double f = (double)((mw >> (8 * j)) & 0xffu) / 255.0;                              // main.cpp:775
#pragma unroll
        for (int c = 0; c < BPP; ++c) {
            const int bi = BPP * j + c;
            const uint32_t ch = (w[bi >> 2] >> (8 * (bi & 3))) & 0xffu;
            o[bi >> 2] |= (c < 3 ? (uint32_t)modulate_channel(ch, f) : ch) << (8 * (bi & 3));    // alpha stays
        }
    }
#pragma unroll
    for (int k = 0; k < BPP; ++k) words[k] = o[k];
}

}  // namespace

namespace trgl {

void launch_shadow_mask(hipStream_t s, const ShadowArgs& a) {
    const uint32_t tiles_x = (uint32_t)(((int64_t)a.w + 3 + SHADOW_TILE_W - 1) / SHADOW_TILE_W);
    const uint64_t tiles = (uint64_t)tiles_x * (((uint64_t)a.h + SHADOW_TILE_H - 1) / SHADOW_TILE_H);
    hipLaunchKernelGGL(k_shadow_mask, dim3((uint32_t)(tiles < MAX_GRID ? tiles : MAX_GRID)), dim3(256), 0, s, a, tiles_x, tiles);
}

void launch_modulate(hipStream_t s, uint8_t* pixels, uint64_t npixels, int bpp, const uint8_t* mask) {
    // the first pixel at a word-aligned address: base + bpp * head = 0 (mod 4)
    const uint32_t mis = (uint32_t)((uintptr_t)pixels & 3);
    const bool wide = bpp != 4 || mis == 0;
    uint64_t head = !wide ? 0 : bpp == 1 ? (4 - mis) & 3 : bpp == 3 ? mis : 0;
    if (head > npixels) head = npixels;
    const uint64_t groups = (npixels - head) / 4;
    const dim3 grid((uint32_t)((groups + 1 + 255) / 256));
    if (bpp == 1) hipLaunchKernelGGL(k_modulate<1>, grid, dim3(256), 0, s, pixels, mask, npixels, (uint32_t)head, groups, wide);
    else if (bpp == 3) hipLaunchKernelGGL(k_modulate<3>, grid, dim3(256), 0, s, pixels, mask, npixels, (uint32_t)head, groups, wide);
    else hipLaunchKernelGGL(k_modulate<4>, grid, dim3(256), 0, s, pixels, mask, npixels, (uint32_t)head, groups, wide);
}

}  // namespace trgl
