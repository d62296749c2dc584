// kernels_resolve.hip — the exact integer box filter of box_core.h for an image in HBM (trgl_image_downsample, trgl_framebuffer_resolve,
// trgl_texture_from_image / _from_framebuffer): f x f source bytes of a channel become one output byte.  New work, the reference has none.
//
// A streaming kernel: f source rows in, one output row out, every source byte read once.  Integer sums commute, so unlike the blur of
// kernels_image.hip nothing forces one-byte accesses or one thread per output byte.
//   tile     RES_BYTES consecutive bytes of RES_ROWS output rows (the last tile of a row or of the image is ragged).  The source of one
//            tile row is one segment of `len` = pixels * f * bpp consecutive bytes in each of f source rows.
//   staging  a thread owns 16 consecutive bytes of the segment and adds them up over the f source rows in registers, as eight dwords of
//            two 16-bit sums each (f * 255 <= 4080).  A source row starts at any byte (bpp = 3, odd w, a caller's sub-image), and each of
//            the f rows at another one: the thread reads the ALIGNED 16-byte word that holds its first byte and, unless that byte sits at
//            the word's start, the next word, and shifts the pair right by address & 15 bytes.  The first word always holds a byte of
//            the image; the second is read only when it starts before the 16-byte boundary that ends the image, and counts as zero
//            otherwise (those bytes belong to no output).  So no word without a byte of the image is read, and a word that holds one
//            lies in that byte's page.  The column sums go to LDS as 16-bit values, two 16-byte stores per thread.
//            As many tile rows as fit the LDS array are staged at once (all RES_ROWS up to f = 3, three or four at f = 4, one at f = 16).
//   compute  a thread produces four consecutive output bytes per tile row: per byte f reads of the column sums, bpp apart, then
//            (sum + f * f / 2) / (f * f) as a multiplication (box_core.h).  j / bpp without a division, as in kernels_image.hip.
//   stores   an output row starts at any byte too: the four bytes of a thread begin at the row's first 4-byte boundary at or before the
//            tile, so all complete groups go out as aligned dwords and only the ragged ends of a tile row as single bytes.  Nothing
//            outside dst is written: the zero tail of a texture and a caller's neighbouring bytes survive.
// One launch per call, one workgroup per tile, no loop over tiles, no atomics.
// Factor 1 is not this kernel but a device-to-device hipMemcpyAsync of the w * h * bpp bytes on the same stream (launch_box_filter):
// the filter is the identity there, and both give the same bytes.  No shape needs a fallback: the widest segment (f = 16) fits the array.
#include <hip/hip_runtime.h>
#include "box_core.h"
#include "launch.h"

namespace {

using namespace trgl;

constexpr int RES_BYTES = 1024, RES_ROWS = 4;              // tile: bytes of an output row (four per thread) x output rows
constexpr int RES_THREADS = 256;
// the longest segment: the pixels that RES_BYTES bytes touch (one more than they fill when the tile starts inside a pixel) * 16 * bpp
constexpr int res_len(int bpp) { return ((RES_BYTES + bpp - 1) / bpp + 1) * bpp * TRGL_MAX_BOX_FACTOR; }
constexpr int res_max(int a, int b) { return a > b ? a : b; }
constexpr int RES_SPAN = (res_max(res_len(1), res_max(res_len(3), res_len(4))) + 15) & ~15;      // column sums in LDS
static_assert(RES_BYTES == 4 * RES_THREADS, "a thread owns four bytes of a tile row");
static_assert(RES_BYTES + 4 < 65536, "div_bpp");
static_assert(RES_SPAN * 2 <= 64 * 1024, "LDS");

// j / bpp for bpp in {1, 3, 4} and j < 65536 without a division
__device__ __forceinline__ uint32_t div_bpp(uint32_t j, int bpp) { return bpp == 1 ? j : bpp == 4 ? j >> 2 : (j * 0xAAABu) >> 17; }

// src_end16: the 16-byte boundary at or behind the image's last byte.  f in 2..16; grid = segs * bands.
__global__ __launch_bounds__(RES_THREADS) void k_box_filter(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int bpp, int f,
                                                            int w2, int h2, uint32_t segs, uint32_t magic, uintptr_t src_end16) {
    __shared__ __attribute__((aligned(16))) uint16_t cs[RES_SPAN];
    const uint32_t tid = threadIdx.x;
    const uint32_t seg = blockIdx.x % segs, band = blockIdx.x / segs;
    const uint32_t row2 = (uint32_t)w2 * (uint32_t)bpp;
    const size_t row = (size_t)w * bpp;
    const uint32_t b0 = seg * RES_BYTES;                                       // first byte of the tile in its output row
    const uint32_t nb = row2 - b0 < (uint32_t)RES_BYTES ? row2 - b0 : (uint32_t)RES_BYTES;
    const uint32_t px0 = b0 / (uint32_t)bpp, ch0 = b0 - px0 * (uint32_t)bpp;
    const uint32_t px1 = (b0 + nb - 1) / (uint32_t)bpp;
    const uint32_t fb = (uint32_t)f * (uint32_t)bpp;
    const uint32_t len = (px1 - px0 + 1) * fb;                                 // bytes of the segment, <= RES_SPAN
    const uint32_t nwords = (len + 15) >> 4;
    const size_t e0 = (size_t)px0 * fb;                                        // the segment's first byte in its source row
    const uint32_t y0 = band * RES_ROWS;
    const uint32_t rows = (uint32_t)h2 - y0 < (uint32_t)RES_ROWS ? (uint32_t)h2 - y0 : (uint32_t)RES_ROWS;
    const uint32_t fit = (uint32_t)RES_SPAN / (nwords * 16);                   // >= 1
    const uint32_t per_pass = fit < rows ? fit : rows;
    const uint32_t half = (uint32_t)(f * f) / 2;

    for (uint32_t r0 = 0; r0 < rows; r0 += per_pass) {
        const uint32_t rp = rows - r0 < per_pass ? rows - r0 : per_pass;
        for (uint32_t i = tid; i < rp * nwords; i += RES_THREADS) {
            const uint32_t r = i / nwords, k = i - r * nwords;
            const uint8_t* a = src + ((size_t)(y0 + r0 + r) * f * row + e0 + (size_t)k * 16);          // a byte of the image
            uint32_t e0s = 0, e1s = 0, e2s = 0, e3s = 0, o0s = 0, o1s = 0, o2s = 0, o3s = 0;      // per dword: the sums of bytes 0 | 2 and of bytes 1 | 3
            for (int j = 0; j < f; ++j, a += row) {
                const uint32_t p = (uint32_t)(uintptr_t)a & 15u;
                const uint4* wp = reinterpret_cast<const uint4*>(a - p);
                const uint4 A = wp[0];
                uint4 B = make_uint4(0, 0, 0, 0);
                if (p != 0 && (uintptr_t)(wp + 1) < src_end16) B = wp[1];
                // the 32 bytes shifted right by 8 bytes, then by 4, then by p & 3
                const bool s8 = (p & 8u) != 0, s4 = (p & 4u) != 0;
                const uint32_t t0 = s8 ? A.z : A.x, t1 = s8 ? A.w : A.y, t2 = s8 ? B.x : A.z, t3 = s8 ? B.y : A.w, t4 = s8 ? B.z : B.x, t5 = s8 ? B.w : B.y;
                const uint32_t u0 = s4 ? t1 : t0, u1 = s4 ? t2 : t1, u2 = s4 ? t3 : t2, u3 = s4 ? t4 : t3, u4 = s4 ? t5 : t4;
                const uint32_t sh = (p & 3u) * 8u;
                const uint32_t v0 = __funnelshift_r(u0, u1, sh), v1 = __funnelshift_r(u1, u2, sh), v2 = __funnelshift_r(u2, u3, sh), v3 = __funnelshift_r(u3, u4, sh);
                e0s += v0 & 0x00ff00ffu; o0s += (v0 >> 8) & 0x00ff00ffu;
                e1s += v1 & 0x00ff00ffu; o1s += (v1 >> 8) & 0x00ff00ffu;
                e2s += v2 & 0x00ff00ffu; o2s += (v2 >> 8) & 0x00ff00ffu;
                e3s += v3 & 0x00ff00ffu; o3s += (v3 >> 8) & 0x00ff00ffu;
            }
            uint4* out = reinterpret_cast<uint4*>(cs + ((size_t)r * nwords + k) * 16);
            out[0] = make_uint4((e0s & 0xffffu) | (o0s << 16), (e0s >> 16) | (o0s & 0xffff0000u), (e1s & 0xffffu) | (o1s << 16), (e1s >> 16) | (o1s & 0xffff0000u));
            out[1] = make_uint4((e2s & 0xffffu) | (o2s << 16), (e2s >> 16) | (o2s & 0xffff0000u), (e3s & 0xffffu) | (o3s << 16), (e3s >> 16) | (o3s & 0xffff0000u));
        }
        __syncthreads();
        for (uint32_t r = 0; r < rp; ++r) {
            uint8_t* D = dst + (size_t)(y0 + r0 + r) * row2 + b0;
            const int ph = (int)((uintptr_t)D & 3u);
            const uint16_t* c = cs + (size_t)r * nwords * 16;
            // thread 0 comes round a second time for the bytes behind the last complete dword of a full tile row
            for (int o0 = (int)tid * 4 - ph; o0 < (int)nb; o0 += RES_BYTES) {
                uint32_t v = 0;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int o = o0 + m;
                    const uint32_t jj = ch0 + (uint32_t)((o >= 0 && o < (int)nb) ? o : 0);
                    const uint32_t px = div_bpp(jj, bpp);
                    const uint16_t* q = c + px * fb + (jj - px * (uint32_t)bpp);
                    uint32_t sum = 0;
                    for (int i = 0; i < f; ++i) sum += q[i * bpp];
                    v |= box_round(sum, half, magic) << (8 * m);
                }
                if (o0 >= 0 && o0 + 4 <= (int)nb) *reinterpret_cast<uint32_t*>(D + o0) = v;
                else {
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (o0 + m >= 0 && o0 + m < (int)nb) D[o0 + m] = (uint8_t)(v >> (8 * m));
                }
            }
        }
        __syncthreads();
    }
}

// table[slot] = t, in stream order: flushes queued earlier still see the old entry, later ones the new
__global__ void k_set_texture(DevTexture* table, int slot, DevTexture t) { table[slot] = t; }

}  // namespace

namespace trgl {

hipError_t launch_set_texture(hipStream_t s, DevTexture* table, int slot, const DevTexture& t) {
    hipLaunchKernelGGL(k_set_texture, dim3(1), dim3(1), 0, s, table, slot, t);
    return hipGetLastError();
}

hipError_t launch_box_filter(hipStream_t s, const uint8_t* src, int w, int h, int bpp, int f, uint8_t* dst) {
    const size_t nsrc = (size_t)w * h * bpp;
    if (f == 1) return hipMemcpyAsync(dst, src, nsrc, hipMemcpyDeviceToDevice, s);
    const int w2 = w / f, h2 = h / f;
    const uint32_t segs = (uint32_t)(((uint64_t)w2 * bpp + RES_BYTES - 1) / RES_BYTES);
    const uint32_t bands = (uint32_t)((h2 + RES_ROWS - 1) / RES_ROWS);
    const uintptr_t src_end16 = ((uintptr_t)src + nsrc + 15) & ~(uintptr_t)15;
    hipLaunchKernelGGL(k_box_filter, dim3(segs * bands), dim3(RES_THREADS), 0, s, src, dst, w, bpp, f, w2, h2, segs, box_magic(f), src_end16);
    return hipGetLastError();
}

}  // namespace trgl
