// kernels_bin.hip — per-triangle setup and the order-preserving binning prepass (gfx950).
//
//   setup      : our_gl.cpp:89-141 for every triangle -> TriRec + number of tiles overlapped
//   scan       : exclusive scan (counts -> pair offsets; radix histograms -> scatter bases)
//   expand     : (tile id, triangle id) pairs in triangle order
//   radix pass : stable LSD counting sort of the pairs by tile id, so every tile's slice lists its
//                triangles in SUBMISSION ORDER (z ties keep the earlier triangle, our_gl.cpp:165;
//                fragments_drawn / z-range are order dependent, our_gl.cpp:194-198); the last pass also
//                leaves the per-tile [start,end) of the sorted pair list
//
// All integer / fp64 IEEE work; built with -ffp-contract=off so no product is fused into a sum.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "trgl_device.h"
#include "launch.h"
#include "device_util.h"

namespace {

__device__ __forceinline__ double dmin3(double a, double b, double c) { double m = a; if (b < m) m = b; if (c < m) m = c; return m; }
__device__ __forceinline__ double dmax3(double a, double b, double c) { double m = a; if (m < b) m = b; if (m < c) m = c; return m; }
using trgl_dev::dot4; using trgl_dev::wave_incl_scan; using trgl_dev::block_excl_scan;

__device__ __forceinline__ int wave_min_i(int v) {
    for (int o = 32; o; o >>= 1) { int t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int o = 32; o; o >>= 1) { int t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// blocks of tile (tx, ty) inside the block-unit box [qx0, qx1] x [qy0, qy1] (the box reaches the tile)
__device__ __forceinline__ uint32_t tile_block_mask(uint32_t tx, uint32_t ty, uint32_t qx0, uint32_t qy0, uint32_t qx1, uint32_t qy1) {
    const uint32_t c0 = qx0 > 4 * tx ? qx0 - 4 * tx : 0u, c1 = qx1 < 4 * tx + 3 ? qx1 - 4 * tx : 3u;
    const uint32_t r0 = qy0 > 4 * ty ? qy0 - 4 * ty : 0u, r1 = qy1 < 4 * ty + 3 ? qy1 - 4 * ty : 3u;
    return (((2u << c1) - (1u << c0)) & 0xfu) * 0x1111u & ((0xffffu >> (12 - 4 * r1)) & (0xffffu << (4 * r0)));
}
// The pairs of a block of 256 triangles, the one statement of their rules for k_expand and for k_setup's direct path.  Thread `tid` holds
// triangle i of the flush: c tiles, the box `tb` k_setup left in `tilebox`, and o = the pairs of the block's earlier triangles.
// put(j, tile id, triangle word, mask) receives pair j of the block: a triangle's tiles in row-major order over the tile rows this
// context owns, the triangle word = index | zq << 25 (TRGL_VAL_TRI | TRGL_VAL_ZQ).  Triangles with more than 8 tiles are written
// by the whole wave.  No barrier inside.
template <class Put>
__device__ __forceinline__ void block_pairs(const FrameParams& fp, int tiles_x, uint32_t i, uint32_t c, uint2 tb, uint32_t o, Put put) {
    constexpr uint32_t SMALL = 8;
    if (c && c <= SMALL) {
        // row-major walk with running counters instead of a division and a modulo per pair
        const uint32_t qx0 = tb.x & 0x1fff, qy0 = (tb.x >> 16) & 0x1fff, qx1 = tb.y & 0x1fff, qy1 = (tb.y >> 16) & 0x1fff;
        const uint32_t iz = i | ((((tb.x >> 13) & 7u) | (((tb.y >> 13) & 7u) << 3) | ((tb.y >> 29) << 6)) << 25);      // TRGL_VAL_TRI | TRGL_VAL_ZQ
        const uint32_t tx0 = qx0 >> 2, ty0 = qy0 >> 2, tx1 = qx1 >> 2;
        uint32_t tx = tx0, row = 0;
        uint32_t ty = fp.il_tiles ? (uint32_t)il_nth_owned_from(fp, (int)ty0, 0) : ty0;
        for (uint32_t k = 0; k < c; ++k) {
            put(o + k, ty * tiles_x + tx, iz, tile_block_mask(tx, ty, qx0, qy0, qx1, qy1));
            if (++tx > tx1) { tx = tx0; ++row; ty = fp.il_tiles ? (uint32_t)il_nth_owned_from(fp, (int)ty0, (int)row) : ty0 + row; }
        }
    }
    unsigned long long big = __ballot(c > SMALL);
    const int lane = threadIdx.x & 63;
    while (big) {
        int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        uint32_t cc = __shfl(c, src), oo = __shfl(o, src), ii = __shfl(i, src);
        uint32_t bx = __shfl(tb.x, src), by = __shfl(tb.y, src);
        const uint32_t qx0 = bx & 0x1fff, qy0 = (bx >> 16) & 0x1fff, qx1 = by & 0x1fff, qy1 = (by >> 16) & 0x1fff;
        ii |= (((bx >> 13) & 7u) | (((by >> 13) & 7u) << 3) | ((by >> 29) << 6)) << 25;
        uint32_t tx0 = qx0 >> 2, ty0 = qy0 >> 2, tx1 = qx1 >> 2;
        uint32_t wdt = tx1 - tx0 + 1;
        for (uint32_t k = lane; k < cc; k += 64) {
            uint32_t ty = fp.il_tiles ? (uint32_t)il_nth_owned_from(fp, (int)ty0, (int)(k / wdt)) : ty0 + k / wdt, tx = tx0 + k % wdt;
            put(oo + k, ty * tiles_x + tx, ii, tile_block_mask(tx, ty, qx0, qy0, qx1, qy1));
        }
    }
}

// the direct path's segments: at most SEG_MAX pair slots per setup block (two words per pair fill k_setup's 32 KB of LDS), a multiple of 4;
// a block of the first radix pass owns at most SEG_MAX_GROUP consecutive segments
constexpr uint32_t SEG_MAX = 4096, SEG_MAX_GROUP = 16;

// ---------------------------------------------------------------------------------------------
// setup: one thread per triangle of one draw.  Follows our_gl.cpp:89-141 line by line.
// HBM traffic is staged through LDS so that both the 96-B/triangle clip stream and the 128-B/triangle
// record stream move as 16 B per lane, fully coalesced (a lane reading its own 96-B triangle straight
// from HBM touches 64 different lines per load instruction).
// ---------------------------------------------------------------------------------------------
constexpr int SETUP_THREADS = 256;

__global__ __launch_bounds__(SETUP_THREADS) void k_setup(FrameParams fp, DrawDesc d, DrawDesc* __restrict__ draws_out, int draw_idx,
                                                         TriRec* __restrict__ recs, TriW* __restrict__ recs_w, uint32_t* __restrict__ cnt,
                                                         uint2* __restrict__ tilebox, DevStats* __restrict__ stats,
                                                         uint32_t* __restrict__ blk_sums, uint32_t blk_base,
                                                         uint32_t* __restrict__ seg_k, uint32_t* __restrict__ seg_v, uint32_t seg_S) {
    __shared__ __attribute__((aligned(16))) double s_buf[SETUP_THREADS * 16];    // 32 KB: in [256][12], then out [256][16], then the block's pairs
    // The draw's descriptor arrives as a kernel argument (scalar loads from the argument segment; no copy command on the stream before
    // the flush's first kernel) and is left in device memory for the kernels behind this one, which read uniforms and arrays through it.
    if (blockIdx.x == 0 && threadIdx.x == 0) draws_out[draw_idx] = d;
    const uint32_t b0 = blockIdx.x * SETUP_THREADS;
    const uint32_t nb = min((uint32_t)SETUP_THREADS, d.n - b0);
    const uint32_t tid = threadIdx.x;
    const uint32_t i = b0 + tid;
    const bool in_range = tid < nb;

    // ---- clip stream in: nb*96 contiguous bytes ------------------------------------------------
    const double* src = d.clip + (size_t)b0 * 12;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const double2* s2 = reinterpret_cast<const double2*>(src);
        double2* l2 = reinterpret_cast<double2*>(s_buf);
        typedef double f64x2 __attribute__((ext_vector_type(2)));
        for (uint32_t k = tid; k < nb * 6; k += SETUP_THREADS)
            *reinterpret_cast<f64x2*>(&l2[k]) = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(&s2[k]));
    } else {
        for (uint32_t k = tid; k < nb * 12; k += SETUP_THREADS) s_buf[k] = src[k];
    }
    __syncthreads();
    double v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = in_range ? s_buf[tid * 12 + k] : 0.0;
    __syncthreads();

    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;   // contribution to bbox stats
    uint32_t ntiles = 0;
    bool large = false;
    uint2 tb = make_uint2(0, 0);
    TriRec r;
    {
        uint4* z4 = reinterpret_cast<uint4*>(&r);
#pragma unroll
        for (int k = 0; k < 8; ++k) z4[k] = make_uint4(0, 0, 0, 0);
    }
    if (in_range) {
        bool ok = !(v[3] <= 1e-12 || v[7] <= 1e-12 || v[11] <= 1e-12);                     // :94 (:97 is dead)
        double ndc[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ndc[4 * q + k] = v[4 * q + k] / v[4 * q + 3];      // :101
            // w / w is exactly 1.0 for every finite non-zero w and NaN for an infinite one
            ndc[4 * q + 3] = __builtin_isfinite(v[4 * q + 3]) ? 1.0 : __builtin_nan("");
        }
        bool zo0 = (ndc[2] < -1.0 || ndc[2] > 1.0), zo1 = (ndc[6] < -1.0 || ndc[6] > 1.0),
             zo2 = (ndc[10] < -1.0 || ndc[10] > 1.0);
        ok = ok && !(zo0 && zo1 && zo2);                                                   // :103-106
#pragma unroll
        for (int k = 0; k < 12; ++k) ok = ok && __builtin_isfinite(ndc[k]);                // :109-114
        double sx[3], sy[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { const double* v = ndc + 4 * q; sx[q] = dot4(fp.vp, v[0], v[1], v[2], v[3]); sy[q] = dot4(fp.vp + 4, v[0], v[1], v[2], v[3]); }  // :117-121
        double e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
        double cross_product = e1x * e2y - e1y * e2x;                                      // :124-126
        ok = ok && !(cross_product <= 0);                                                  // :127
        int min_x_px = max(0, x86_cvttsd2si(floor(dmin3(sx[0], sx[1], sx[2]))));           // :130-133
        int max_x_px = min(fp.W - 1, x86_cvttsd2si(ceil(dmax3(sx[0], sx[1], sx[2]))));
        int min_y_px = max(0, x86_cvttsd2si(floor(dmin3(sy[0], sy[1], sy[2]))));
        int max_y_px = min(fp.H - 1, x86_cvttsd2si(ceil(dmax3(sy[0], sy[1], sy[2]))));
        ok = ok && !(min_x_px > max_x_px || min_y_px > max_y_px);                          // :135
        if (ok) {
            bx0 = min_x_px; by0 = min_y_px; bx1 = max_x_px; by1 = max_y_px;                // :138-141
            r.ax = sx[0]; r.ay = sy[0];
            r.s0x = sx[2] - sx[0]; r.s0y = sx[1] - sx[0];                                  // :78
            r.s1x = sy[2] - sy[0]; r.s1y = sy[1] - sy[0];                                  // :79
            r.uz = r.s0x * r.s1y - r.s0y * r.s1x;                                          // :80 (cross().z)
            // "Well scaled": every screen coordinate below 2^200 in magnitude, every edge delta zero or at
            // least 2^-250, u.z negative (it is -cross_product) and not tiny.  Then no product, sum or
            // quotient of the pixel loop can overflow, underflow or be NaN, which is what the division-free
            // coverage test and the FMA division by u.z in k_raster rely on ("exactness").
            {
                const double BIG = 0x1p200, SMALL = 0x1p-250;
                bool ws = r.uz < 0.0 && !(fabs(r.uz) < 1e-12);
#pragma unroll
                for (int q = 0; q < 3; ++q) ws = ws && fabs(sx[q]) < BIG && fabs(sy[q]) < BIG;
                const double dl[4] = { r.s0x, r.s0y, r.s1x, r.s1y };
#pragma unroll
                for (int q = 0; q < 4; ++q) ws = ws && (dl[q] == 0.0 || fabs(dl[q]) >= SMALL);
                // ... and not a sliver whose coverage roundings could reach past its bounding box.  k_raster's fast visit does not test
                // a pixel against the bbox of :130-133: with every computed u within E = 2^-50 S R of its exact value (S = sum of the
                // |edge deltas|, R >= |A - pixel centre| (L1) on the blocks the bbox touches) and u.z within 2^-52 S^2, a pixel that
                // passes the sign test has exact barycentrics >= -eps, eps < 2^-48 S R / |u.z|, so it lies within 2 eps S of the
                // triangle's extent in x and in y - while a pixel centre outside floor(min) .. ceil(max) is at least 0.5 away from it.
                // 2^-40 S^2 R < |u.z| (R >= S) makes 2 eps S < 2^-7.  The others take the literal path, which tests the bbox.
                {
                    const double S = (fabs(r.s0x) + fabs(r.s0y)) + (fabs(r.s1x) + fabs(r.s1y));
                    const double rx = fmax(fabs(r.ax - ((double)bx0 + 0.5)), fabs(r.ax - ((double)bx1 + 0.5)));
                    const double ry = fmax(fabs(r.ay - ((double)by0 + 0.5)), fabs(r.ay - ((double)by1 + 0.5)));
                    ws = ws && 0x1p-40 * (S * S) * (rx + ry + 17.0 + S) < fabs(r.uz);
                }
                r.ruz = ws ? 1.0 / r.uz : 0.0;
            }
            r.z0 = ndc[2]; r.z1 = ndc[6]; r.z2 = ndc[10];
            r.bx0 = (uint16_t)bx0; r.by0 = (uint16_t)by0; r.bx1 = (uint16_t)bx1; r.by1 = (uint16_t)by1;
            r.color = d.colors ? d.colors[i] : 0xffffffffu;
            r.dl = ((uint32_t)draw_idx << 24) | i | (r.ruz == 0.0 ? TRGL_DL_LITERAL : 0u);
            // Depth plane of the early depth test (k_raster).  The z of our_gl.cpp:156-158 is the plane
            //   z0 + ((ax - x) Gx + (ay - y) Gy) / u.z,  Gx = s1x (z1-z0) - s1y (z2-z0),  Gy = s0y (z2-z0) - s0x (z1-z0)
            // through the three vertices up to the roundings of u.x, u.y, the three quotients and the weighted sum: at most
            // 2^-50 max|z_i| (R S / |u.z| + 1) for a covered pixel, where R >= |A - pixel centre| (L1) over the clamped bbox (and R >= S)
            // and S = the sum of the |edge deltas|.  g1 = Gx/u.z and g2 = Gy/u.z carry a few more roundings of that size, so does the
            // evaluation c0 + (ax - x) g1 + (ay - y) g2 itself, and c0 = z0 - 2^-39 max|z_i| (R S / |u.z| + 1) covers all of it a
            // thousand times over: a pixel whose plane value is >= the stored depth fails the strict `<` of :165 whatever its
            // coverage and low bits.  Switched off (c0 = -inf, g = 0) for triangles that are not well scaled and when a constant
            // could leave the normal range.
            r.c0 = -__builtin_inf(); r.g1 = 0.0; r.g2 = 0.0;
            if (r.ruz != 0.0) {
                const double zabs = dmax3(fabs(r.z0), fabs(r.z1), fabs(r.z2));
                const double dz1 = r.z1 - r.z0, dz2 = r.z2 - r.z0;
                const double h1 = (r.s1x * dz1 - r.s1y * dz2) * r.ruz, h2 = (r.s0y * dz2 - r.s0x * dz1) * r.ruz;
                const double rx = fmax(fabs(r.ax - ((double)bx0 + 0.5)), fabs(r.ax - ((double)bx1 + 0.5)));
                const double ry = fmax(fabs(r.ay - ((double)by0 + 0.5)), fabs(r.ay - ((double)by1 + 0.5)));
                const double Ssum = (fabs(r.s0x) + fabs(r.s0y)) + (fabs(r.s1x) + fabs(r.s1y));
                const double R = rx + ry + 1.0 + Ssum;       // (+ S: the plane is also evaluated at the three vertices, k_raster's cull)
                const double mz = zabs * 0x1p-39 * (R * Ssum * fabs(r.ruz) + 1.0) + 0x1p-600;
                // trusted only while nothing can overflow (R |g| bounds each product of the test); NaN compares false
                const bool okp = zabs < 0x1p1000 && R * fabs(h1) < 0x1p900 && R * fabs(h2) < 0x1p900 && mz < 0x1p1000;
                if (okp) { r.c0 = r.z0 - mz; r.g1 = h1; r.g2 = h2; }
            }
            if (d.kind != TRGL_SHADER_FLAT) {                                                  // :168-170
                TriW w;
                w.iw0 = (fabs(v[3]) > 1e-12) ? (1.0 / v[3]) : 0.0;
                w.iw1 = (fabs(v[7]) > 1e-12) ? (1.0 / v[7]) : 0.0;
                w.iw2 = (fabs(v[11]) > 1e-12) ? (1.0 / v[11]) : 0.0;
                w.pad = 0.0;
                recs_w[d.first + i] = w;
            }
            // barycentric() rejects every pixel when |u.z| < 1e-12 (our_gl.cpp:82-83): no pairs then.
            // Rows outside this context's strip are not ours either.
            int y_lo = max(by0, fp.strip_y0), y_hi = min(by1, fp.strip_y1 - 1);
            if (!(fabs(r.uz) < 1e-12) && y_lo <= y_hi) {
                uint32_t tx0 = bx0 >> TRGL_TILE_LOG2, tx1 = bx1 >> TRGL_TILE_LOG2;
                uint32_t ty0 = y_lo >> TRGL_TILE_LOG2, ty1 = y_hi >> TRGL_TILE_LOG2;
                // tile rows of the box that this context owns: all of them for a strip (the box is clipped to it), the ones of
                // its bands with interleaved ownership (k_expand walks the same rows)
                const uint32_t rows = fp.il_tiles ? (uint32_t)(il_owned_below(fp, (int)ty1 + 1) - il_owned_below(fp, (int)ty0)) : ty1 - ty0 + 1;
                ntiles = (tx1 - tx0 + 1) * rows;
                // the box in BLOCK units (8 x 8 pixels; tile = block >> 2): k_expand derives from it, for every tile of the box,
                // the 4 x 4 mask of the tile's blocks that the box reaches
                tb = make_uint2(((uint32_t)bx0 >> TRGL_BLOCK_LOG2) | (((uint32_t)y_lo >> TRGL_BLOCK_LOG2) << 16),
                                ((uint32_t)bx1 >> TRGL_BLOCK_LOG2) | (((uint32_t)y_hi >> TRGL_BLOCK_LOG2) << 16));
                // A 7-bit lower bound of the triangle's depths rides with every pair (in the spare bits of its triangle word, k_expand):
                // every covered pixel has z above the depth plane's smallest value at the three vertices (k_raster's cull explains
                // why), zv, hence z >= -1 + zq / 64 for zq = floor((zv + 1) 64 - 2^-20).  In the spare bits of the box: block
                // coordinates stay below 2^13.  A flush that holds large triangles (`large`) makes k_raster's list steps use it: an
                // entry whose bound is not below the block's largest depth never becomes a candidate - no gather, no test.
                uint32_t zq = 0;
                if (r.c0 > -__builtin_inf()) {
                    const double zv = dmin3(r.c0, __builtin_fma(-r.s0y, r.g1, __builtin_fma(-r.s1y, r.g2, r.c0)),
                                            __builtin_fma(-r.s0x, r.g1, __builtin_fma(-r.s1x, r.g2, r.c0)));
                    const double t = (zv + 1.0) * 64.0 - 0x1p-20;
                    if (t >= 1.0) zq = t >= 127.0 ? 127u : (uint32_t)x86_cvttsd2si(floor(t));
                }
                tb.x |= (zq & 7u) << 13; tb.y |= ((zq >> 3) & 7u) << 13; tb.y |= (zq >> 6) << 29;
                large = ntiles != 0 && (bx1 - bx0 >= 64 || y_hi - y_lo >= 64);      // (no tile in this context's bands: no pair to profit)
            }
        }
        cnt[d.first + i] = ntiles;
        tilebox[d.first + i] = tb;
    }
    // ---- record stream out: each wave stages its own 64 records (8 KB) in LDS, 16-B chunks XOR-swizzled so neither the
    // per-thread writes (128-B stride) nor the linear read-out conflict on banks, and writes them as one contiguous run.
    // A record is only ever read through a (tile, triangle) pair: triangles without pairs (rejected, or outside this
    // context's strip - 7 of 8 on an 8-GPU shard) need no 128-B store; which ones is a wave ballot, so the phase needs no
    // block barrier and no LDS beyond the 32 KB staging buffer (5 blocks per CU instead of 4).
    const uint32_t lane = tid & 63, wbase = tid & ~63u;
    {
        uint4* l4 = reinterpret_cast<uint4*>(s_buf);
        const uint4* r4 = reinterpret_cast<const uint4*>(&r);
#pragma unroll
        for (int c = 0; c < 8; ++c) l4[tid * 8 + (c ^ (tid & 7))] = r4[c];
        const unsigned long long keep = __ballot(ntiles != 0);
        __builtin_amdgcn_wave_barrier();
        uint4* dst = reinterpret_cast<uint4*>(recs + d.first + b0 + wbase);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const uint32_t k = lane + 64u * it, t = k >> 3, c = k & 7;            // chunk c of the wave's record t
            if ((keep >> t) & 1ull) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(&l4[(wbase + t) * 8 + (c ^ (t & 7))]), reinterpret_cast<u32x4*>(&dst[k]));
            }
        }
    }
    // triangles with pairs that take the literal (dividing) path of k_raster: none in any realistic frame, and then the host
    // launches the raster kernel that does not contain that path (trgl_flush_end)
    {
        const unsigned long long lit = __ballot(ntiles != 0 && r.ruz == 0.0);
        if (lit && lane == 0) atomicAdd(&stats->literal_tris, (unsigned long long)__popcll(lit));
        const unsigned long long lrg = __ballot(large);
        if (lrg && lane == 0) atomicAdd(&stats->large_tris, (unsigned long long)__popcll(lrg));
    }
    // bbox stats (our_gl.cpp:138-141): one set of atomics per wave
    int wx0 = wave_min_i(bx0), wy0 = wave_min_i(by0), wx1 = wave_max_i(bx1), wy1 = wave_max_i(by1);
    // All waves hit the same four words, and same-address atomics serialise at ~11 ns each, so only
    // issue one when it would change the value.  The plain loads may be stale, but min only falls and
    // max only rises: a stale value can cause a redundant atomic, never a missed one.
    if ((threadIdx.x & 63) == 0 && wx0 != INT_MAX) {
        if (wx0 < __builtin_nontemporal_load(&stats->min_x)) atomicMin(&stats->min_x, wx0);
        if (wy0 < __builtin_nontemporal_load(&stats->min_y)) atomicMin(&stats->min_y, wy0);
        if (wx1 > __builtin_nontemporal_load(&stats->max_x)) atomicMax(&stats->max_x, wx1);
        if (wy1 > __builtin_nontemporal_load(&stats->max_y)) atomicMax(&stats->max_y, wy1);
    }
    // pairs of this block of 256 triangles: the offset of every triangle's pairs inside the block's run, and the run's length.
    // k_expand derives every triangle's slice of the pair list from these sums (k_chunk_spine) and a block-level scan of `cnt`,
    // so no scan pass ever walks the N-element arrays.
    uint32_t tot;
    const uint32_t off = block_excl_scan(ntiles, reinterpret_cast<uint32_t*>(s_buf), &tot);      // (its first barrier: every wave is done with the staging buffer)
    if (tid == 0) blk_sums[blk_base + blockIdx.x] = tot;
    // The direct path (seg_S != 0): the block leaves its pairs itself, in submission order, in its own segment of seg_S slots -
    // no offset from any other block is needed.  They are assembled in the staging buffer (sort words in its first half, triangle
    // words in its second: SEG_MAX slots each) and go out linearly, 16 bytes per lane.  A block with more pairs than the segment
    // holds writes none: k_chunk_spine sees its sum and flags the flush, which then takes k_expand.
    if (seg_S && tot && tot <= seg_S) {                      // block-uniform
        __syncthreads();                                     // the scan's wave totals have been read
        uint32_t* const s_k = reinterpret_cast<uint32_t*>(s_buf);
        uint32_t* const s_v = s_k + SEG_MAX;
        block_pairs(fp, fp.tiles_x, d.first + i, ntiles, tb, off, [&](uint32_t j, uint32_t key, uint32_t iz, uint32_t m) { s_k[j] = key | (m << 16); s_v[j] = iz; });
        __syncthreads();
        uint4* const kq = reinterpret_cast<uint4*>(seg_k + (size_t)(blk_base + blockIdx.x) * seg_S);
        uint4* const vq = reinterpret_cast<uint4*>(seg_v + (size_t)(blk_base + blockIdx.x) * seg_S);
        // (seg_S is a multiple of 4: the last 16-byte group stays inside the segment; its words past `tot` are never read)
        for (uint32_t q = tid; 4 * q < tot; q += SETUP_THREADS) {
            kq[q] = *reinterpret_cast<const uint4*>(s_k + 4 * q);
            vq[q] = *reinterpret_cast<const uint4*>(s_v + 4 * q);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// pair offsets.  k_setup leaves one pair count per block of 256 triangles (blk_sums, blocks numbered across the
// draws of the flush).  k_chunk_spine (one block) scans them in chunks of 16: chunk_off[c] = pairs before block 16c.
// k_expand then finds its block's base (chunk offset + the <= 15 preceding block sums of its chunk) and scans the 256
// counts of its own triangles in LDS.
// ---------------------------------------------------------------------------------------------
constexpr int EXPAND_CHUNK = 16;

constexpr int SPINE_THREADS = 1024;
__global__ __launch_bounds__(SPINE_THREADS) void k_chunk_spine(const uint32_t* __restrict__ blk_sums, uint32_t nblk,
                                                               uint32_t* __restrict__ chunk_off,
                                                               unsigned long long* __restrict__ total64, unsigned long long* __restrict__ host_copy,
                                                               uint4* __restrict__ bounds16, uint32_t n_half16,
                                                               uint32_t seg_S, uint32_t seg_G, uint32_t seg_chunk,
                                                               uint32_t* __restrict__ seg_flag, uint32_t* __restrict__ seg_flag_host) {
    __shared__ unsigned long long s_wave[SPINE_THREADS / 64];
    // Do the flush's counts fit the direct path's segments (k_setup) and groups (the first radix pass)?  seg_flag = 1 when a setup block
    // has more than seg_S pairs or seg_G consecutive blocks have more than seg_chunk (or seg_S is 0: no sizes to fit).  The kernels of
    // the direct path do nothing then, and the host queues k_expand and the dense passes (trgl_flush_end).  Evaluated for every
    // flush, also one that takes k_expand anyway: the host returns to the direct path once a flush fits.
    // (the blocks against seg_S, and groups of 16 - which are the chunks - against seg_chunk, in the scan loop below; groups of another
    // size here: one group per thread, its up to 16 loads issued together)
    int seg_bad = seg_S == 0;
    if (seg_S && seg_G != EXPAND_CHUNK) {
        for (uint32_t g = threadIdx.x; (uint64_t)g * seg_G < nblk; g += SPINE_THREADS) {
            uint32_t t[EXPAND_CHUNK];
#pragma unroll
            for (uint32_t k = 0; k < EXPAND_CHUNK; ++k) { const uint32_t q = g * seg_G + k; t[k] = (k < seg_G && q < nblk) ? blk_sums[q] : 0u; }
            unsigned long long sum = 0;
#pragma unroll
            for (uint32_t k = 0; k < EXPAND_CHUNK; ++k) sum += t[k];
            seg_bad |= sum > seg_chunk;
        }
    }
    const uint32_t blk_max = seg_S ? seg_S : ~0u;
    const unsigned long long grp_max = (seg_S && seg_G == EXPAND_CHUNK) ? seg_chunk : ~0ull;
    // (the tile bounds of the flush start empty, tile_start at ~0 and tile_end at 0 - the last radix pass narrows them with atomics:
    // set here instead of by fill commands of their own on the stream, 4.6 us each)
    for (uint32_t k = threadIdx.x; k < 2 * n_half16; k += SPINE_THREADS) bounds16[k] = k < n_half16 ? make_uint4(~0u, ~0u, ~0u, ~0u) : make_uint4(0, 0, 0, 0);
    const uint32_t nchunks = (nblk + EXPAND_CHUNK - 1) / EXPAND_CHUNK;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // One chunk (16 block sums = 64 bytes) per thread, 1024 chunks per round.  Offsets are 32-bit by design (a flush holds
    // fewer than 2^32 pairs); everything is accumulated in 64 bits so that a flush beyond that limit is seen as such by the
    // host and by the guards of the kernels queued behind this one instead of wrapping (100 k full-screen triangles at
    // 8192^2 are 6.5e9 pairs).
    unsigned long long running = 0;
    for (uint32_t start = 0; start < nchunks; start += SPINE_THREADS) {
        const uint32_t c = start + threadIdx.x;
        unsigned long long v = 0;
        if (c < nchunks) {
            const uint32_t q0 = c * EXPAND_CHUNK;
            if (q0 + EXPAND_CHUNK <= nblk) {
                const uint4* p4 = reinterpret_cast<const uint4*>(blk_sums + q0);
#pragma unroll
                for (int k = 0; k < EXPAND_CHUNK / 4; ++k) {
                    const uint4 t = p4[k]; v += (unsigned long long)t.x + t.y + t.z + t.w;
                    seg_bad |= max(max(t.x, t.y), max(t.z, t.w)) > blk_max;
                }
            } else {
                for (uint32_t q = q0; q < nblk; ++q) { const uint32_t t = blk_sums[q]; v += t; seg_bad |= t > blk_max; }
            }
            seg_bad |= v > grp_max;
        }
        unsigned long long inc = v;                                   // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) s_wave[w] = inc;
        __syncthreads();
        unsigned long long base = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < SPINE_THREADS / 64; ++k) { const unsigned long long t = s_wave[k]; if (k < w) base += t; tot += t; }
        if (c < nchunks) chunk_off[c] = (uint32_t)(running + base + inc - v);
        running += tot;
        __syncthreads();
    }
    seg_bad = __syncthreads_or(seg_bad);
    if (threadIdx.x == 0) {
        *total64 = running;
        // The host needs the pair count and the two triangle counts that k_setup left behind it (DevStats: literal_tris, large_tris at
        // total64[1] and [2], pinned by the static_asserts under DevStats in trgl_device.h)
        // before it launches the raster: written straight into its pinned memory instead of a copy command on the stream (4.6 us).
        *seg_flag = (uint32_t)seg_bad; *seg_flag_host = (uint32_t)seg_bad;
        host_copy[0] = running; host_copy[1] = total64[1]; host_copy[2] = total64[2];
        __threadfence_system();
    }
}

// expand: triangle i owns pairs [off, off + cnt[i]) = its tiles in row-major order; off is computed here.
// Triangles with many tiles are written by the whole wave.  One launch per draw (same blocks as k_setup).
// The pairs of a block are consecutive in the output (the offsets are a prefix sum in submission order), so they are
// assembled in LDS and written out linearly, 16 bytes per lane: pair j of the block sits at LDS slot (base & 3) + j, so a
// group of four LDS slots is a 16-byte-aligned group of four pairs in memory.  A block whose triangles cover more than
// EXPAND_STAGE tiles writes straight to memory.
// Every pair also carries the 4 x 4 mask of the tile's 8 x 8-pixel blocks that the triangle's clamped bbox reaches (bit 4 cy + cx):
// the raster wave that owns a block picks its candidates from the tile's list by that bit, without touching their records.
// The sort word of a pair: while the frame has at most 65536 tiles (up to 8192x8192) the tile id in its low 16 bits and the mask in
// its high 16 (one 4-byte stream for both); beyond that (WIDE) the 32-bit tile id, and the mask in a 16-bit stream of its own.
constexpr uint32_t EXPAND_STAGE = 3072;
template <bool WIDE>
__global__ __launch_bounds__(256) void k_expand(FrameParams fp, uint32_t first, uint32_t n, int tiles_x, const uint32_t* __restrict__ cnt,
                                                const uint32_t* __restrict__ blk_sums, const uint32_t* __restrict__ chunk_off,
                                                uint32_t blk_base, const uint2* __restrict__ tilebox,
                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint16_t* __restrict__ bmask,
                                                const unsigned long long* __restrict__ pairs_total, uint32_t cap) {
    __shared__ uint32_t smem[4];
    __shared__ __attribute__((aligned(16))) uint32_t s_k[EXPAND_STAGE + 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_v[EXPAND_STAGE + 4];
    __shared__ __attribute__((aligned(16))) uint16_t s_m[WIDE ? EXPAND_STAGE + 4 : 4];
    if (*pairs_total > cap) return;        // the host sized the buffers from an earlier flush: it will grow them and launch again
    const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = first + local;                          // index of the triangle within the flush
    const uint32_t blk = blk_base + blockIdx.x;
    uint32_t c = 0; uint2 tb = make_uint2(0, 0);
    if (local < n) { c = cnt[i]; if (c) tb = tilebox[i]; }
    // pairs before this block = those before its chunk of 16 blocks (k_chunk_spine) + the sums of the blocks before it inside the chunk:
    // ONE load by up to 15 lanes and four butterfly steps (a loop of up to 15 dependent wave-uniform loads cost ~1 us each)
    uint32_t base;
    {
        const uint32_t q0 = blk - blk % EXPAND_CHUNK, l = threadIdx.x & 63u;
        uint32_t part = l < blk - q0 ? blk_sums[q0 + l] : 0u;
        for (int o = 8; o; o >>= 1) part += __shfl_xor(part, o);
        base = chunk_off[blk / EXPAND_CHUNK] + (uint32_t)__builtin_amdgcn_readfirstlane((int)part);
    }
    uint32_t tot;
    const uint32_t o = block_excl_scan(c, smem, &tot);         // offset inside the block's run of pairs
    const bool staged = tot <= EXPAND_STAGE;                   // block-uniform
    const uint32_t sh = base & 3u;
    uint32_t* const kdst = keys + base; uint32_t* const vdst = vals + base; uint16_t* const mdst = bmask + base;
    auto put = [&](uint32_t j, uint32_t key, uint32_t iz, uint32_t m) {
        const uint32_t word = WIDE ? key : key | (m << 16);
        if (staged) { s_k[sh + j] = word; s_v[sh + j] = iz; if (WIDE) s_m[sh + j] = (uint16_t)m; }
        else { kdst[j] = word; vdst[j] = iz; if (WIDE) mdst[j] = (uint16_t)m; }
    };
    block_pairs(fp, tiles_x, i, c, tb, o, put);
    if (staged) {
        __syncthreads();
        // LDS slots [sh, sh + tot) = pairs [base, base + tot); slot group q = the 16-byte-aligned pairs base - sh + 4q .. + 3.
        // Groups the run covers entirely go out as one 16-byte store per stream; the (at most two) partial ones pair by pair.
        uint32_t* const kq = keys + (base - sh); uint32_t* const vq = vals + (base - sh); uint16_t* const mq = bmask + (base - sh);
        const uint32_t end = sh + tot;
        for (uint32_t q = threadIdx.x; 4 * q < end; q += 256) {
            const uint32_t j0 = 4 * q;
            if (j0 >= sh && j0 + 4 <= end) {
                *reinterpret_cast<uint4*>(kq + j0) = *reinterpret_cast<const uint4*>(s_k + j0);
                *reinterpret_cast<uint4*>(vq + j0) = *reinterpret_cast<const uint4*>(s_v + j0);
                if (WIDE) *reinterpret_cast<uint2*>(mq + j0) = *reinterpret_cast<const uint2*>(s_m + j0);
            } else {
                for (uint32_t j = j0; j < j0 + 4; ++j)
                    if (j >= sh && j < end) { kq[j] = s_k[j]; vq[j] = s_v[j]; if (WIDE) mq[j] = s_m[j]; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// stable LSD radix pass on `bits` key bits at `shift`.  A block of RADIX_WAVES waves owns RADIX_CHUNK = RADIX_WAVES x 1024 consecutive
// pairs; wave w owns the w-th part and walks it in order, 64 pairs a step, ranking equal digits
// by their lane numbers, so equal keys keep their input order (= triangle submission order).  The chunk is
// then reordered by digit in LDS and written out linearly, so global stores are contiguous runs
// (RADIX_CHUNK / 2^bits pairs per digit on average) instead of 64 scattered 4-byte elements per
// instruction.  hist layout: [digit][chunk] so one exclusive scan yields every chunk's base per digit.
// The scatter's grid is what the device holds at once; a block walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ... (a static
// stride: no work counter, no block waits for another) with the loads of its next chunk in flight behind the current one.
// A pair is its sort word (k_expand) and its triangle word; WIDE frames also move the 16-bit mask stream.  The last pass writes
// what k_raster reads - triangle words and masks, no sort words - and the tile bounds (k_radix_scatter).
// ---------------------------------------------------------------------------------------------
// A block has RADIX_WAVES waves: 8 (8192 pairs, 75 KB of LDS, two blocks per CU) when the pair buffers hold at least
// RADIX_BIG_CAP pairs, else 4 (4096 pairs, four blocks per CU).  8 waves give runs of 64 pairs per digit at 7-bit digits; measured
// against 4 on the 4096^2 frame (18 M pairs): first pass 94 -> 85 us, last pass 107 -> 101 us, row scans 8 -> 5 us.  On the head frames
// (C2 / C3, a few hundred thousand pairs: under 100 blocks of 8192 for 256 CUs) 8 waves made the binning 4 us slower.
constexpr int RADIX_ROUNDS = 16;
constexpr int RADIX_WAVE_CHUNK = RADIX_ROUNDS * 64;      // 1024
constexpr uint32_t RADIX_BIG_CAP = 4u << 20;
constexpr int RADIX_MAX_BITS = 8;

__global__ __launch_bounds__(256) void k_radix_hist(const uint32_t* __restrict__ keys, const unsigned long long* __restrict__ pairs_total,
                                                    uint32_t cap, int shift, int bits, uint32_t chunk,
                                                    uint32_t nblocks, uint32_t* __restrict__ hist, const uint32_t* __restrict__ skip) {
    __shared__ uint32_t s_cnt[1 << RADIX_MAX_BITS];
    const unsigned long long P64 = *pairs_total;
    // over capacity: nothing was expanded; every block counts nothing.  skip: a later pass of the direct path, whose first pass did
    // nothing when the flush did not fit the segments (k_chunk_spine's flag) - its input is not this flush's
    const uint32_t P = (P64 > cap || (skip && *skip)) ? 0u : (uint32_t)P64;
    const uint32_t nb = 1u << bits, mask = nb - 1;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) s_cnt[b] = 0;
    __syncthreads();
    const uint64_t beg = (uint64_t)blockIdx.x * chunk;
    uint64_t end = beg + chunk; if (end > P) end = P;      // blocks past the last pair (the grid covers the capacity) add zeros
    for (uint64_t p = beg + 4u * threadIdx.x; p < end; p += 1024) {
        const uint4 q = *reinterpret_cast<const uint4*>(keys + p);   // (the pair buffers hold a multiple of 4 entries, p is one too)
        const uint32_t k[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int j = 0; j < 4; ++j) if (p + j < end) atomicAdd(&s_cnt[(k[j] >> shift) & mask], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += 256) hist[(size_t)b * nblocks + blockIdx.x] = s_cnt[b];
}

// The first pass of the direct path reads k_setup's segments: a block owns seg.G consecutive setup blocks, whose pairs - segment after
// segment, blk_sums[b] of them at b * seg.S - are its chunk in submission order.
struct SegIn { const uint32_t* blk_sums; const uint32_t* flag; uint32_t nsetup, S, G; };

__global__ __launch_bounds__(256) void k_radix_hist_seg(const uint32_t* __restrict__ seg_k, SegIn seg, const unsigned long long* __restrict__ pairs_total,
                                                        uint32_t cap, int shift, int bits, uint32_t nblocks, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_cnt[1 << RADIX_MAX_BITS];
    const bool live = *seg.flag == 0 && *pairs_total <= cap;      // else nothing is sorted from the segments: every block counts nothing
    const uint32_t nb = 1u << bits, mask = nb - 1;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) s_cnt[b] = 0;
    __syncthreads();
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (live) {
        // one wave per segment, wave w the segments w, w + 4, ...: the first 512 sort words of its (up to) four segments are requested
        // together, the rare rest of a segment in a loop behind them
        static_assert(SEG_MAX_GROUP == 16, "four waves of four segments");
        auto count4 = [&](const uint4 q, uint32_t p, uint32_t n) {
            const uint32_t k[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int j = 0; j < 4; ++j) if (p + j < n) atomicAdd(&s_cnt[(k[j] >> shift) & mask], 1u);
        };
        uint32_t n[4]; const uint32_t* keys[4]; uint4 q[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t sg = w + 4 * j, b = blockIdx.x * seg.G + sg;
            const bool has = sg < seg.G && b < seg.nsetup;
            n[j] = has ? min(seg.blk_sums[b], seg.S) : 0u;
            keys[j] = seg_k + (size_t)(has ? b : 0u) * seg.S;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const uint32_t p = 4 * lane + 256 * it;                       // (S is a multiple of 4)
                q[j][it] = p < n[j] ? *reinterpret_cast<const uint4*>(keys[j] + p) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int it = 0; it < 2; ++it) count4(q[j][it], 4 * lane + 256 * it, n[j]);
            for (uint32_t p = 512 + 4 * lane; p < n[j]; p += 256) count4(*reinterpret_cast<const uint4*>(keys[j] + p), p, n[j]);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += 256) hist[(size_t)b * nblocks + blockIdx.x] = s_cnt[b];
}

// One block per digit: exclusive scan of the digit's row of per-block counts, in place ([digit][block] layout: a row is contiguous),
// and the row's total to totals[digit].  k_radix_scatter adds the exclusive scan of the (at most 256) totals itself.  One launch instead
// of the three of a generic scan over the whole table (17 -> 6 us per pass on the C4 frame).
constexpr int ROWSCAN_THREADS = 1024, ROWSCAN_PER = 8;
__global__ __launch_bounds__(ROWSCAN_THREADS) void k_radix_scan_rows(uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_wave[ROWSCAN_THREADS / 64];
    uint32_t* row = hist + (size_t)blockIdx.x * nblocks;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t running = 0;
    for (uint32_t start = 0; start < nblocks; start += ROWSCAN_THREADS * ROWSCAN_PER) {
        const uint32_t base = start + threadIdx.x * ROWSCAN_PER;
        uint32_t v[ROWSCAN_PER], sum = 0;
#pragma unroll
        for (int k = 0; k < ROWSCAN_PER; ++k) { v[k] = (base + k < nblocks) ? row[base + k] : 0; sum += v[k]; }
        uint32_t inc = sum;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        if (lane == 63) s_wave[w] = inc;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < ROWSCAN_THREADS / 64; ++k) { const uint32_t t = s_wave[k]; if (k < w) wbase += t; tot += t; }
        uint32_t run = running + wbase + inc - sum;
#pragma unroll
        for (int k = 0; k < ROWSCAN_PER; ++k) { if (base + k < nblocks) row[base + k] = run; run += v[k]; }
        running += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = running;
}

// LAST: the pass that leaves the list k_raster reads.  It writes the triangle words and the 16-bit masks only (the sort words are not
// needed behind it) and the tile bounds: in the sorted chunk every run of one tile id is a run of consecutive positions of the
// output, and a tile's slice is the union of its runs over the blocks, so each run takes its first position into tile_start[key]
// (atomicMin; k_chunk_spine sets it to ~0) and its end into tile_end[key] (atomicMax; set to 0).  That is two atomics per run - about
// 128 per block - where k_bounds read the whole sorted key list again.
// f(r) for the rounds r = R, R + 1, ... < N of a wave whose part holds `part` pairs: as long as 64 r < part (r a constant in every call)
template <int R, int N, class F>
__device__ __forceinline__ void rounds_below(uint32_t part, F& f) {
    if constexpr (R < N) {
        if ((uint32_t)(R * 64) < part) { f(R); rounds_below<R + 1, N>(part, f); }
    }
}

// SEG: the first pass of the direct path.  keys_in / vals_in are k_setup's segments and the block's chunk is the pairs of its seg.G setup
// blocks: logical pair p of the chunk, in submission order, sits in segment s at p - s_off[s], for the s with s_off[s] <= p < s_off[s + 1].
// Everything behind the loads - ranks, the reorder, the dense output - is the same code.
template <int RADIX_WAVES, bool WIDE, bool LAST, bool SEG>
__global__ __launch_bounds__(RADIX_WAVES * 64, WIDE ? 2 : 4) void k_radix_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                                 const uint16_t* __restrict__ msk_in,
                                                                 const unsigned long long* __restrict__ pairs_total, uint32_t cap,
                                                                 int shift, int bits, uint32_t nblocks,
                                                                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ totals,
                                                                 uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                                 uint16_t* __restrict__ msk_out,
                                                                 uint32_t* __restrict__ tile_start, uint32_t* __restrict__ tile_end, SegIn seg) {
    constexpr int RADIX_THREADS = RADIX_WAVES * 64, RADIX_CHUNK = RADIX_WAVES * RADIX_WAVE_CHUNK;
    static_assert(!(SEG && WIDE), "the direct path sorts 32-bit sort words only");
    __shared__ uint32_t s_off[SEG ? SEG_MAX_GROUP + 1 : 1];        // pairs of the group before segment s; [SEG_MAX_GROUP] = all of them
    __shared__ uint32_t s_cnt[RADIX_WAVES][1 << RADIX_MAX_BITS];     // per wave: running count, then (after phase 2) local start
    __shared__ uint32_t s_start[1 << RADIX_MAX_BITS];      // first local position of each digit in the chunk
    __shared__ uint32_t s_gbase[1 << RADIX_MAX_BITS];      // global position of the chunk's first pair of each digit
    __shared__ uint32_t s_tot[1 << RADIX_MAX_BITS];        // pairs of all smaller digits in the whole input
    __shared__ uint32_t s_val[RADIX_CHUNK];
    __shared__ __attribute__((aligned(16))) uint32_t s_key[RADIX_CHUNK];
    __shared__ uint16_t s_msk[WIDE ? RADIX_CHUNK : 2];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned long long P64 = *pairs_total;
    const uint32_t P = (P64 > cap || (!SEG && seg.flag && *seg.flag)) ? 0u : (uint32_t)P64;      // (seg.flag in a dense pass: a later pass of the direct path, k_radix_hist)
    // the chunks of this flush: the table has `nblocks` columns (the capacity of the buffers, or the groups), the flush fills the first of them
    uint32_t nchunks = nblocks;
    if (SEG) {
        // the flush does not fit the segments, or the output buffers: the host bins again  (the sizes: k_chunk_spine flags such a flush, never taken)
        if (*seg.flag || P64 > cap || seg.S > SEG_MAX || seg.G > SEG_MAX_GROUP) return;
    } else {
        nchunks = min(nblocks, (uint32_t)(((uint64_t)P + RADIX_CHUNK - 1) / RADIX_CHUNK));
    }
    uint32_t chunk = blockIdx.x;
    if (chunk >= nchunks) return;
    const uint32_t nb = 1u << bits, mask = nb - 1;
    // the prefix sums of a group's segment sizes: pairs of the group before segment s
    auto put_offsets = [&](const uint32_t c) {       // (wave 0; c: blk_sums of the group's lane-th setup block, 0 behind the group)
        const uint32_t inc = wave_incl_scan(c);
        if (lane <= SEG_MAX_GROUP) s_off[lane] = inc - c;     // (lanes from seg.G on hold the total: no pair is looked for behind it)
    };
    auto group_count = [&](const uint32_t c) {
        const uint32_t b = c * seg.G + lane;
        return (lane < seg.G && b < seg.nsetup) ? seg.blk_sums[b] : 0u;
    };
    if (w == 0) {
        if (SEG) put_offsets(group_count(chunk));
        // the pairs of all smaller digits: exclusive scan of the row totals (nb <= 256: up to 4 digits per lane); the same for every chunk
        uint32_t tot[4], run = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const uint32_t d = lane * 4 + q; tot[q] = d < nb ? totals[d] : 0; run += tot[q]; }
        uint32_t inc = run;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        uint32_t ex = inc - run;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const uint32_t d = lane * 4 + q; if (d < nb) s_tot[d] = ex; ex += tot[q]; }
    }
    __syncthreads();
    // The span of a chunk: it holds n pairs, and wave w ranks the `part` of them from w * part on, 64 a round.  Positions are counted
    // inside the chunk from here on.
    // (SEG: s_off must hold the group's offsets.  A group rarely fills the chunk, so its pairs are dealt to the waves in equal parts, in
    // order - fewer rounds for every wave instead of idle last waves; a part is a multiple of 64, and the rounds behind it are skipped)
    struct Span { uint32_t n, part; };
    auto span_of = [&](const uint32_t c) {
        Span sp;
        if (SEG) {
            sp.n = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_off[SEG_MAX_GROUP]);
            sp.part = ((sp.n + RADIX_THREADS - 1) / RADIX_THREADS) * 64;
        } else {
            const uint64_t cbeg = (uint64_t)c * RADIX_CHUNK;
            sp.n = (uint32_t)min((uint64_t)RADIX_CHUNK, (uint64_t)P - cbeg);      // (c < nchunks: cbeg < P)
            sp.part = RADIX_WAVE_CHUNK;
        }
        return sp;
    };
    Span cur = span_of(chunk);
    if (SEG && cur.n > (uint32_t)RADIX_CHUNK) return;      // (k_chunk_spine flags such a flush: never taken; block-uniform)
    const unsigned long long lt = (1ull << lane) - 1ull;

    // the wave's match table of phase 1, a 64-bit word per digit: in s_key, which is idle until phase 3 (a wave's share of s_key holds 512)
    static_assert(RADIX_WAVE_CHUNK * sizeof(uint32_t) >= (sizeof(unsigned long long) << RADIX_MAX_BITS), "a match table per wave in s_key");
    unsigned long long* const match = reinterpret_cast<unsigned long long*>(s_key) + (size_t)w * (RADIX_WAVE_CHUNK / 2);
    uint32_t k[RADIX_ROUNDS], v[RADIX_ROUNDS], rk[RADIX_ROUNDS];
    uint16_t mk[WIDE ? RADIX_ROUNDS : 1];
    // round r of wave w of chunk c into k[r], v[r] (mk[r]).  The addresses are a base that is the same for the whole block plus a 32-bit
    // offset, so that the sixteen rounds in flight do not hold sixteen 64-bit addresses in registers.
    auto load_round = [&](const int r, const uint32_t c, const Span& sp) {
        const uint32_t q0 = (uint32_t)w * sp.part + lane, q = q0 + (uint32_t)r * 64;
        // (q < n, written so that the round's part of it is scalar arithmetic; positions are below 2^14)
        const bool act = (int)q0 < (int)sp.n - r * 64 && (!SEG || (uint32_t)(r * 64) < sp.part);
        if (SEG) {
            // (a binary search over the group's 17 offsets per pair; measured against a table of the segment every 64th pair sits in
            // and a walk from there: 98.6 against 104.5 us on the C4 frame)
            uint32_t sg = 0;
            if (act) {
#pragma unroll
                for (uint32_t st = SEG_MAX_GROUP / 2; st; st >>= 1) if (q >= s_off[sg + st]) sg += st;
            }
            const size_t group = (size_t)c * seg.G * seg.S;
            const uint32_t a = sg * seg.S + (q - s_off[sg]);       // (G S <= 16 x 4096)
            k[r] = act ? (keys_in + group)[a] : 0; v[r] = act ? (vals_in + group)[a] : 0;
        } else {
            const size_t cbeg = (size_t)c * RADIX_CHUNK;
            k[r] = act ? (keys_in + cbeg)[q] : 0; v[r] = act ? (vals_in + cbeg)[q] : 0;
            if (WIDE) mk[WIDE ? r : 0] = act ? (msk_in + cbeg)[q] : (uint16_t)0;
        }
    };
#pragma unroll
    for (int r = 0; r < RADIX_ROUNDS; ++r) load_round(r, chunk, cur);

    // A block takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ... and never waits for another block.  While it reorders and writes
    // chunk i, the loads of chunk i + 1 are in flight: round r of the next chunk is requested as soon as phase 3 has consumed k[r], v[r]
    // and rk[r], so the registers of one chunk serve both.  Five block barriers per chunk.  What one chunk's phases share with the
    // next one's: s_off is written in phase 2 for the NEXT group (its last readers were the loads of phase 3 of the chunk before, so one
    // copy is enough); s_gbase and s_start are written behind the barrier that follows the ranking; s_key holds the match tables of
    // the ranking, hence the barrier at the bottom of the loop.
    for (;;) {
    const uint32_t next = chunk + gridDim.x;
    bool more = next < nchunks;
    const uint32_t wave_part = cur.part, n_chunk = cur.n;
    const int pos0 = (int)((uint32_t)w * wave_part + lane);      // the lane's pair of round r is pos0 + 64 r, and is there if that is < n_chunk
    // requested here, used behind the ranking: pairs of each digit in the chunks before this one (k_radix_scan_rows), and the segment
    // sizes of the next group
    const uint32_t gb = threadIdx.x < nb ? base[(size_t)threadIdx.x * nblocks + chunk] : 0u;      // (nb <= 256 <= RADIX_THREADS)
    uint32_t next_count = 0;
    if (SEG && w == 0 && more) next_count = group_count(next);
    for (uint32_t d = lane; d < nb; d += 64) { s_cnt[w][d] = 0; match[d] = 0ull; }
    __builtin_amdgcn_wave_barrier();
    // ---- phase 1: stable rank of every pair among the equal digits of its wave's part ------------
    auto rank_round = [&](const int r) {
        const bool act = pos0 < (int)n_chunk - r * 64;
        const uint32_t dgt = (k[r] >> shift) & mask;
        // the lanes of the round that hold the same digit: every lane ORs its bit into the digit's word of the wave's match table, then
        // reads the word back (a wave's LDS operations complete in the order they were issued); the first lane of a digit leaves the
        // word 0 for the next round.  OR does not depend on the order of the lanes and the ranks come from the lane numbers, so
        // the sort stays stable; lanes past the chunk's end take no part.
        unsigned long long* const slot = match + dgt;
        if (act) __hip_atomic_fetch_or(slot, lt + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_wave_barrier();
        const unsigned long long same = act ? __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 0ull;
        const uint32_t cur = act ? s_cnt[w][dgt] : 0;
        __builtin_amdgcn_wave_barrier();
        const uint32_t r_in = __popcll(same & lt);
        rk[r] = cur + r_in;
        asm volatile("" : "+v"(rk[r]));      // (one register per round from here on, not the count and the mask it is made of)
        if (act && r_in == 0) { s_cnt[w][dgt] = cur + (uint32_t)__popcll(same); *slot = 0ull; }
        __builtin_amdgcn_wave_barrier();
    };
    if constexpr (SEG) {
        rounds_below<0, RADIX_ROUNDS>(wave_part, rank_round);       // (one forward branch out of the unrolled rounds, wave-uniform)
    } else {
#pragma unroll
        for (int r = 0; r < RADIX_ROUNDS; ++r) rank_round(r);
    }
    __syncthreads();
    // ---- phase 2: local layout: digits ascending, inside a digit waves ascending ------------------------
    if (threadIdx.x < nb) s_gbase[threadIdx.x] = gb + s_tot[threadIdx.x];
    if (w == 0) {
        // (the offsets of the next group: the last reader of this group's was phase 3 of the chunk before)
        if (SEG && more) put_offsets(next_count);
        // exclusive scan over digits of the chunk totals (nb <= 256: up to 4 digits per lane)
        uint32_t tot[4], run = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t d = lane * 4 + q;
            uint32_t t = 0;
            if (d < nb) {
#pragma unroll
                for (int ww = 0; ww < RADIX_WAVES; ++ww) t += s_cnt[ww][d];
            }
            tot[q] = t;
            run += tot[q];
        }
        uint32_t inc = run;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        uint32_t ex = inc - run;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const uint32_t d = lane * 4 + q; if (d < nb) s_start[d] = ex; ex += tot[q]; }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < nb; d += RADIX_THREADS) {
        uint32_t run = s_start[d];
#pragma unroll
        for (int ww = 0; ww < RADIX_WAVES; ++ww) { const uint32_t c = s_cnt[ww][d]; s_cnt[ww][d] = run; run += c; }
    }
    Span nxt = cur;
    if (more) {
        nxt = span_of(next);        // (SEG: s_off holds the next group's offsets from here on)
        if (SEG && nxt.n > (uint32_t)RADIX_CHUNK) more = false;      // (k_chunk_spine flags such a flush: never taken; block-uniform)
    }
    __syncthreads();
    // ---- phase 3: reorder in LDS (4-byte words: lanes of one digit write consecutive banks), and request the next chunk ----------
    auto place_round = [&](const int r) {
        if (pos0 < (int)n_chunk - r * 64) {
            const uint32_t dgt = (k[r] >> shift) & mask;
            const uint32_t lp = s_cnt[w][dgt] + rk[r];
            s_key[lp] = k[r]; s_val[lp] = v[r];
            if (WIDE) s_msk[lp] = mk[WIDE ? r : 0];
        }
    };
#pragma unroll
    for (int r = 0; r < RADIX_ROUNDS; ++r) {
        if (!SEG || (uint32_t)(r * 64) < wave_part) place_round(r);        // (wave-uniform)
        if (more && (!SEG || (uint32_t)(r * 64) < nxt.part)) load_round(r, next, nxt);
    }
    __syncthreads();
    // ---- phase 4: linear read-out, contiguous global runs per digit ------------------------------------------
    constexpr uint32_t KEY_MASK = WIDE ? 0xffffffffu : 0xffffu;
    for (uint32_t i = threadIdx.x; i < n_chunk; i += RADIX_THREADS) {
        const uint32_t word = s_key[i];
        const uint32_t dgt = (word >> shift) & mask;
        const uint32_t dst = s_gbase[dgt] + (i - s_start[dgt]);
        vals_out[dst] = s_val[i];
        if (!LAST) {
            keys_out[dst] = word;
            if (WIDE) msk_out[dst] = s_msk[i];
        } else {
            msk_out[dst] = WIDE ? s_msk[i] : (uint16_t)(word >> 16);
            const uint32_t key = word & KEY_MASK;
            if (i == 0 || (s_key[i - 1] & KEY_MASK) != key) atomicMin(&tile_start[key], dst);
            if (i + 1 == n_chunk || (s_key[i + 1] & KEY_MASK) != key) atomicMax(&tile_end[key], dst + 1);
        }
    }
    if (!more) break;
    chunk = next; cur = nxt;
    __syncthreads();        // (the match tables of the next chunk's ranking lie in s_key, which the write-out reads)
    }
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------
namespace trgl {

uint32_t setup_num_blocks(uint32_t n) { return (n + SETUP_THREADS - 1) / SETUP_THREADS; }

void launch_setup(hipStream_t s, const FrameParams& fp, const DrawDesc& draw, DrawDesc* draws_dev, int draw_idx, uint32_t n,
                  TriRec* recs, TriW* recs_w, uint32_t* cnt, uint2* tilebox, DevStats* stats, uint32_t* blk_sums, uint32_t blk_base,
                  const SegLayout* seg) {
    if (!n) return;
    hipLaunchKernelGGL(k_setup, dim3(setup_num_blocks(n)), dim3(SETUP_THREADS), 0, s, fp, draw, draws_dev, draw_idx, recs, recs_w, cnt, tilebox,
                       stats, blk_sums, blk_base, seg ? seg->keys : nullptr, seg ? seg->vals : nullptr, seg ? seg->S : 0u);
}

void launch_chunk_spine(hipStream_t s, const uint32_t* blk_sums, uint32_t nblk, uint32_t* chunk_off, unsigned long long* total64, unsigned long long* host_copy,
                        uint32_t* tile_bounds, size_t half_words, uint32_t seg_S, uint32_t seg_G, uint32_t seg_chunk, uint32_t* seg_flag,
                        uint32_t* seg_flag_host) {
    hipLaunchKernelGGL(k_chunk_spine, dim3(1), dim3(SPINE_THREADS), 0, s, blk_sums, nblk, chunk_off, total64, host_copy, (uint4*)tile_bounds,
                       (uint32_t)(half_words / 4), seg_S, seg_G, seg_chunk, seg_flag, seg_flag_host);
}

void launch_expand(hipStream_t s, const FrameParams& fp, uint32_t first, uint32_t n, int tiles_x, const uint32_t* cnt, const uint32_t* blk_sums,
                   const uint32_t* chunk_off, uint32_t blk_base, const uint2* tilebox, uint32_t* keys, bool wide, uint32_t* vals, uint16_t* bmask,
                   const unsigned long long* pairs_total, uint32_t cap) {
    if (!n) return;
    if (wide)
        hipLaunchKernelGGL(k_expand<true>, dim3(setup_num_blocks(n)), dim3(SETUP_THREADS), 0, s, fp, first, n, tiles_x, cnt, blk_sums, chunk_off,
                           blk_base, tilebox, keys, vals, bmask, pairs_total, cap);
    else
        hipLaunchKernelGGL(k_expand<false>, dim3(setup_num_blocks(n)), dim3(SETUP_THREADS), 0, s, fp, first, n, tiles_x, cnt, blk_sums, chunk_off,
                           blk_base, tilebox, keys, vals, bmask, pairs_total, cap);
}

static uint32_t radix_waves(uint32_t cap) { return cap >= RADIX_BIG_CAP ? 8u : 4u; }
uint32_t radix_chunk(uint32_t cap) { return radix_waves(cap) * RADIX_WAVE_CHUNK; }
// blocks of a pass over pair buffers of capacity `cap`
uint32_t radix_num_workers(uint32_t cap) { const uint64_t chunk = radix_chunk(cap); return (uint32_t)((cap + chunk - 1) / chunk); }
uint32_t seg_num_groups(const SegLayout& seg) { return (seg.nsetup + seg.G - 1) / seg.G; }
bool seg_layout_ok(const SegLayout& seg) { return seg.S >= 4 && seg.S <= SEG_MAX && seg.S % 4 == 0 && seg.G >= 1 && seg.G <= SEG_MAX_GROUP; }

// The pair count of the flush stays on the device (`pairs_total`): grids cover `cap`, the capacity of the pair buffers,
// and blocks past the last pair do nothing, so the host never has to wait for the count before it can queue these.
// The scatter's grid: as many blocks as the device holds at once, at most one per chunk (`chunks`: the columns of the table) and at
// most `max_blocks` (0: no such limit); every block walks its chunks with a stride of the grid.  The blocks per CU of a variant are
// asked for once per thread and device.
template <int WAVES, bool WIDE, bool LAST, bool SEG>
static uint32_t scatter_grid(uint32_t chunks, uint32_t max_blocks) {
    thread_local int for_dev = -1;
    thread_local uint32_t resident = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev != for_dev) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_radix_scatter<WAVES, WIDE, LAST, SEG>, WAVES * 64, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
        resident = (uint32_t)per_cu * (uint32_t)cus;
        for_dev = dev;
    }
    uint32_t g = std::min(chunks, resident);
    if (max_blocks) g = std::min(g, max_blocks);
    return std::max(g, 1u);
}

template <int WAVES, bool WIDE, bool LAST>
static uint32_t radix_pass_t(hipStream_t s, const RadixPass& ps, const unsigned long long* pairs_total, uint32_t cap, uint32_t* hist, uint32_t* scan_tmp,
                             const uint32_t* skip, uint32_t max_blocks) {
    const uint32_t nblk = radix_num_workers(cap), grid = scatter_grid<WAVES, WIDE, LAST, false>(nblk, max_blocks);
    hipLaunchKernelGGL(k_radix_hist, dim3(nblk), dim3(256), 0, s, ps.keys_in, pairs_total, cap, ps.shift, ps.bits, (uint32_t)(WAVES * RADIX_WAVE_CHUNK),
                       nblk, hist, skip);
    hipLaunchKernelGGL(k_radix_scan_rows, dim3(1u << ps.bits), dim3(ROWSCAN_THREADS), 0, s, hist, nblk, scan_tmp);
    hipLaunchKernelGGL((k_radix_scatter<WAVES, WIDE, LAST, false>), dim3(grid), dim3(WAVES * 64), 0, s, ps.keys_in, ps.vals_in, ps.msk_in, pairs_total, cap,
                       ps.shift, ps.bits, nblk, hist, scan_tmp, ps.keys_out, ps.vals_out, ps.msk_out, ps.tile_start, ps.tile_end, SegIn{ nullptr, skip, 0, 0, 0 });
    return grid;
}
// the first pass of the direct path: one chunk per group of seg.G setup blocks, input from their segments
template <int WAVES, bool LAST>
static uint32_t radix_pass_seg(hipStream_t s, const RadixPass& ps, const SegLayout& sl, const unsigned long long* pairs_total, uint32_t cap, uint32_t* hist,
                               uint32_t* scan_tmp, uint32_t max_blocks) {
    const uint32_t nblk = seg_num_groups(sl), grid = scatter_grid<WAVES, false, LAST, true>(nblk, max_blocks);
    const SegIn seg{ sl.blk_sums, sl.flag, sl.nsetup, sl.S, sl.G };
    hipLaunchKernelGGL(k_radix_hist_seg, dim3(nblk), dim3(256), 0, s, sl.keys, seg, pairs_total, cap, ps.shift, ps.bits, nblk, hist);
    hipLaunchKernelGGL(k_radix_scan_rows, dim3(1u << ps.bits), dim3(ROWSCAN_THREADS), 0, s, hist, nblk, scan_tmp);
    hipLaunchKernelGGL((k_radix_scatter<WAVES, false, LAST, true>), dim3(grid), dim3(WAVES * 64), 0, s, sl.keys, sl.vals, ps.msk_in, pairs_total, cap,
                       ps.shift, ps.bits, nblk, hist, scan_tmp, ps.keys_out, ps.vals_out, ps.msk_out, ps.tile_start, ps.tile_end, seg);
    return grid;
}

template <int WAVES>
static uint32_t radix_pass_w(hipStream_t s, const RadixPass& ps, bool wide, bool last, const unsigned long long* pairs_total, uint32_t cap,
                             uint32_t* hist, uint32_t* scan_tmp, const SegLayout* seg, const uint32_t* skip, uint32_t mb) {
    if (seg) return last ? radix_pass_seg<WAVES, true>(s, ps, *seg, pairs_total, cap, hist, scan_tmp, mb) : radix_pass_seg<WAVES, false>(s, ps, *seg, pairs_total, cap, hist, scan_tmp, mb);
    if (wide) return last ? radix_pass_t<WAVES, true, true>(s, ps, pairs_total, cap, hist, scan_tmp, skip, mb) : radix_pass_t<WAVES, true, false>(s, ps, pairs_total, cap, hist, scan_tmp, skip, mb);
    return last ? radix_pass_t<WAVES, false, true>(s, ps, pairs_total, cap, hist, scan_tmp, skip, mb) : radix_pass_t<WAVES, false, false>(s, ps, pairs_total, cap, hist, scan_tmp, skip, mb);
}

uint32_t launch_radix_pass(hipStream_t s, const RadixPass& ps, bool wide, bool last, const unsigned long long* pairs_total, uint32_t cap,
                           uint32_t* hist, uint32_t* scan_tmp, const SegLayout* seg, const uint32_t* skip, uint32_t max_blocks) {
    if (!cap || (seg && (wide || !seg->nsetup))) return 0;
    if (radix_waves(cap) == 8) return radix_pass_w<8>(s, ps, wide, last, pairs_total, cap, hist, scan_tmp, seg, skip, max_blocks);
    return radix_pass_w<4>(s, ps, wide, last, pairs_total, cap, hist, scan_tmp, seg, skip, max_blocks);
}

}  // namespace trgl
