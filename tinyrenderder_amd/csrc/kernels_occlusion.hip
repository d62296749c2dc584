// kernels_occlusion.hip — occlusion culling of boxes against a depth image (include/trgl.h: trgl_occlusion_boxes_image), gfx950.
//
//   k_occl_build : one pass over the depths that leaves two levels of maxima, of the 8 x 8 and of the 64 x 64 pixel blocks.
//   k_occl_query : one wavefront per box: steps 1-6 of the header (occlusion_core.h, the host path's very functions), then step 7 -
//                  is some depth of the rectangle above zq - answered from the levels where a block lies wholly inside the rectangle
//                  and from the depths along the border.
// Both levels are exact maxima (a NaN counts as -inf: nothing passes our_gl.cpp:165 against it; an edge block covers the pixels that
// exist), and "zq < the maximum of a set" is "zq < some member of it", so the codes are those of a scan of every pixel.  The sign of a
// zero maximum depends on the order it was taken in; no comparison sees it.
//
// k_occl_build.  A workgroup of four waves owns one 64 x 64 block.  A row of it is 512 bytes: 32 lanes x 16 bytes, so a wave reads two
// rows per load and four loads cover the 8 rows of a band of level-1 blocks; wave v takes bands v and v + 4, its 8 loads issued before
// the first maximum.  A lane owns columns 2c and 2c + 1 (c = lane & 31): four neighbouring lanes and the wave's two half-waves hold one
// 8 x 8 block, three xor steps fold it, and lanes 0, 4, .. 28 store a band's 8 maxima as 64 contiguous bytes.  Level 2 takes three more
// xor steps and four words of LDS.  Whether a row's pairs are 16-byte aligned depends on the base address and on y * w: where they are
// not, the lane reads the aligned pair one column to the right (columns 2c + 1, 2c + 2), lane 31 reads columns 63 and 0 by themselves, and
// column 2c arrives from the lane to the left by a rotation within the half-wave.  A pair cut by the image's right edge is read as
// single doubles.
//
// k_occl_query.  Every lane transforms corner lane & 7, so three xor steps leave the fold of all 8 corners in every lane.  The
// rectangle then falls into: the level-2 blocks wholly inside it; around them the ring of level-1 blocks wholly inside it (at most 7
// wide); around those the ring of pixels (at most 7 wide).  A ring is up to four rectangles of an array; the wave lays its lanes over
// a rectangle as 64 x 1, 32 x 2, .. 1 x 64, whichever is the narrowest that spans it, reads four such steps, and leaves on the first
// ballot that has a bit set.
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "occlusion_core.h"

namespace {

using namespace trgl;

typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double occl_clean(double v) { return v == v ? v : -__builtin_inf(); }     // a NaN counts as -inf
__device__ __forceinline__ double occl_xor_max(double v, int mask) { return dmax(v, __shfl_xor(v, mask)); }

// levels: level 1 [h1][w1], then level 2 [h2][w2]
__global__ __launch_bounds__(256) void k_occl_build(const double* __restrict__ depth, int w, int h, int w1, int h1, int w2,
                                                    double* __restrict__ levels) {
    static_assert(OCCL_L1 == 8 && OCCL_L2 == 64, "a wave reads 2 rows of 64 pixels per load, 4 loads per band of 8 x 8 blocks");
    __shared__ double s_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, half = lane >> 5;
    const int bx2 = blockIdx.x % (uint32_t)w2, by2 = blockIdx.x / (uint32_t)w2;
    const int64_t X0 = (int64_t)bx2 * OCCL_L2, Y0 = (int64_t)by2 * OCCL_L2;
    const int cols = (int)((int64_t)w - X0 < OCCL_L2 ? (int64_t)w - X0 : OCCL_L2);                   // columns of the block that exist
    const double ninf = -__builtin_inf();
    const uint32_t base_odd = (uint32_t)(reinterpret_cast<uintptr_t>(depth) >> 3) & 1u;

    double a[8], b[8];          // per load: the pair read (aligned row: columns 2c, 2c + 1; else 2c + 1, 2c + 2 - lane 31: 63, 0)
    bool odd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int band = wave + 4 * (k >> 2);
        const int64_t y = Y0 + 8 * band + 2 * (k & 3) + half;
        a[k] = ninf; b[k] = ninf; odd[k] = false;
        if (y < h) {
            const int64_t e = y * w + X0;                                                          // index of the row's first pixel of the block
            const double* row = depth + e;
            odd[k] = (((uint32_t)e & 1u) ^ base_odd) != 0;
            const int ca = odd[k] ? 2 * c + 1 : 2 * c;
            const int cb = odd[k] ? (c == 31 ? 0 : 2 * c + 2) : 2 * c + 1;
            if (cb == ca + 1 && cb < cols) {
                const f64x2 v = *reinterpret_cast<const f64x2*>(row + ca);
                a[k] = v.x; b[k] = v.y;
            } else {
                if (ca < cols) a[k] = row[ca];
                if (cb < cols) b[k] = row[cb];
            }
        }
    }
    double band_max[2] = { ninf, ninf };
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // column 2c of an unaligned row is what the lane to the left (lane 31 for lane 0) holds as its second value
        const double left = __shfl(b[k], (lane & 32) | ((c + 31) & 31));
        const double v0 = occl_clean(odd[k] ? left : a[k]), v1 = occl_clean(odd[k] ? a[k] : b[k]);
        band_max[k >> 2] = dmax(band_max[k >> 2], dmax(v0, v1));
    }
    double m2 = ninf;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double m = band_max[j];
        m = occl_xor_max(m, 1); m = occl_xor_max(m, 2); m = occl_xor_max(m, 32);                    // the 8 x 8 block of columns 8 (c >> 2) ..
        const int64_t y1 = (int64_t)by2 * 8 + wave + 4 * j, x1 = (int64_t)bx2 * 8 + (c >> 2);
        if ((lane & 35) == 0 && y1 < h1 && x1 < w1) levels[y1 * w1 + x1] = m;
        m2 = dmax(m2, m);
    }
    m2 = occl_xor_max(m2, 4); m2 = occl_xor_max(m2, 8); m2 = occl_xor_max(m2, 16);
    if (lane == 0) s_max[wave] = m2;
    __syncthreads();
    if (threadIdx.x == 0) levels[(int64_t)w1 * h1 + blockIdx.x] = dmax(dmax(s_max[0], s_max[1]), dmax(s_max[2], s_max[3]));
}

// Is zq < p[x + y * stride] for some x0 <= x <= x1, y0 <= y <= y1?  Wave-uniform arguments and result; an empty rectangle: no.
__device__ bool occl_scan(const double* __restrict__ p, int64_t stride, int64_t x0, int64_t x1, int64_t y0, int64_t y1, double zq, int lane) {
    if (x0 > x1 || y0 > y1) return false;
    int lw_log2 = 0;
    while (lw_log2 < 6 && ((int64_t)1 << lw_log2) <= x1 - x0) ++lw_log2;                           // the narrowest power of two that spans the columns, at most 64
    const int lw = 1 << lw_log2, lh = 64 >> lw_log2;
    const int lx = lane & (lw - 1), ly = lane >> lw_log2;
    for (int64_t yb = y0; yb <= y1; yb += 4 * lh)
        for (int64_t xb = x0; xb <= x1; xb += lw) {
            const int64_t x = xb + lx;
            bool hit = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t y = yb + u * lh + ly;
                if (x <= x1 && y <= y1) hit |= zq < p[y * stride + x];                             // a NaN never, +inf always
            }
            if (__any(hit)) return true;
        }
    return false;
}

// ... for some (x, y) of [x0, x1] x [y0, y1] outside the hole [hx0, hx1] x [hy0, hy1], which lies inside the rectangle or is empty
__device__ bool occl_scan_ring(const double* __restrict__ p, int64_t stride, int64_t x0, int64_t x1, int64_t y0, int64_t y1,
                               int64_t hx0, int64_t hx1, int64_t hy0, int64_t hy1, double zq, int lane) {
    if (hx0 > hx1 || hy0 > hy1) return occl_scan(p, stride, x0, x1, y0, y1, zq, lane);
    return occl_scan(p, stride, x0, x1, y0, hy0 - 1, zq, lane) || occl_scan(p, stride, x0, x1, hy1 + 1, y1, zq, lane) ||
           occl_scan(p, stride, x0, hx0 - 1, hy0, hy1, zq, lane) || occl_scan(p, stride, hx1 + 1, x1, hy0, hy1, zq, lane);
}

// The blocks of `side` pixels wholly inside the pixels [p0, p1] of an axis of `extent` pixels, p1 <= extent - 1: the last block is
// ragged and ends where the axis does.  Empty: *b0 > *b1.
__device__ __forceinline__ void occl_blocks_inside(int p0, int p1, int extent, int side, int64_t* b0, int64_t* b1) {
    *b0 = ((int64_t)p0 + side - 1) / side;
    *b1 = p1 == extent - 1 ? ((int64_t)extent - 1) / side : ((int64_t)p1 + 1) / side - 1;
}

__global__ __launch_bounds__(64 * OCCL_QUERY_BOXES) void k_occl_query(OcclArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t box = (uint64_t)blockIdx.x * OCCL_QUERY_BOXES + (threadIdx.x >> 6);
    if (box >= a.n) return;                                                                        // (a whole wave; the kernel has no barrier)
    const double* src = a.boxes + box * 6;
    double bx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) bx[k] = src[k];
    OcclFold f = occl_corner(a.M, a.V, bx, lane & 7);                                              // steps 1-3, 5
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        OcclFold o;
        o.zmin = __shfl_xor(f.zmin, m); o.zmax = __shfl_xor(f.zmax, m);
        o.sx_min = __shfl_xor(f.sx_min, m); o.sx_max = __shfl_xor(f.sx_max, m);
        o.sy_min = __shfl_xor(f.sy_min, m); o.sy_max = __shfl_xor(f.sy_max, m);
        o.undecided = __shfl_xor(f.undecided, m);
        f = occl_merge(f, o);
    }
    OcclRect r;
    int code = occl_decide(f, a.w, a.h, &r);                                                       // steps 4-6; the same in every lane
    if (code < 0) {                                                                                // step 7
        const int64_t w1 = ((int64_t)a.w + OCCL_L1 - 1) / OCCL_L1, h1 = ((int64_t)a.h + OCCL_L1 - 1) / OCCL_L1;
        const int64_t w2 = ((int64_t)a.w + OCCL_L2 - 1) / OCCL_L2;
        const double* l1 = a.levels; const double* l2 = a.levels + w1 * h1;
        int64_t X2a, X2b, Y2a, Y2b, X1a, X1b, Y1a, Y1b;
        occl_blocks_inside(r.x0, r.x1, a.w, OCCL_L2, &X2a, &X2b); occl_blocks_inside(r.y0, r.y1, a.h, OCCL_L2, &Y2a, &Y2b);
        occl_blocks_inside(r.x0, r.x1, a.w, OCCL_L1, &X1a, &X1b); occl_blocks_inside(r.y0, r.y1, a.h, OCCL_L1, &Y1a, &Y1b);
        const bool any2 = X2a <= X2b && Y2a <= Y2b, any1 = X1a <= X1b && Y1a <= Y1b;
        // the level-2 blocks in level-1 blocks, the level-1 blocks in pixels: the holes of the two rings
        const int64_t r1 = OCCL_L2 / OCCL_L1;
        const int64_t HX1a = X2a * r1, HX1b = X2b * r1 + r1 - 1 < w1 - 1 ? X2b * r1 + r1 - 1 : w1 - 1;
        const int64_t HY1a = Y2a * r1, HY1b = Y2b * r1 + r1 - 1 < h1 - 1 ? Y2b * r1 + r1 - 1 : h1 - 1;
        const int64_t HXa = X1a * OCCL_L1, HXb = X1b * OCCL_L1 + OCCL_L1 - 1 < a.w - 1 ? X1b * OCCL_L1 + OCCL_L1 - 1 : a.w - 1;
        const int64_t HYa = Y1a * OCCL_L1, HYb = Y1b * OCCL_L1 + OCCL_L1 - 1 < a.h - 1 ? Y1b * OCCL_L1 + OCCL_L1 - 1 : a.h - 1;
        bool vis = any2 && occl_scan(l2, w2, X2a, X2b, Y2a, Y2b, r.zq, lane);
        if (!vis && any1)
            vis = any2 ? occl_scan_ring(l1, w1, X1a, X1b, Y1a, Y1b, HX1a, HX1b, HY1a, HY1b, r.zq, lane)
                       : occl_scan(l1, w1, X1a, X1b, Y1a, Y1b, r.zq, lane);
        if (!vis)
            vis = any1 ? occl_scan_ring(a.depth, a.w, r.x0, r.x1, r.y0, r.y1, HXa, HXb, HYa, HYb, r.zq, lane)
                       : occl_scan(a.depth, a.w, r.x0, r.x1, r.y0, r.y1, r.zq, lane);
        code = vis ? TRGL_OCCL_VISIBLE : TRGL_OCCL_HIDDEN;
    }
    if (lane == 0) a.codes[box] = (uint8_t)code;
}

}  // namespace

namespace trgl {

size_t occl_level_doubles(int w, int h) {
    const size_t w1 = ((size_t)w + OCCL_L1 - 1) / OCCL_L1, h1 = ((size_t)h + OCCL_L1 - 1) / OCCL_L1;
    const size_t w2 = ((size_t)w + OCCL_L2 - 1) / OCCL_L2, h2 = ((size_t)h + OCCL_L2 - 1) / OCCL_L2;
    return w1 * h1 + w2 * h2;
}

void launch_occl_build(hipStream_t s, const double* depth, int w, int h, double* levels) {
    // (in 64 bits: a frame one pixel thin may be INT_MAX long)
    const int w1 = (int)(((int64_t)w + OCCL_L1 - 1) / OCCL_L1), h1 = (int)(((int64_t)h + OCCL_L1 - 1) / OCCL_L1);
    const int w2 = (int)(((int64_t)w + OCCL_L2 - 1) / OCCL_L2), h2 = (int)(((int64_t)h + OCCL_L2 - 1) / OCCL_L2);
    hipLaunchKernelGGL(k_occl_build, dim3((uint32_t)w2 * (uint32_t)h2), dim3(256), 0, s, depth, w, h, w1, h1, w2, levels);
}

void launch_occl_query(hipStream_t s, const OcclArgs& a) {
    const uint64_t blocks = (a.n + OCCL_QUERY_BOXES - 1) / OCCL_QUERY_BOXES;
    hipLaunchKernelGGL(k_occl_query, dim3((uint32_t)blocks), dim3(64 * OCCL_QUERY_BOXES), 0, s, a);
}

}  // namespace trgl
