// kernels_raster.hip — the block rasterizer (gfx950): bounding-box scan, barycentric coverage test,
// fp64 z-test and the fragment shader of our_gl.cpp:147-199, one WAVEFRONT per 8x8-pixel block of a 32x32 screen tile.
//
// The block's z-buffer (fp64), colours and owners live in the wave's REGISTERS for the whole kernel (lane = pixel), so the
// compare-and-write of our_gl.cpp:165,191 needs no atomics and no memory at all: one wave walks the tile's triangle list in
// submission order and every lane owns a different pixel.  Depths and colours leave the chip once, at the end, as rows of the
// block; PHONG / EYE pixels are shaded once per visible pixel afterwards (k_shade).
//
// Arithmetic is the reference's, operation for operation, in fp64 with contraction off.  The three
// IEEE divisions per pixel of barycentric() (our_gl.cpp:85) matter because the `>= 0` coverage test
// and the written z depend on their rounding; for well-scaled triangles the same bits come from sign
// tests and FMA divisions by the per-triangle constant u.z ("exactness").
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "shade_common.h"
#include "frag_builtin.h"

namespace {
using namespace trgl_shade;

// v_max_f64 as one instruction (a NaN operand yields the other one): for the depth maxima, where a pixel holding NaN can
// never be written again (z < NaN is false), so leaving it out of a maximum keeps the maximum a valid bound
__device__ __forceinline__ double vmax(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double vmin(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// maximum over the 64 lanes, in every lane (NaN operands are skipped by v_max_f32)
__device__ __forceinline__ float wave_max_f32(float v) {
    float t;
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=&v"(t) : "v"(v)); v = t;
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=&v"(t) : "v"(v)); v = t;
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=&v"(t) : "v"(v)); v = t;
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=&v"(t) : "v"(v)); v = t;
    // every lane now holds the maximum of its row of 16: fold row 0 into 1 and 2 into 3, then rows 0-1 into 2-3; lane 63 has it all
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf" : "=&v"(t) : "v"(v), "0"(v)); v = t;
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf" : "=&v"(t) : "v"(v), "0"(v)); v = t;
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// double -> float rounded towards +inf (NaN stays NaN): a bound that stays a bound in single precision
__device__ __forceinline__ float f32_up(double d) {
    float f = (float)d;
    if ((double)f < d) { const uint32_t b = __float_as_uint(f); f = __uint_as_float((b >> 31) ? b - 1u : b + 1u); }
    return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_raster: ONE WAVEFRONT PER 8x8-PIXEL BLOCK, the block's depths, colours (and owners) in REGISTERS.
//
// A workgroup is four waves = one row of four blocks of a 32x32 tile; all sixteen block waves of a tile walk the tile's
// triangle list (submission order, from the binning) on their own, without barriers.  Lane l of a wave owns pixel
// (l & 7, l >> 3) of the block for the whole kernel: its depth is a register pair, the compare-and-write of our_gl.cpp:165,191
// is two register moves, nothing about a pixel ever goes through LDS, and every pixel leaves the chip exactly once at the end
// (depth 8 B, colour bpp B, written as whole rows of the block).
//
// Per wave:
//  1. candidates   The pairs of the tile carry a 4x4 mask of the tile's blocks that the triangle's clamped bbox reaches
//                  (k_expand); the wave takes the entries with its bit, 64 list entries per step, and compacts their triangle
//                  ids into a small ring in LDS (order preserved).
//  2. cull         Whenever 64 candidates are waiting (or the list ends): lane = candidate.  The lane reads 96 B of its
//                  triangle's record and drops the triangle when one of the three edge functions excludes every pixel of
//                  (bbox n block) or when its depth plane cannot get below the block's largest stored depth (both tests in fp64
//                  with margins 2^10 times the rounding they cover; "edge" and "depth" below).  The gather of a round is requested
//                  one round ahead: between the test of the round before it and the visits of that round's survivors.
//  3. visits       The survivors (compacted into the low lanes), in list order.  The triangle's constants arrive as wave-uniform
//                  values through the scalar cache (two s_load_dwordx16 = the whole record, requested one visit ahead), so the
//                  vector instructions take them as scalar operands and no vector register holds a per-triangle constant.
//                  Per visit, one pixel per lane: depth plane against the lane's stored depth, barycentric() + sign coverage test
//                  (no bbox test: k_setup sends the slivers that would need one down the literal path).  That is where a visit
//                  ENDS: the covered lanes only note (u.x, u.y, triangle) in registers ...
//  4. resolve      ... and the three divisions of our_gl.cpp:85, the depth of :156-158, the z-test and the fragment run later
//                  for ALL noted lanes at once, each lane with its own triangle (its u.z, 1/u.z, depths and colour were noted too:
//                  no memory access): when a visit covers a lane that still holds a note (so that every pixel sees its
//                  fragments in submission order) and at the end of the list.  Small triangles cover a few lanes each;
//                  resolving several of them together is what fills the lanes of the most expensive part of the pixel loop.
//
// The scalar unit issues one instruction per cycle for the four SIMDs of a CU and was as busy as the vector units in the first
// version of this kernel: the visit loop is written to need few scalar instructions (k_raster).
//
// Exactness: as before, operation for operation in fp64 with contraction off; sign coverage + FMA division by u.z for
// well-scaled triangles ("exactness"), the literal divisions for the others (`dl` bit 31).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KIND_ANY = TRGL_NUM_SHADERS;          // per-fragment switch on the draw's kind (mixed flushes)
constexpr int RING = 512;                           // candidate ring of a wave (triangle ids): a power of two >= 63 left over + 256 of a step

#ifdef TRGL_DEBUG_COUNTERS
#define TRGL_DBG(i, n) do { S.dbg[i] += (unsigned long long)(n); } while (0)
// phase clocks of the diagnostic build: the cycles since the last stamp go to counter i
#ifdef TRGL_DEBUG_NOSTAMP      // (counters 10-13 then describe the first list entry that is no triangle, profiles/one_case.py)
#define TRGL_STAMP(i) ((void)0)
#else
#define TRGL_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); S.dbg[i] += t_ - S.t_prev; S.t_prev = t_; } while (0)
#endif
#else
#define TRGL_DBG(i, n) ((void)0)
#define TRGL_STAMP(i) ((void)0)
#endif

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// The scan constants of one triangle, wave-uniform (SGPRs): its whole record, two scalar loads of 64 B.
struct TriScan {
    double ax, ay, s0x, s0y, s1x, s1y, c0, uz, g1, g2;
    uint32_t bx, by;      // as stored: bx0 | by0 << 16, bx1 | by1 << 16
    uint32_t color, dl;
    double ruz, z0, z1, z2;       // ride along for the lanes that note a fragment (see BlockState)
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    u32x16 lo, hi;                // the 32 registers as requested: all of them stay allocated until scan_wait()
};
__device__ __forceinline__ TriScan load_scan(const TriRec* __restrict__ recs, uint32_t tri) {
    TriScan T;
#if __HIP_DEVICE_COMPILE__
    // (a flush holds at most TRGL_FLUSH_MAX_TRIS = 2^25 records: the byte offset fits the 32-bit scalar offset of s_load)
    // The record as TWO requests of 16 dwords, written out: from C++ the second half becomes three (8 + 4 + 2 dwords around the bbox,
    // which the fast visit does not use).  The compiler does not know that these registers arrive later: every use is preceded by
    // scan_wait() below, and nothing else may touch them in between (the two sets A and B of the visit loop are never copied).
    TriScan::u32x16 g, h;
    asm volatile("s_load_dwordx16 %0, %2, %3 offset:0x0\n\ts_load_dwordx16 %1, %2, %3 offset:0x40" : "=&s"(g), "=&s"(h) : "s"(recs), "s"(tri << 7));
    T.lo = g; T.hi = h;
#ifdef TRGL_DEBUG_COUNTERS
    // (the diagnostic build keeps so many counters in scalar registers that the compiler spills a set while its request is still out -
    // tools/check_scan_regs.py refuses that; here the request is waited for at once, which costs the visits of THIS build their overlap)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(T.lo), "+s"(T.hi) :: "memory");
    g = T.lo; h = T.hi;
#endif
    auto dg = [&](int i) { return __builtin_bit_cast(double, ((unsigned long long)g[i + 1] << 32) | g[i]); };
    auto dh = [&](int i) { return __builtin_bit_cast(double, ((unsigned long long)h[i + 1] << 32) | h[i]); };
    T.ax = dg(0); T.ay = dg(2); T.s0x = dg(4); T.s0y = dg(6); T.s1x = dg(8); T.s1y = dg(10); T.c0 = dg(12); T.uz = dg(14);
    T.g1 = dh(0); T.g2 = dh(2); T.ruz = dh(4); T.z0 = dh(6); T.z1 = dh(8); T.z2 = dh(10);
    T.bx = h[12]; T.by = h[13]; T.color = h[14]; T.dl = h[15];
#endif
    return T;
}
// (the registers of a set are inputs of the wait: a field that the kernel variant never reads - the bbox, colour or `dl` - would otherwise
// be dead from the start, and its register handed to something else while the load that writes it is still in flight)
__device__ __forceinline__ void scan_wait(const TriScan& T) { asm volatile("s_waitcnt lgkmcnt(0)" :: "s"(T.lo), "s"(T.hi) : "memory"); }

// Per-wave state: the block's pixels (one per lane) and the running statistics of our_gl.cpp:194-198.
struct BlockState {
    double z;               // stored depth of the lane's pixel (-inf: a pixel this wave does not own - never written, never stored)
    uint32_t color;         // its colour, b | g << 8 | r << 16 | a << 24
    uint32_t id;            // PHONG / EYE flushes: draw << 24 | triangle of the fragment that owns the pixel, ~0u = none (k_shade)
    double pxc, pyc;        // pixel centre (x + 0.5, y + 0.5), our_gl.cpp:149
    // deferred fragments: lanes of `pend` hold (u.x, u.y) of barycentric(), their triangle and - copied from the wave-uniform
    // constants of the visit, so that resolving them needs no memory access at all - its u.z, 1/u.z and the three vertex depths
    double pux, puy; uint32_t ptri;
    double puz, pruz, pz0, pz1, pz2;
    uint32_t pcd;           // ... and its colour (FLAT flushes) or `dl` (all others)
    uint32_t frags; double zmax;   // z range of the fragments the lane wrote: the largest one is kept; the smallest IS the pixel's
                                   // final depth (every write lowers it), read off at block-out
    us2 xy;                 // x | y << 16 as two 16-bit words (the bbox test of a visit is packed 16-bit arithmetic)
#ifdef TRGL_DEBUG_COUNTERS
    unsigned long long dbg[16];    // work counters of the diagnostic build (profiles/raster_counters.py); [8] is summed over the lanes
    unsigned long long t_prev;
#endif
};

// Resolve the deferred fragments: our_gl.cpp:85 (the three quotients), :156-165 (depth, finite check, strict z-test), :168-192
// (perspective-correct barycentrics, fragment, writes) and :194-198 (counters), each lane for its own triangle.
template <int KIND, bool ALLWS, bool DEFERRED>
__device__ __forceinline__ void resolve(BlockState& S, unsigned long long pend, const TriRec* __restrict__ recs, const TriW* __restrict__ recs_w,
                                        const DrawDesc* __restrict__ draws, DevStats* __restrict__ stats, bool zero_locked) {
    TRGL_DBG(6, 1); TRGL_DBG(7, __popcll(pend));
#ifdef TRGL_DEBUG_COUNTERS
    const unsigned long long t_res = __builtin_amdgcn_s_memtime();
#endif
    // PLAIN: every fragment of the flush is FLAT, PHONG or EYE: its colour / owner id depends on the triangle only and rides with the
    // deferred fragment (S.pcd), so resolving touches no memory at all.
    constexpr bool PLAIN = KIND == TRGL_SHADER_FLAT || KIND == TRGL_SHADER_PHONG || KIND == TRGL_SHADER_EYE;
    if (__builtin_amdgcn_inverse_ballot_w64(pend)) {
        const double uz = S.puz, ruz = S.pruz, z0 = S.pz0, z1 = S.pz1, z2 = S.pz2;
        const double ux = S.pux, uy = S.puy, us = ux + uy;
        double b0, b1, b2;
        if (ALLWS || ruz != 0.0) {
            b0 = 1.0 - div_by_uz(us, uz, ruz);                              // :85 through the reciprocal ("exactness")
            b1 = div_by_uz(uy, uz, ruz);
            b2 = div_by_uz(ux, uz, ruz);
        } else {
            b0 = 1.0 - us / uz;                                             // :85, as written
            b1 = uy / uz;
            b2 = ux / uz;
        }
        const double z = b0 * z0 + b1 * z1 + b2 * z2;                       // :156-158
        if (__builtin_isfinite(z) && (z < S.z)) {                           // :160, :165
            uint32_t color = S.pcd, id = 0xffffffffu;
            bool discard = false;
            if (KIND == TRGL_SHADER_PHONG || KIND == TRGL_SHADER_EYE) id = TRGL_DL_ID(S.pcd);
            if (!PLAIN) {
                const uint32_t dl = S.pcd;
                color = recs[S.ptri].color;
                const DrawDesc* d = draws + TRGL_DL_DRAW(dl);
                const int kind = KIND == KIND_ANY ? d->kind : KIND;
                if (kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE || kind >= TRGL_SHADER_USER_FIRST) {
                    // not shaded here: the pixel remembers which triangle owns it and k_shade (or the user kind's shade kernel,
                    // shade_user.h) runs the fragment shader once per visible pixel (these shaders have no side effects and never
                    // discard, so the image is the same as shading every z-pass in order, and the counters do not depend on colours)
                    id = TRGL_DL_ID(dl);
                } else if (kind != TRGL_SHADER_FLAT) {
                    const TriW w = recs_w[S.ptri];
                    double pc[3];
                    const double denom = b0 * w.iw0 + b1 * w.iw1 + b2 * w.iw2;                    // :172-174
                    if (fabs(denom) < 1e-15) { pc[0] = b0; pc[1] = b1; pc[2] = b2; }              // :177-185
                    else { pc[0] = (b0 * w.iw0) / denom; pc[1] = (b1 * w.iw1) / denom; pc[2] = (b2 * w.iw2) / denom; }
                    if (kind == TRGL_SHADER_GOURAUD) {
                        const double* vary = d->vary + (size_t)TRGL_DL_LOCAL(dl) * 3;
                        const double vv[3] = { vary[0], vary[1], vary[2] };
                        color = frag_gouraud(color, vv, pc);
                    } else {                                                                      // TRGL_SHADER_CHECKER
                        discard = frag_checker_discards(d->u.reserved, pc);                       // our_gl.cpp:187-188
                    }
                }
            }
            if (!discard) {
                // :191-198, committed IN PLACE (asm operands tied to the state registers): written through ordinary assignments the
                // compiler gives every state variable a second register inside the conditional resolve and copies all of them back at
                // its end - nine moves per covered visit.  v_max gives std::max up to the sign of a zero, which k_fold_stats settles
                // from the first-zero keys below (as it does for the minimum, taken from the final depths at block-out).
                asm volatile(
                    "v_mov_b64 %[sz], %[z]\n\t"                                                // :191
                    "v_add_u32 %[fr], 1, %[fr]\n\t"                                            // :194
                    "v_max_f64 %[zmax], %[zmax], %[z]"                                           // :198
                    : [sz] "+v"(S.z), [fr] "+v"(S.frags), [zmax] "+v"(S.zmax)
                    : [z] "v"(z));
                if (KIND == TRGL_SHADER_PHONG || KIND == TRGL_SHADER_EYE) {
                    asm volatile("v_mov_b32 %0, %1" : "+v"(S.id) : "v"(id));                    // (the colour comes from k_shade)
                } else {
                    const uint32_t ncol = (!DEFERRED || id == 0xffffffffu) ? color : S.color;   // :192 (tgaimage.cpp:32-39 at block-out)
                    asm volatile("v_mov_b32 %0, %1" : "+v"(S.color) : "v"(ncol));
                    if (DEFERRED) asm volatile("v_mov_b32 %0, %1" : "+v"(S.id) : "v"(id));
                }
                TRGL_DBG(8, 1);
                // std::min / std::max keep the first of equal values and +0.0 == -0.0: when the z range ends in a zero its sign is that
                // of the first zero written in the reference's order (triangle, x, y), see DevStats
                if (z == 0.0 && !zero_locked) {
                    const uint32_t xy = __builtin_bit_cast(uint32_t, S.xy);
                    unsigned long long order = ((unsigned long long)S.ptri << 32) | ((unsigned long long)(xy & 0xffffu) << 16) | (unsigned long long)(xy >> 16);
                    atomicMin(__builtin_signbit(z) ? &stats->zero_neg_key : &stats->zero_pos_key, order);
                }
            }
        }
    }
#if defined(TRGL_DEBUG_COUNTERS) && !defined(TRGL_DEBUG_NOSTAMP)
    S.dbg[14] += __builtin_amdgcn_s_memtime() - t_res;
#endif
}

#ifndef TRGL_RASTER_WAVES
#define TRGL_RASTER_WAVES 5        // waves per SIMD the register allocation of k_raster aims at (96 vector registers; 6 waves = 80 registers spill 8 dwords per list step: 2 % slower)
#endif

// BPP: the framebuffer's bytes per pixel when the kernel is compiled for one (3 or 4, FLAT only), 0 = read from FrameParams
// ALLWS: the flush holds no triangle that needs the literal path (k_setup counted them): the kernel is compiled without it
// DEFERRED: the flush has PHONG / EYE draws (visibility buffer + k_shade)
template <int KIND, int BPP = 0, bool ALLWS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TRGL_RASTER_WAVES, 8))) void k_raster(FrameParams fp, const TriRec* __restrict__ recs, const TriW* __restrict__ recs_w,
                                                const uint32_t* __restrict__ vals, const uint16_t* __restrict__ bmask,
                                                const uint32_t* __restrict__ tile_start,
                                                const uint32_t* __restrict__ tile_end,
                                                const DrawDesc* __restrict__ draws, DevStats* __restrict__ stats,
                                                const uint4* __restrict__ items, const uint32_t* __restrict__ n_items,
                                                unsigned long long* __restrict__ item_stats) {
    constexpr bool DEFERRED = KIND == TRGL_SHADER_PHONG || KIND == TRGL_SHADER_EYE || KIND == KIND_ANY;
    __shared__ uint32_t s_ring[4][RING];
    __shared__ uint32_t s_out[4][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t g;                                           // this workgroup's item (work_items.h: an eighth of the list per XCD)
    if (!trgl_item_of_workgroup(blockIdx.x, n_items[0], &g)) return;   // (block-uniform, like the clear-only exit below: the one barrier at the end is safe)
    const uint4 item4 = items[g];                         // work item, its tile's slice [beg, end) of the sorted pair list
    const uint32_t item = item4.x;
    const int t = (int)trgl_item_tile(item);
    const int tile_y = t / fp.tiles_x, tile_x = t - tile_y * fp.tiles_x;
    const int px0 = tile_x << TRGL_TILE_LOG2, py0 = tile_y << TRGL_TILE_LOG2;
    unsigned long long* my_stats = item_stats + (size_t)g * TRGL_ITEM_STATS_WORDS;
    if (item & TRGL_ITEM_CLEAR) {                         // cleared and empty: store the clear values, nothing else
        // rows [py0 + 8 w, py0 + 8 w + 7] of the tile for wave w
        const int ya = max(py0 + 8 * w, fp.strip_y0), yb = min(min(py0 + 8 * w + 7, fp.H - 1), fp.strip_y1 - 1);
        if (ya <= yb) clear_rows(fp, lane, px0, ya, yb);
        if (threadIdx.x == 0) trgl_item_stats_store(my_stats, 0ull, TRGL_ITEM_KMIN_NONE, TRGL_ITEM_KMAX_NONE);
        return;
    }
    const int brow = (int)trgl_item_brow(item);
    const int kblk = 4 * brow + w;                        // this wave's block of the tile: bit 4 cy + cx of the pair masks
    const int X0 = px0 + 8 * w, Y0 = py0 + 8 * brow;

    BlockState S;
    const int lx = X0 + (lane & 7), ly = Y0 + (lane >> 3);          // the lane's pixel
    S.xy = __builtin_bit_cast(us2, (uint32_t)lx | ((uint32_t)ly << 16));
    const bool owned = lx < fp.W && ly < fp.H && ly >= fp.strip_y0 && ly < fp.strip_y1;
    const size_t pix = (size_t)lx + (size_t)ly * fp.W;
    S.pxc = (double)lx + 0.5; S.pyc = (double)ly + 0.5;
    // Pixels of the block that this context does not own (rows outside the strip, beyond the image) hold -inf: no fragment
    // passes there, and they are not stored.
    S.z = -__builtin_inf();
    if (owned) S.z = fp.init_from_clear ? fp.clear_z : fp.zb[pix];
    S.color = fp.clear_color;
    S.id = 0xffffffffu;
    S.pux = 0.0; S.puy = 0.0; S.ptri = 0;
    S.puz = -1.0; S.pruz = -1.0; S.pz0 = 0.0; S.pz1 = 0.0; S.pz2 = 0.0; S.pcd = 0;
    S.frags = 0; S.zmax = -__builtin_inf();
    const bool zero_locked = stats->zero_locked != 0;
#ifdef TRGL_DEBUG_COUNTERS
    for (int k = 0; k < 16; ++k) S.dbg[k] = 0;
    S.t_prev = __builtin_amdgcn_s_memtime();
#endif
    unsigned long long pend = 0;                          // lanes that hold a deferred fragment (wave-uniform)

    const uint32_t beg = item4.y, end = item4.z;
    uint32_t* ring = s_ring[w];
    uint32_t head = 0, cnt = 0;                           // ring: `cnt` candidates wait from position `head` on
    // The list, 256 entries per step: lane l takes entries 4 l .. 4 l + 3 of the step (one 16-byte load of triangle ids, one 8-byte
    // load of block masks; steps start at a multiple of 4 entries, the pair buffers hold a multiple of 4).  The entries of the next
    // step are requested before the candidates of this one are processed.  Loads without a branch around them (clamped index, masks
    // cleared outside [beg, end)), so that the wait for THIS step's entries can leave the next step's loads in flight.
    // the round whose gather is in flight: its candidates (lane = candidate), how many, and chunks 0-4 and 7 of their records
    uint32_t pn = 0, ptri = 0;
    double2 pq0 = make_double2(0, 0), pq1 = pq0, pq2 = pq0, pq3 = pq0, pq4 = pq0;
    uint4 pq5 = make_uint4(0, 0, 0, 0);
    // ---- visits: the survivors in list order, constants through the scalar cache one visit ahead -------------------
    // One visit = our_gl.cpp:147-152 for one triangle on this block, one pixel per lane, up to the coverage decision.
    auto visit = [&](const TriScan& T, uint32_t tcur) {
        // the lanes of `m` note (u.x, u.y, triangle): moves under the mask, in place
        auto note = [&](unsigned long long m, double ux, double uy) {
            unsigned long long sv;
            asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m]\n\tv_mov_b64 %[px], %[ux]\n\tv_mov_b64 %[py], %[uy]\n\t"
                         "v_mov_b32 %[pt], %[t]\n\tv_mov_b64 %[puz], %[uz]\n\tv_mov_b64 %[pruz], %[ruz]\n\t"
                         "v_mov_b64 %[pz0], %[z0]\n\tv_mov_b64 %[pz1], %[z1]\n\tv_mov_b64 %[pz2], %[z2]\n\tv_mov_b32 %[pcd], %[cd]\n\ts_mov_b64 exec, %[sv]"
                         : [px] "+v"(S.pux), [py] "+v"(S.puy), [pt] "+v"(S.ptri), [sv] "=&s"(sv),
                           [puz] "+v"(S.puz), [pruz] "+v"(S.pruz), [pz0] "+v"(S.pz0), [pz1] "+v"(S.pz1), [pz2] "+v"(S.pz2), [pcd] "+v"(S.pcd)
                         : [ux] "v"(ux), [uy] "v"(uy), [t] "s"(tcur), [m] "s"(m), [cd] "s"(KIND == TRGL_SHADER_FLAT ? T.color : T.dl),
                           [uz] "s"(T.uz), [ruz] "s"(T.ruz), [z0] "s"(T.z0), [z1] "s"(T.z1), [z2] "s"(T.z2));
        };
        double ux, uy;
        unsigned long long cm;                    // lanes with a covered pixel that can still win the z-test (wave-uniform)
        unsigned long long both, sv, sx;          // ... that still hold a fragment of an earlier triangle; scratch
#ifdef TRGL_DEBUG_COUNTERS
        unsigned long long am = 0;
#endif
        const uint32_t ext = T.by - T.bx;         // (hi >= lo in both 16-bit halves: no borrow)
        if (ALLWS || !(T.dl & TRGL_DL_LITERAL)) {
            // The core of a visit is written out instruction by instruction: 16 vector instructions, straight-line
            // but for two exits.  (From C++ the compiler builds it with exec-mask regions: zero-initialised phi registers,
            // save / restore pairs and a mask -> vector -> mask round trip for the ballot: ~30 vector + ~25 scalar.)  Every
            // vector instruction issues for all 64 lanes whether they matter or not, so nothing is masked: lanes outside
            // (bbox n block), hidden lanes and uncovered lanes only drop out of the final mask.
            //   NO test of the lane's pixel against the triangle's bbox (our_gl.cpp:130-133 only visits bbox pixels): a pixel centre
            //     outside floor(min) .. ceil(max) is at least half a pixel away from the triangle, and k_setup sends every triangle
            //     for which the roundings of u could bridge that (2^-40 S^2 R >= |u.z|) down the literal path below, which keeps the
            //     test.  Pixels beyond the image or outside the strip hold -inf and fail the depth comparison.
            //   barycentric(), our_gl.cpp:77-86: s0z = ax - x, s1z = ay - y (s0.xy, s1.xy and u.z hoisted into the record)
            //   depth first: zpl = fma(s0z, g1, fma(s1z, g2, c0)); a pixel with zpl >= its stored depth fails the z-test whatever
            //     its coverage (k_setup); NaN reads as keep.  No lane left: the visit ends here.
            //   u.x = s0y s1z - s0z s1y (geometry.h:145), u.y = s0z s1x - s0x s1z (:146), us = u.x + u.y, every product and sum
            //     rounded on its own as in the reference
            //   covered <=> !(us < u.z) && !(u.y > 0) && !(u.x > 0): u.z < 0 and nothing can over/underflow, so the signs of the
            //     quotients of :85 are known without dividing ("exactness"); max(u.x, u.y) > 0 <=> one of them is.
            double s0z, s1z, ta, tb2;
#ifdef TRGL_DEBUG_COUNTERS
            am = __ballot(__builtin_bit_cast(uint32_t, __builtin_elementwise_max(S.xy - __builtin_bit_cast(us2, T.bx), __builtin_bit_cast(us2, ext))) == ext);
#endif
            // (`asm goto` would let the exits of this block skip the test of `both` behind it; this compiler's AMDGPU back end
            // loses the block's contents when it has branch targets outside, so the exits set both = 0 and fall out.)
            asm volatile(
                "v_add_f64 %[s0z], %[ax], -%[pxc]\n\t"
                "v_add_f64 %[s1z], %[ay], -%[pyc]\n\t"
                "v_mov_b64 %[ta], %[c0]\n\t"
                "v_fmac_f64 %[ta], %[g2], %[s1z]\n\t"
                "v_fmac_f64 %[ta], %[g1], %[s0z]\n\t"
                "v_cmp_nge_f64_e32 vcc, %[ta], %[z]\n\t"
#ifdef TRGL_DEBUG_COUNTERS
                "s_mov_b64 %[cm], 0\n\t"
#endif
                "s_cbranch_vccz .Lvisit_end%=\n\t"
                "v_mul_f64 %[ta], %[s0y], %[s1z]\n\t"
                "v_mul_f64 %[tb], %[s1y], %[s0z]\n\t"
                "v_add_f64 %[ux], %[ta], -%[tb]\n\t"
                "v_mul_f64 %[ta], %[s1x], %[s0z]\n\t"
                "v_mul_f64 %[tb], %[s0x], %[s1z]\n\t"
                "v_add_f64 %[uy], %[ta], -%[tb]\n\t"
                "v_add_f64 %[ta], %[ux], %[uy]\n\t"
                "v_max_f64 %[tb], %[ux], %[uy]\n\t"
                "v_cmp_nlt_f64_e64 %[cm], %[ta], %[uz]\n\t"
                "s_and_b64 %[cm], %[cm], vcc\n\t"
                "v_cmp_nlt_f64_e32 vcc, 0, %[tb]\n\t"
                "s_and_b64 %[cm], %[cm], vcc\n\t"
                "s_cbranch_scc0 .Lvisit_end%=\n\t"
                // covered lanes: those that hold no fragment note (u.x, u.y, triangle) at once, in place (moves under the mask);
                // `both` = the covered lanes that still hold one (the code behind the block resolves first, then notes theirs)
                "s_andn2_b64 %[sv], %[cm], %[pend]\n\t"
                "s_cbranch_scc0 .Lvisit_noted%=\n\t"
                "s_mov_b64 %[sx], exec\n\t"
                "s_mov_b64 exec, %[sv]\n\t"
                "v_mov_b64 %[pux], %[ux]\n\t"
                "v_mov_b64 %[puy], %[uy]\n\t"
                "v_mov_b32 %[ptri], %[tcur]\n\t"
                "v_mov_b64 %[puz], %[uz]\n\t"
                "v_mov_b64 %[pruz], %[ruz]\n\t"
                "v_mov_b64 %[pz0], %[z0]\n\t"
                "v_mov_b64 %[pz1], %[z1]\n\t"
                "v_mov_b64 %[pz2], %[z2]\n\t"
                "v_mov_b32 %[pcd], %[cd]\n\t"
                "s_mov_b64 exec, %[sx]\n"
                ".Lvisit_noted%=:\n\t"
                "s_or_b64 %[pend], %[pend], %[cm]\n\t"
                "s_xor_b64 %[both], %[cm], %[sv]\n\t"
                "s_branch .Lvisit_done%=\n"
                ".Lvisit_end%=:\n\t"
                "s_mov_b64 %[both], 0\n"
                ".Lvisit_done%=:"
                : [cm] "=&s"(cm), [ux] "=&v"(ux), [uy] "=&v"(uy), [s0z] "=&v"(s0z), [s1z] "=&v"(s1z), [ta] "=&v"(ta), [tb] "=&v"(tb2),
                  [both] "=&s"(both), [sv] "=&s"(sv), [sx] "=&s"(sx), [pend] "+s"(pend), [pux] "+v"(S.pux), [puy] "+v"(S.puy), [ptri] "+v"(S.ptri),
                  [puz] "+v"(S.puz), [pruz] "+v"(S.pruz), [pz0] "+v"(S.pz0), [pz1] "+v"(S.pz1), [pz2] "+v"(S.pz2), [pcd] "+v"(S.pcd)
                : [pxc] "v"(S.pxc), [pyc] "v"(S.pyc), [z] "v"(S.z), [tcur] "s"(tcur),
                  [ax] "s"(T.ax), [ay] "s"(T.ay), [c0] "s"(T.c0), [g1] "s"(T.g1), [g2] "s"(T.g2),
                  [s0x] "s"(T.s0x), [s0y] "s"(T.s0y), [s1x] "s"(T.s1x), [s1y] "s"(T.s1y), [uz] "s"(T.uz),
                  [ruz] "s"(T.ruz), [z0] "s"(T.z0), [z1] "s"(T.z1), [z2] "s"(T.z2), [cd] "s"(KIND == TRGL_SHADER_FLAT ? T.color : T.dl)
                : "vcc", "scc");
        } else {
            // a triangle that is not well scaled: the same visit from C++, coverage from the literal quotients of :85
            const us2 off = S.xy - __builtin_bit_cast(us2, T.bx);
            const bool act = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(off, __builtin_bit_cast(us2, ext))) == ext;
            const double s0z = T.ax - S.pxc, s1z = T.ay - S.pyc;
            const double zpl = __builtin_fma(s0z, T.g1, __builtin_fma(s1z, T.g2, T.c0));
            ux = T.s0y * s1z - s0z * T.s1y;                               // geometry.h:145
            uy = s0z * T.s1x - T.s0x * s1z;                               // geometry.h:146
            const double us = ux + uy;
            const double b0 = 1.0 - us / T.uz, b1 = uy / T.uz, b2 = ux / T.uz;      // :85, as written
            cm = __ballot(act && !(zpl >= S.z) && !(b0 < 0 || b1 < 0 || b2 < 0));  // :152
#ifdef TRGL_DEBUG_COUNTERS
            am = __ballot(act);
#endif
            both = cm & pend;
            note(cm & ~pend, ux, uy);
            pend |= cm;
        }
        TRGL_DBG(2, tcur < fp.n_tris ? 1 : 0); TRGL_DBG(3, __popcll(am)); TRGL_DBG(4, cm ? 1 : 0); TRGL_DBG(5, __popcll(cm));
        if (both) {
            // Some covered lanes still hold a fragment of an earlier triangle, which has to be resolved first (submission
            // order per pixel).  Everything that can go goes in that one pass: the old fragments of all noted lanes AND the
            // new ones of the lanes that held none (`pend` holds them already); only the conflicting lanes' new fragments
            // stay noted afterwards.
            resolve<KIND, ALLWS, DEFERRED>(S, pend, recs, recs_w, draws, stats, zero_locked);
            note(both, ux, uy);
            asm volatile("s_mov_b64 %0, %1" : "+s"(pend) : "s"(both));      // pend = both, in the register that holds it
        }
    };
    const uint32_t p_first = beg & ~3u;
    auto load_step = [&](uint32_t p0, uint4& tri4, uint2& m) {
        const uint32_t pl = p0 + 4u * (uint32_t)lane, p = min(pl, (end - 1u) & ~3u);
        tri4 = *reinterpret_cast<const uint4*>(vals + p);
        m = *reinterpret_cast<const uint2*>(bmask + p);
    };
    uint4 tri_n = make_uint4(0, 0, 0, 0); uint2 m_n = make_uint2(0, 0);
    if (beg < end) load_step(p_first, tri_n, m_n);
    for (uint32_t p0 = p_first; p0 < end; p0 += 256) {
        const uint4 tri_c = tri_n; const uint2 m_c = m_n;
        TRGL_STAMP(10);            // startup (first step) / whatever is left between the stamps below
        load_step(p0 + 256, tri_n, m_n);                  // (past the end: clamped index; its entries are never looked at)
        // append the step's candidates to the ring in list order: entry 4 l + j comes after every entry of the lanes below l
        {
            // c_j: entry 4 l + j of the step reaches this wave's block (bit kblk of its mask) ...
            uint32_t c0 = (m_c.x >> kblk) & 1u, c1 = (m_c.x >> (16 + kblk)) & 1u, c2 = (m_c.y >> kblk) & 1u, c3 = (m_c.y >> (16 + kblk)) & 1u;
            if (p0 < beg || p0 + 256u > end) {
                // ... and lies in [beg, end): only the first and the last step of a list hold entries that do not.  Valid entries of
                // the lane: [lo, hi).  (Written without a wrapping subtraction under a select: `pl < end ? min(end - pl, 4) : 0` reached
                // the ISA as a saturating 4 - (end - pl), which takes every lane PAST the end for fully valid - lists shorter than a
                // step then appended whatever followed them in the pair buffer, stale words of an earlier flush included;
                // profiles/one_case.py with the diagnostic build found it.)
                const uint32_t pl = p0 + 4u * (uint32_t)lane;
                const uint32_t lo = min(beg - min(pl, beg), 4u), hi = min(end - min(pl, end), 4u);
                const uint32_t v = (0xfu << lo) & (0xfu >> (4u - hi));
                c0 &= v; c1 &= v >> 1; c2 &= v >> 2; c3 &= v >> 3;
            }
            if (fp.zq_cull) {
                // The flush holds large triangles: an entry whose depth bound (7 bits in its triangle word, k_setup) is not below the
                // block's largest stored depth cannot put a fragment into this block - it never becomes a candidate.  qb: the depth
                // rounded UP to the bound's grid (a float rounded up, then 2^-10 of a step more for the roundings here; 128 = nothing
                // stored yet).  Occluded triangles of frames with a high depth complexity die here, 256 entries per step, without
                // their records being touched.
                const float zmb = wave_max_f32(f32_up(S.z));
                const float tq = (zmb + 1.0f) * 64.0f + 0x1p-10f;
                const uint32_t qb = !(tq < 128.0f) ? 128u : (tq <= 1.0f ? 1u : (uint32_t)__builtin_ceilf(tq));      // (>= 1: zq = 0 says nothing)
                c0 = TRGL_VAL_ZQ(tri_c.x) < qb ? c0 : 0u; c1 = TRGL_VAL_ZQ(tri_c.y) < qb ? c1 : 0u;
                c2 = TRGL_VAL_ZQ(tri_c.z) < qb ? c2 : 0u; c3 = TRGL_VAL_ZQ(tri_c.w) < qb ? c3 : 0u;
            }
            const unsigned long long b0 = __ballot(c0), b1 = __ballot(c1), b2 = __ballot(c2), b3 = __ballot(c3);
            if (b0 | b1 | b2 | b3) {
                uint32_t pos = head + cnt;
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u));
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b2, 0u));
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(b3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b3, 0u));
                if (c0) ring[pos & (RING - 1)] = tri_c.x;
                pos += c0;
                if (c1) ring[pos & (RING - 1)] = tri_c.y;
                pos += c1;
                if (c2) ring[pos & (RING - 1)] = tri_c.z;
                pos += c2;
                if (c3) ring[pos & (RING - 1)] = tri_c.w;
#ifdef TRGL_DEBUG_COUNTERS
                {   // a candidate that is no triangle of the flush: remember where the first one came from
                    const uint32_t trs[4] = { tri_c.x, tri_c.y, tri_c.z, tri_c.w };
                    const uint32_t cs[4] = { c0, c1, c2, c3 };
                    for (int j = 0; j < 4; ++j)
                        if (cs[j] && TRGL_VAL_TRI(trs[j]) >= fp.n_tris && atomicCAS(&stats->dbg[10], 0ull, 1ull) == 0ull) {
                            stats->dbg[11] = ((unsigned long long)(p0 + 4u * (uint32_t)lane + (uint32_t)j) << 32) | trs[j];
                            stats->dbg[12] = ((unsigned long long)beg << 32) | end;
                            stats->dbg[13] = ((unsigned long long)(uint32_t)t << 32) | (uint32_t)kblk;
                        }
                }
#endif
                const uint32_t added = (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
                cnt += added;
                TRGL_DBG(0, added);
            }
        }
        const bool last = p0 + 256 >= end;
        TRGL_STAMP(11);            // list step: wait for its entries, append the candidates
        // Rounds of up to 64 candidates, two in the pipe: the gather of round k + 1 is REQUESTED between the test of round k and the
        // visits of its survivors, so that it flies under them; its test follows the visits and sees the depths they left.  A
        // requested round also stays in flight over a list step when the ring cannot start the one after it yet.
        for (;;) {
            const bool can = cnt >= 64 || (last && cnt);
            bool keep = false;
            if (pn) {
                if (!can && !last) break;
            // ---- cull: lane = candidate ------------------------------------------------------------------------------
                // largest stored depth of the block (deferred fragments only lower depths later: a stale maximum stays a bound;
                // a pixel holding NaN can never be written again, v_max skips it)
                // (as a float rounded up: six v_max_f32 with DPP / permlane operands instead of 64-bit shuffles through LDS)
                const double zmaxb = (double)wave_max_f32(f32_up(S.z));
                keep = (uint32_t)lane < pn;
#ifdef TRGL_DEBUG_COUNTERS
                if (keep && ptri >= fp.n_tris) { atomicAdd(&stats->dbg[9], 1ull); keep = false; }      // must stay 0: a list entry that is no triangle
#endif
                if (keep) {
                    const double2 q0 = pq0, q1 = pq1, q2 = pq2, q3 = pq3, q4 = pq4;
                    const uint4 q5 = pq5;
                    if (ALLWS || !(q5.w & TRGL_DL_LITERAL)) {
                        const double ax = q0.x, ay = q0.y, s0x = q1.x, s0y = q1.y, s1x = q2.x, s1y = q2.y, c0 = q3.x, uz = q3.y, g1 = q4.x, g2 = q4.y;
                        // pixel centres of (bbox n block): the rectangle with centre (xm, ym) and half-widths (xh, yh)
                        const int bx0 = (int)(q5.x & 0xffffu), by0 = (int)(q5.x >> 16), bx1 = (int)(q5.y & 0xffffu), by1 = (int)(q5.y >> 16);
                        const int xl = max(bx0, X0), xr = min(bx1, X0 + 7), yl = max(by0, Y0), yr = min(by1, Y0 + 7);
                        const double xm = __builtin_fma((double)(xl + xr), 0.5, 0.5), xh = (double)(xr - xl) * 0.5;
                        const double ym = __builtin_fma((double)(yl + yr), 0.5, 0.5), yh = (double)(yr - yl) * 0.5;
                        const double dxm = ax - xm, dym = ay - ym;
                        // (edge)  a pixel is covered iff the rounded u.x <= 0, u.y <= 0 and u.x + u.y >= u.z (the sign form of :152).
                        // Each is affine in the pixel centre: over the rectangle it stays within (sum of |gradient| x half-width) of its
                        // value at the centre, and the value computed THERE (with the operations of the scan) differs from what the
                        // scan computes at a pixel by that affine change + at most 2^-51 (sum of |products|) <= 2^-51 Sa R:
                        // margins of 2^-40 of the same magnitudes.  (No corner is selected: a select of a double is two instructions.)
                        const double uxc = s0y * dym - dxm * s1y;                                             // u.x at the centre
                        const double uyc = dxm * s1x - s0x * dym;                                             // u.y
                        const double gx = s1y - s1x, gy = s0x - s0y;                                           // gradient of u.x + u.y
                        const double sp1 = __builtin_fma(fabs(s1y), xh, fabs(s0y) * yh);                      // how far u.x can fall below uxc
                        const double sp2 = __builtin_fma(fabs(s1x), xh, fabs(s0x) * yh);                      // ... u.y below uyc
                        const double sp3 = __builtin_fma(fabs(gx), xh, fabs(gy) * yh);                        // ... u.x + u.y rise above uxc + uyc
                        const double R = ((fabs(dxm) + xh) + (fabs(dym) + yh)) + 16.0;                       // >= |A - pixel| (L1) on the rectangle
                        const double ma = 0x1p-40 * ((fabs(s0y) + fabs(s1y)) * R) + 0x1p-1000;
                        const double mb = 0x1p-40 * ((fabs(s0x) + fabs(s1x)) * R) + 0x1p-1000;
                        // (depth)  every covered pixel's z is above the plane c0 + (ax - x) g1 + (ay - y) g2 (k_setup), whose minimum
                        // over the rectangle is its value at the centre minus (|g1| xh + |g2| yh); if even that is not below the block's
                        // largest stored depth, no pixel of the block passes the strict `<` of :165.  NaN compares false = keep.
                        // The plane reaches below the triangle's own depths outside the triangle; a covered pixel also has b_i >= 0 and
                        // b0 + b1 + b2 = 1 +- 2^-50, hence z >= min(z0, z1, z2) - 2^-40 max|z_i|, and the plane's values AT the three vertices
                        // A, A + (s0y, s1y), A + (s0x, s1x) are z_i minus k_setup's margin (>= 2^-39 max|z_i| (R S/|u.z| + 1) with R >= S, which
                        // also covers the roundings of these evaluations): their minimum is below that bound.  The larger of the two
                        // lower bounds counts.
                        const double zpl = __builtin_fma(dxm, g1, __builtin_fma(dym, g2, c0)) - __builtin_fma(fabs(g1), xh, fabs(g2) * yh);
                        const double zv = vmin(vmin(c0, __builtin_fma(-s0y, g1, __builtin_fma(-s1y, g2, c0))), __builtin_fma(-s0x, g1, __builtin_fma(-s1x, g2, c0)));
                        if (uxc - sp1 > ma || uyc - sp2 > mb || (uxc + uyc) + sp3 < uz - (ma + mb) || vmax(zpl, zv) >= zmaxb) keep = false;
                    }
                }
            } else if (!can) break;
            const unsigned long long surv = __ballot(keep);
            const uint32_t tri = ptri;                   // the tested round's candidates (the survivors among them are visited below)
            TRGL_DBG(1, __popcll(surv));
            TRGL_STAMP(12);        // cull round (tests)
            if (can) {
                const uint32_t n = cnt < 64 ? cnt : 64;
                __builtin_amdgcn_wave_barrier();
                ptri = TRGL_VAL_TRI(ring[(head + lane) & (RING - 1)]);
                __builtin_amdgcn_wave_barrier();
                head += n; cnt -= n; pn = n;
                if ((uint32_t)lane < n
#ifdef TRGL_DEBUG_COUNTERS
                    && ptri < fp.n_tris
#endif
                    ) {
                    const double2* q = reinterpret_cast<const double2*>(recs + ptri);
                    pq0 = q[0]; pq1 = q[1]; pq2 = q[2]; pq3 = q[3]; pq4 = q[4];
                    pq5 = reinterpret_cast<const uint4*>(q)[7];
                }
            } else pn = 0;
            if (surv) {
                // The survivors move to lanes 0 .. ns - 1 (through LDS, order kept), so that the visit loop counts instead of peeling bits
                // off a 64-bit mask: 2 scalar instructions per visit instead of 8 - the scalar unit, one instruction per cycle for the
                // whole CU, is as busy in this kernel as the vector units.
                const uint32_t ns = (uint32_t)__popcll(surv);
                uint32_t* comp = s_out[w];
                if (keep) comp[__builtin_amdgcn_mbcnt_hi((uint32_t)(surv >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)surv, 0u))] = tri;
                __builtin_amdgcn_wave_barrier();
                uint32_t tri_s = comp[lane];
                // The lanes behind them name the record behind the flush's last one (k_make_items): the loop below runs in PAIRS of visits -
                // one counter update and one exit test per pair - and the partner of an odd last survivor is that record, whose
                // visit ends at its first test.
                if ((uint32_t)lane >= ns) tri_s = fp.n_tris;
                // Two sets of constants, A and B, take turns (no register copies): while a visit works on one, the request for
                // the next survivor's record fills the other.  The wait for a set sits behind the visit that ran under its request.
                // (The last request of a round names lane ns + 1 or, behind lane 63, lane 0 or 1: valid addresses, nobody reads the result.)
                uint32_t i = 0;
                uint32_t ta = (uint32_t)__builtin_amdgcn_readlane((int)tri_s, 0), tb;
                TriScan A = load_scan(recs, ta), B;
                scan_wait(A);                        // the first triangle's constants are waited for HERE, not behind the first request inside the loop
                do {
                    tb = (uint32_t)__builtin_amdgcn_readlane((int)tri_s, (int)(i + 1u));
                    B = load_scan(recs, tb);
                    __builtin_amdgcn_sched_barrier(0);
                    visit(A, ta);
                    __builtin_amdgcn_sched_barrier(0);
                    scan_wait(B);
                    ta = (uint32_t)__builtin_amdgcn_readlane((int)tri_s, (int)(i + 2u));
                    A = load_scan(recs, ta);
                    __builtin_amdgcn_sched_barrier(0);
                    visit(B, tb);
                    __builtin_amdgcn_sched_barrier(0);
                    scan_wait(A);
                    i += 2;
                } while (i < ns);
            }
            TRGL_STAMP(13);        // visits of the round (resolves included; their own clock is counter 14)
        }
    }
    if (pend) resolve<KIND, ALLWS, DEFERRED>(S, pend, recs, recs_w, draws, stats, zero_locked);

    TRGL_STAMP(13);
    // ---- block out: every owned pixel once ---------------------------------------------------------------------------
    // depth: 8 B per lane, a row of the block is 64 contiguous bytes
    if (owned) __builtin_nontemporal_store(S.z, &fp.zb[pix]);
    if (DEFERRED && fp.idbuf && owned) fp.idbuf[pix] = S.id;
    {
        const int bpp = BPP ? BPP : fp.bpp;
        const bool whole = fp.init_from_clear && X0 + 7 < fp.W;      // every pixel of an owned row is written: rows as dwords
        if (bpp == 4) {
            if (owned && (fp.init_from_clear || S.frags)) *reinterpret_cast<uint32_t*>(fp.fb + pix * 4) = S.color;
        } else if (bpp == 3 && whole) {
            // a row of the block is 24 B = 6 dwords: lanes 8 r + 0..5 assemble them from the row's 8 colours (through LDS)
            uint32_t* so = s_out[w];
            so[lane] = S.color;
            __builtin_amdgcn_wave_barrier();
            const int r = lane >> 3, dw = lane & 7;
            if (dw < 6) {
                const int y = Y0 + r;
                if (y < fp.H && y >= fp.strip_y0 && y < fp.strip_y1) {
                    // bytes 4 dw .. 4 dw + 3 of the row: pixel (4 dw + i) / 3, channel (4 dw + i) % 3
                    const int p0 = (4 * dw) / 3, sh = (4 * dw) % 3;
                    // (two pixels hold them: 3 - sh bytes of pixel p0, the rest of pixel p0 + 1 <= 7)
                    const uint32_t ca = so[8 * r + p0] & 0xffffffu, cb2 = so[8 * r + p0 + 1] & 0xffffffu;
                    const unsigned long long bytes = ((unsigned long long)ca | ((unsigned long long)cb2 << 24)) >> (8 * sh);
                    uint32_t* dst = reinterpret_cast<uint32_t*>(fp.fb + ((size_t)X0 + (size_t)y * fp.W) * 3) + dw;
                    *dst = (uint32_t)bytes;
                }
            }
        } else {
            if (owned && (fp.init_from_clear || S.frags)) {
                uint8_t* dst = fp.fb + pix * bpp;
                if (bpp == 3) { *reinterpret_cast<uint16_t*>(dst) = (uint16_t)S.color; dst[2] = (uint8_t)(S.color >> 16); }   // TGAImage::set: b, g, r
                else dst[0] = (uint8_t)S.color;
            }
        }
    }

    TRGL_STAMP(15);                // block out
    // ---- stats: our_gl.cpp:194-198, reduced per wave, then per workgroup: one partial per work item (k_fold_stats) ------
    // (std::min over the written depths of a pixel is its last one: the z-test only lets smaller ones through)
    // One reduction per WORKGROUP: every lane leaves its three values in its wave's candidate ring (done with by now), and behind the
    // kernel's only block-level barrier the first wave folds the four waves' values lane by lane and runs the butterflies once
    // (~100 vector + 30 LDS instructions that three of four waves no longer spend; three same-address LDS atomics per wave instead
    // cost 0.5 ms of k_raster - the LDS serialises the 64 lanes).
    {
        unsigned long long* red = reinterpret_cast<unsigned long long*>(ring);       // [0..63] smallest, [64..127] largest depth key, then the counts
        red[lane] = zkey(S.frags ? S.z : __builtin_inf());
        red[64 + lane] = zkey(S.zmax);
        ring[256 + lane] = S.frags;
    }
#ifdef TRGL_DEBUG_COUNTERS
    for (int o = 32; o; o >>= 1) S.dbg[8] += __shfl_xor(S.dbg[8], o);
    if (lane == 0) for (int k = 0; k < 16; ++k) if (S.dbg[k]) atomicAdd(&stats->dbg[k], S.dbg[k]);
#endif
    __syncthreads();                 // the only block-level barrier of the kernel, when every wave of the workgroup is done
    if (w == 0) {
        unsigned long long frags = 0, kmin = TRGL_ITEM_KMIN_NONE, kmax = TRGL_ITEM_KMAX_NONE;
        for (int k = 0; k < 4; ++k) {
            const unsigned long long* red = reinterpret_cast<const unsigned long long*>(s_ring[k]);
            const unsigned long long a = red[lane], b = red[64 + lane];
            frags += s_ring[k][256 + lane]; kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
        }
        for (int o = 32; o; o >>= 1) {                  // (one butterfly for the three: as three reductions in a row the kernel's instructions change)
            frags += __shfl_xor(frags, o);
            unsigned long long a = __shfl_xor(kmin, o); kmin = a < kmin ? a : kmin;
            unsigned long long b = __shfl_xor(kmax, o); kmax = b > kmax ? b : kmax;
        }
        if (lane == 0) trgl_item_stats_store(my_stats, frags, kmin, kmax);
    }
}

// ---------------------------------------------------------------------------------------------
// k_shade<PHONG|EYE>: the fragment stage of a PHONG / EYE flush, once per visible pixel.
// k_raster left, for every pixel whose depth it wrote in this flush, the record index of the LAST triangle that passed the
// z-test there (fp.idbuf).  IShader::fragment has no side effects and always returns discard = false (main.cpp:92-170,
// 220-261), so calling it for that triangle only gives the same framebuffer as calling it for every z-pass in order
// (our_gl.cpp:187-192) - with 64 busy lanes per wave instead of the few pixels of one small triangle.  One 256-thread
// block per work item of k_raster (so tiles this flush did not touch are not visited), one 8x8 block per wave; the
// barycentrics are recomputed per pixel with exactly the operations of the scan (same bits).  k_shade<KIND_ANY> leaves the
// pixels of user kinds alone: each user kind's own kernel (shade_user.h) shades them behind it.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_shade(FrameParams fp, const TriRec* __restrict__ recs, const TriW* __restrict__ recs_w,
                                                const DrawDesc* __restrict__ draws,
                                                const DevTexture* __restrict__ tex, const uint4* __restrict__ items,
                                                const uint32_t* __restrict__ n_items) {
    const int lane = threadIdx.x & 63;
    const uint32_t item_idx = blockIdx.x;                // one 256-thread block per work item: wave w shades block w of the item's row
    if (item_idx >= *n_items) return;
    const uint32_t item = items[item_idx].x;
    if (item & TRGL_ITEM_CLEAR) return;                  // no triangles: no owners
    const int t = (int)trgl_item_tile(item);
    const int tile_y = t / fp.tiles_x, tile_x = t - tile_y * fp.tiles_x;
    const int x = (tile_x << TRGL_TILE_LOG2) + 8 * (int)(threadIdx.x >> 6) + (lane & 7);
    const int y = (tile_y << TRGL_TILE_LOG2) + 8 * (int)trgl_item_brow(item) + (lane >> 3);
    const bool mine = x < fp.W && y < fp.H && y >= fp.strip_y0 && y < fp.strip_y1;
    const size_t idx = (size_t)x + (size_t)y * fp.W;
    // The kernel is bound by dependent memory latencies: owner -> record -> varyings -> texels.  The visibility buffer holds
    // `draw << 24 | triangle in its draw`, from which BOTH the record (recs[draw.first + triangle]) and the varyings are addressed:
    // two loads in flight instead of one after the other.
    const uint32_t dl = mine ? fp.idbuf[idx] : 0xffffffffu;
    if (dl == 0xffffffffu) return;
    // the draw (uniforms, varyings array, first record) is wave-uniform in all but exotic flushes: serve one draw at a time
    uint32_t color = 0;
    bool user = false;
    typedef const __attribute__((address_space(4))) DrawDesc CDrawK;
    unsigned long long todo = __ballot(true);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        const uint32_t di = (uint32_t)__builtin_amdgcn_readlane((int)(dl >> 24), src);
        const bool here = (dl >> 24) == di;
        todo &= ~__ballot(here);
        if (KIND == KIND_ANY && here && ((CDrawK*)draws)[di].kind >= TRGL_SHADER_USER_FIRST) {
            user = true;                                      // a user kind's pixel: its own kernel shades it (shade_user.h)
        } else if (here) {
            // descriptors through the CONSTANT address space: the draw index is wave-uniform, so every field (uniforms, texture
            // descriptors) comes in by scalar loads through the scalar cache.  As plain global loads they were vector loads, each
            // waited for on its own: ~20 memory round trips in a row per block, 68 % of the kernel's wave time in s_waitcnt.
            typedef const __attribute__((address_space(4))) DrawDesc CDraw;
            typedef const __attribute__((address_space(4))) DevTexture CTex;
            // (under `here` the compiler knows di == dl >> 24 and would address the draw per lane: re-derive it as a scalar)
            const uint32_t di_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dl >> 24));
            CDraw& d = ((CDraw*)draws)[di_s];
            CTex* const ctex = (CTex*)tex;
            const uint32_t local = dl & 0xffffffu;
            const TriRec& r = recs[d.first + local];
            const TriW& rw = recs_w[d.first + local];
            const double* vary = d.vary + (size_t)local * 24;
            double pc[3];
            TRGL_OWNER_BARYCENTRICS(r, rw, x, y, pc);                   // barycentric(), our_gl.cpp:77-86, as in k_raster
            const int kind = KIND == KIND_ANY ? d.kind : KIND;        // wave-uniform inside this iteration
            color = kind == TRGL_SHADER_PHONG ? frag_phong(d.u, ctex, vary, pc).bgra : frag_eye(d.u, ctex, vary, pc).bgra;
        }
    }
    if (KIND == KIND_ANY && user) return;
    store_pixel(fp, idx, color);                                   // TGAImage::set, tgaimage.cpp:32-39
}

}  // namespace

namespace trgl {

// a kernel compiled at run time (raster_user.h, shade_user.h), 256 threads per workgroup: its arguments by value, in its parameters' order
template <class... Args>
static void launch_user_kernel(hipFunction_t fn, uint32_t grid, hipStream_t s, Args... a) {
    void* args[] = { &a... };
    (void)hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, s, args, nullptr);
}

void launch_raster(hipStream_t s, const FrameParams& fp, int kind /* TRGL_SHADER_* if uniform over the flush, else -1 */, bool all_well_scaled,
                   const TriRec* recs, const TriW* recs_w, const uint32_t* vals, const uint16_t* bmask,
                   const uint32_t* tile_start, const uint32_t* tile_end, const DrawDesc* draws,
                   const DevTexture* tex, DevStats* stats, uint32_t max_items, uint4* items,
                   uint32_t* n_items, unsigned long long* item_stats, bool builtin_shade, const UserShade* user, int n_user,
                   hipFunction_t user_raster, hipEvent_t ev_before, hipEvent_t ev_after) {
    const int tiles = (fp.strip_ty1 - fp.strip_ty0) * fp.tiles_x;
    if (tiles <= 0 || max_items == 0) {          // a context that owns no rows (a rank beyond the image's bands): nothing to draw
        if (ev_before) (void)hipEventRecord(ev_before, s);
        if (ev_after) (void)hipEventRecord(ev_after, s);
        launch_fold_stats(s, stats, n_items, item_stats);     // n_items is 0: only resets the per-flush counts
        return;
    }
    launch_make_items(s, fp, tiles, tile_start, tile_end, items, n_items, const_cast<TriRec*>(recs));
    dim3 grid(trgl_item_grid(max_items));       // the raster kernels; the shade kernels take one workgroup per item (work_items.h)
    if (ev_before) (void)hipEventRecord(ev_before, s);
    if (user_raster) {                          // a flush of one user kind that may discard: its own raster kernel (raster_user.h)
        launch_user_kernel(user_raster, grid.x, s, fp, recs, recs_w, vals, bmask, draws, tex, stats, items, n_items, item_stats);
        if (ev_after) (void)hipEventRecord(ev_after, s);
        launch_fold_stats(s, stats, n_items, item_stats);
        return;
    }
#define TRGL_LAUNCH_RASTER(...) hipLaunchKernelGGL((k_raster<__VA_ARGS__>), grid, dim3(256), 0, s, fp, recs, recs_w, vals, bmask, tile_start, tile_end, draws, stats, items, n_items, item_stats)
    switch (kind) {
    case TRGL_SHADER_FLAT:
        if (all_well_scaled) {
            if (fp.bpp == 3) TRGL_LAUNCH_RASTER(TRGL_SHADER_FLAT, 3, true);
            else if (fp.bpp == 4) TRGL_LAUNCH_RASTER(TRGL_SHADER_FLAT, 4, true);
            else TRGL_LAUNCH_RASTER(TRGL_SHADER_FLAT, 0, true);
        } else {
            TRGL_LAUNCH_RASTER(TRGL_SHADER_FLAT);
        }
        break;
    case TRGL_SHADER_GOURAUD: if (all_well_scaled) TRGL_LAUNCH_RASTER(TRGL_SHADER_GOURAUD, 0, true); else TRGL_LAUNCH_RASTER(TRGL_SHADER_GOURAUD); break;
    case TRGL_SHADER_PHONG:   if (all_well_scaled) TRGL_LAUNCH_RASTER(TRGL_SHADER_PHONG, 0, true); else TRGL_LAUNCH_RASTER(TRGL_SHADER_PHONG); break;
    case TRGL_SHADER_EYE:     if (all_well_scaled) TRGL_LAUNCH_RASTER(TRGL_SHADER_EYE, 0, true); else TRGL_LAUNCH_RASTER(TRGL_SHADER_EYE); break;
    case TRGL_SHADER_CHECKER: TRGL_LAUNCH_RASTER(TRGL_SHADER_CHECKER); break;
    default:                  TRGL_LAUNCH_RASTER(KIND_ANY); break;
    }
#undef TRGL_LAUNCH_RASTER
    if (ev_after) (void)hipEventRecord(ev_after, s);
    if (fp.idbuf && builtin_shade) {                    // the flush has PHONG / EYE draws: shade the visible pixels they own
#define TRGL_LAUNCH_SHADE(K) hipLaunchKernelGGL(k_shade<K>, dim3(max_items), dim3(256), 0, s, fp, recs, recs_w, draws, tex, items, n_items)
        if (kind == TRGL_SHADER_PHONG) TRGL_LAUNCH_SHADE(TRGL_SHADER_PHONG);
        else if (kind == TRGL_SHADER_EYE) TRGL_LAUNCH_SHADE(TRGL_SHADER_EYE);
        else TRGL_LAUNCH_SHADE(KIND_ANY);
#undef TRGL_LAUNCH_SHADE
    }
    // ... and those of every user kind of the flush, one kernel each, over the same work items (before k_fold_stats clears their count)
    for (int i = 0; i < n_user && fp.idbuf; ++i) launch_user_kernel(user[i].fn, max_items, s, fp, recs, recs_w, draws, tex, items, n_items, user[i].kind);
    launch_fold_stats(s, stats, n_items, item_stats);
}

}  // namespace trgl
