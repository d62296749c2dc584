// raster_user.h — the raster kernel of a user kind that may discard (include/trgl.h, TRGL_SHADER_MAY_DISCARD), compiled by hiprtc
// behind the user's source, which defines `trgl_frag_out trgl_fragment(const trgl_frag_in&)`.
//
// Such a kind cannot be shaded once per visible pixel: a discarded fragment leaves the depth behind it in place, so the fragments
// that follow are tested against it (our_gl.cpp:187-188).  This kernel does for a flush of one such kind what k_raster
// (kernels_raster.hip) does for a CHECKER flush, in the plainest form: the same work items (k_make_items), the same sorted pair
// lists, the same item_stats partials for k_fold_stats behind it.  One 256-thread workgroup per work item, one 8x8 block per
// wave, one pixel per lane; the block's depths and colours stay in registers from the first candidate to the block-out.  Per
// candidate, in list order: the record's bbox test, barycentric() of our_gl.cpp:77-86 with exactly the operations of the scan, the
// coverage test on the quotients, the depth of :156-158, the finite check and the strict z-test, the perspective-correct
// barycentrics of :168-185 and then trgl_fragment - called for every fragment that passes the z-test, in submission order per
// pixel, exactly where our_gl.cpp:187 calls it.  The barycentrics and the correction are written out here, operation for operation
// the text of TRGL_OWNER_BARYCENTRICS (shade_common.h), not an expansion of it: the coverage test, the depth and the z-test stand
// between its two halves.  An edit to either copy belongs in both; tests/test_user_kind_raster_paths_gpu.py holds this one to the
// oracle on the literal and the fallback branch.  k_raster's accelerations (depth-plane cull, depth bound in the pair, deferred
// resolves) are left out: they only skip work, and nothing here depends on them.
//
// Two further flags of such a kind change this one text in straight lines (include/trgl.h, "User shaders that blend"); with both
// off the kernel is the one above, instruction for instruction.  TRGL_USER_READS_DEST: `color` is the pixel from the start (the
// clear colour, or the frame's bytes when the flush does not start from a clear) and its bpp low bytes go to trgl_fragment as
// in.dst.  TRGL_USER_DEPTH_WRITE 0: a drawn fragment skips our_gl.cpp:191, so `z` stays what the flush found and the smallest
// depth written is kept in a register of its own, as the largest is.
#pragma once
#include "user_prelude.h"

static_assert(__is_same(decltype(trgl_fragment(*(const trgl_frag_in*)nullptr)), trgl_frag_out),
              "registered with TRGL_SHADER_MAY_DISCARD: trgl_fragment must return trgl_frag_out { bool discard; uint32_t bgra; }");

extern "C" __global__ __launch_bounds__(256)
void trgl_raster_user(FrameParams fp, const TriRec* __restrict__ recs, const TriW* __restrict__ recs_w, const uint32_t* __restrict__ vals,
                      const uint16_t* __restrict__ bmask, const DrawDesc* __restrict__ draws, const DevTexture* __restrict__ tex,
                      DevStats* __restrict__ stats, const uint4* __restrict__ items,
                      const uint32_t* __restrict__ n_items, unsigned long long* __restrict__ item_stats) {
    typedef const __attribute__((address_space(4))) TriRec CRec;       // records and descriptors through the scalar cache
    typedef const __attribute__((address_space(4))) DrawDesc CDraw;
    typedef const __attribute__((address_space(4))) DevTexture CTex;
    __shared__ unsigned long long s_red[4][3];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t g;                                           // this workgroup's item: the mapping of k_raster (work_items.h)
    if (!trgl_item_of_workgroup(blockIdx.x, n_items[0], &g)) return;   // (workgroup-uniform: the barrier at the end is safe)
    const uint4 item4 = items[g];
    const uint32_t item = item4.x;
    const int t = (int)trgl_item_tile(item);
    const int tile_y = t / fp.tiles_x, tile_x = t - tile_y * fp.tiles_x;
    const int px0 = tile_x << TRGL_TILE_LOG2, py0 = tile_y << TRGL_TILE_LOG2;
    unsigned long long* my_stats = item_stats + (size_t)g * TRGL_ITEM_STATS_WORDS;
    if (item & TRGL_ITEM_CLEAR) {                         // cleared and empty: the clear values, as k_raster stores them
        const int ya = max(py0 + 8 * w, fp.strip_y0), yb = min(min(py0 + 8 * w + 7, fp.H - 1), fp.strip_y1 - 1);
        if (ya <= yb) trgl_shade::clear_rows(fp, lane, px0, ya, yb);
        if (threadIdx.x == 0) trgl_item_stats_store(my_stats, 0ull, TRGL_ITEM_KMIN_NONE, TRGL_ITEM_KMAX_NONE);
        return;
    }
    const int brow = (int)trgl_item_brow(item);
    const int kblk = 4 * brow + w;                        // this wave's block of the tile: bit 4 cy + cx of the pair masks
    const int X0 = px0 + 8 * w, Y0 = py0 + 8 * brow;
    const int x = X0 + (lane & 7), y = Y0 + (lane >> 3);
    // k_make_items gives items to owned tile rows only; inside them, rows outside the strip and pixels beyond the image hold -inf
    // (no fragment passes there) and are not stored
    const bool owned = x < fp.W && y < fp.H && y >= fp.strip_y0 && y < fp.strip_y1;
    const size_t pix = (size_t)x + (size_t)y * fp.W;
    double z = -__builtin_inf();
    if (owned) z = fp.init_from_clear ? fp.clear_z : fp.zb[pix];
    uint32_t color = fp.clear_color;
#if TRGL_USER_READS_DEST
    // TGAImage::get (tgaimage.cpp:24-30): the pixel's bpp bytes, the rest of the TGAColor zero.  `color` holds 32 bits of which bpp
    // bytes are the frame (a fragment's alpha never reaches a 3-byte frame), so in.dst is masked wherever it is formed
    const uint32_t dst_mask = 0xffffffffu >> (8 * (4 - fp.bpp));
    if (owned && !fp.init_from_clear) {
        const uint8_t* src = fp.fb + pix * fp.bpp;
        if (fp.bpp == 3) color = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16);
        else if (fp.bpp == 4) color = *reinterpret_cast<const uint32_t*>(src);
        else color = src[0];
    }
#endif
    uint32_t frags = 0;
    double zmax = -__builtin_inf();
#if !TRGL_USER_DEPTH_WRITE
    double zmin = __builtin_inf();
#endif
    const bool zero_locked = stats->zero_locked != 0;

    const uint32_t beg = item4.y, end = item4.z;
    // the list, 64 entries per step: lane l reads entry p0 + l, and the entries whose block mask has this wave's bit are visited
    // in list order
    for (uint32_t p0 = beg; p0 < end; p0 += 64) {
        const uint32_t p = p0 + (uint32_t)lane;
        uint32_t v = 0;
        bool hit = false;
        if (p < end) { v = vals[p]; hit = (bmask[p] >> kblk) & 1u; }
        unsigned long long cand = __ballot(hit);
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1;
            const uint32_t tri = TRGL_VAL_TRI((uint32_t)__builtin_amdgcn_readlane((int)v, j));   // index of the triangle in the flush
            CRec& r = ((CRec*)recs)[tri];
            // our_gl.cpp:147-148 visits the clamped bbox only
            if (!(x >= (int)r.bx0 && x <= (int)r.bx1 && y >= (int)r.by0 && y <= (int)r.by1)) continue;
            double b[3];
            {
                const double pxc = (double)x + 0.5, pyc = (double)y + 0.5;          // :149
                const double s0z = r.ax - pxc, s1z = r.ay - pyc;
                const double ux = r.s0y * s1z - s0z * r.s1y;                        // geometry.h:145
                const double uy = s0z * r.s1x - r.s0x * s1z;                        // geometry.h:146
                const double us = ux + uy;
                if (r.ruz != 0.0) {                                                 // :85 through the reciprocal ("exactness")
                    b[0] = 1.0 - trgl_shade::div_by_uz(us, r.uz, r.ruz); b[1] = trgl_shade::div_by_uz(uy, r.uz, r.ruz);
                    b[2] = trgl_shade::div_by_uz(ux, r.uz, r.ruz);
                } else {                                                            // :85, as written (TRGL_DL_LITERAL)
                    b[0] = 1.0 - us / r.uz; b[1] = uy / r.uz; b[2] = ux / r.uz;
                }
            }
            if (b[0] < 0 || b[1] < 0 || b[2] < 0) continue;                        // :152
            const double zn = b[0] * r.z0 + b[1] * r.z1 + b[2] * r.z2;               // :156-158
            if (!__builtin_isfinite(zn) || !(zn < z)) continue;                      // :160, :165
            const uint32_t dl = r.dl;
            const uint32_t di = (uint32_t)__builtin_amdgcn_readfirstlane((int)TRGL_DL_DRAW(dl));
            CDraw& d = ((CDraw*)draws)[di];
            const TriW rw = recs_w[tri];
            trgl_frag_in in;
            const double denom = b[0] * rw.iw0 + b[1] * rw.iw1 + b[2] * rw.iw2;      // :172-174
            if (fabs(denom) < 1e-15) { in.bar[0] = b[0]; in.bar[1] = b[1]; in.bar[2] = b[2]; }                  // :177-185
            else { in.bar[0] = (b[0] * rw.iw0) / denom; in.bar[1] = (b[1] * rw.iw1) / denom; in.bar[2] = (b[2] * rw.iw2) / denom; }
            const uint32_t local = TRGL_DL_LOCAL(dl);
            in.vary = d.vary ? d.vary + (size_t)local * (uint32_t)d.K : nullptr;
            in.u = (const trgl_uniforms*)&d.u;
            in.color = r.color;
            in.tex = (const DevTexture*)(CTex*)tex;
#if TRGL_USER_READS_DEST
            in.dst = color & dst_mask;
#else
            in.dst = 0;
#endif
            const trgl_frag_out o = trgl_fragment(in);                               // :187
            if (o.discard) continue;                                                 // :188
#if TRGL_USER_DEPTH_WRITE
            z = zn;                                                                  // :191
#else
            asm("v_min_f64 %0, %0, %1" : "+v"(zmin) : "v"(zn));                      // :197, of the depths :191 would have written
#endif
            color = o.bgra;                                                          // :192 (TGAImage::set at block-out)
            ++frags;                                                                 // :194
            asm("v_max_f64 %0, %0, %1" : "+v"(zmax) : "v"(zn));                      // :198 (the sign of a zero end: below)
            // std::min / std::max keep the first of equal values and +0.0 == -0.0: when the z range ends in a zero its sign is that
            // of the first zero written in the reference's order (triangle, x, y), see DevStats
            if (zn == 0.0 && !zero_locked) {
                const unsigned long long order = ((unsigned long long)tri << 32) | ((unsigned long long)x << 16) | (unsigned long long)y;
                atomicMin(__builtin_signbit(zn) ? &stats->zero_neg_key : &stats->zero_pos_key, order);
            }
        }
    }

    // ---- block out: every owned pixel once (the colour only where this flush wrote it, or from the clear) ----------------
    if (owned) {
#if TRGL_USER_DEPTH_WRITE
        fp.zb[pix] = z;
#else
        if (fp.init_from_clear) fp.zb[pix] = z;           // (otherwise the depth is in place already)
#endif
        if (fp.init_from_clear || frags) trgl_shade::store_pixel(fp, pix, color);
    }
    // ---- one partial of our_gl.cpp:194-198 per work item, in k_raster's layout (work_items.h)
#if TRGL_USER_DEPTH_WRITE
    // (the smallest depth a pixel was written with is its last one: the z-test only lets smaller ones through)
    unsigned long long fr = frags, kmin = zkey(frags ? z : __builtin_inf()), kmax = zkey(zmax);
#else
    unsigned long long fr = frags, kmin = zkey(zmin), kmax = zkey(zmax);
#endif
    for (int o = 32; o; o >>= 1) {
        fr += __shfl_xor(fr, o);
        const unsigned long long a = __shfl_xor(kmin, o); kmin = a < kmin ? a : kmin;
        const unsigned long long c = __shfl_xor(kmax, o); kmax = c > kmax ? c : kmax;
    }
    if (lane == 0) { s_red[w][0] = fr; s_red[w][1] = kmin; s_red[w][2] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            fr += s_red[k][0]; kmin = s_red[k][1] < kmin ? s_red[k][1] : kmin; kmax = s_red[k][2] > kmax ? s_red[k][2] : kmax;
        }
        trgl_item_stats_store(my_stats, fr, kmin, kmax);
    }
}
