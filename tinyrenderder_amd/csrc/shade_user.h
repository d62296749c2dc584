// shade_user.h — the shade kernel of a user kind (include/trgl.h, "User shaders"), compiled by hiprtc behind the user's source,
// which defines trgl_fragment.  The structure of k_shade (kernels_raster.hip): one 256-thread block per work item of k_raster,
// one 8x8 block per wave, the visibility buffer names the pixel's owner, draw descriptors come in through scalar loads from the
// constant address space, and the barycentrics are recomputed with the operations of the scan (TRGL_OWNER_BARYCENTRICS).  A launch
// shades the pixels whose draw has kind `kind` and leaves every other pixel alone.
#pragma once
#include "user_prelude.h"

static_assert(__is_same(decltype(trgl_fragment(*(const trgl_frag_in*)nullptr)), uint32_t),
              "trgl_fragment must return uint32_t (a shader whose fragment returns trgl_frag_out is registered with TRGL_SHADER_MAY_DISCARD)");

extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void trgl_shade_user(FrameParams fp, const TriRec* __restrict__ recs, const TriW* __restrict__ recs_w, const DrawDesc* __restrict__ draws,
                     const DevTexture* __restrict__ tex, const uint4* __restrict__ items, const uint32_t* __restrict__ n_items, int kind) {
    const int lane = threadIdx.x & 63;
    const uint32_t item_idx = blockIdx.x;
    if (item_idx >= *n_items) return;
    const uint32_t item = items[item_idx].x;
    if (item & TRGL_ITEM_CLEAR) return;                  // no triangles: no owners
    const int t = (int)trgl_item_tile(item);
    const int tile_y = t / fp.tiles_x, tile_x = t - tile_y * fp.tiles_x;
    const int x = (tile_x << TRGL_TILE_LOG2) + 8 * (int)(threadIdx.x >> 6) + (lane & 7);
    const int y = (tile_y << TRGL_TILE_LOG2) + 8 * (int)trgl_item_brow(item) + (lane >> 3);
    const bool mine = x < fp.W && y < fp.H && y >= fp.strip_y0 && y < fp.strip_y1;
    const size_t idx = (size_t)x + (size_t)y * fp.W;
    const uint32_t dl = mine ? fp.idbuf[idx] : 0xffffffffu;
    if (dl == 0xffffffffu) return;
    typedef const __attribute__((address_space(4))) DrawDesc CDraw;
    typedef const __attribute__((address_space(4))) DevTexture CTex;
    uint32_t color = 0;
    bool own = false;
    unsigned long long todo = __ballot(true);
    while (todo) {                                       // one draw at a time (wave-uniform in all but exotic flushes)
        const int src = __builtin_ctzll(todo);
        const uint32_t di = (uint32_t)__builtin_amdgcn_readlane((int)(dl >> 24), src);
        const bool here = (dl >> 24) == di;
        todo &= ~__ballot(here);
        if (here && ((CDraw*)draws)[di].kind == kind) {
            const uint32_t di_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dl >> 24));
            CDraw& d = ((CDraw*)draws)[di_s];
            const uint32_t local = dl & 0xffffffu;
            trgl_frag_in in;
            in.vary = d.vary ? d.vary + (size_t)local * (uint32_t)d.K : nullptr;
            in.u = (const trgl_uniforms*)&d.u;
            in.tex = (const DevTexture*)(CTex*)tex;
            in.dst = 0;                                  // (only a kind with TRGL_SHADER_READS_DEST sees the pixel)
            const TriRec& r = recs[d.first + local];
            const TriW& rw = recs_w[d.first + local];
            TRGL_OWNER_BARYCENTRICS(r, rw, x, y, in.bar);
            in.color = r.color;
            color = trgl_fragment(in);
            own = true;
        }
    }
    if (own) trgl_shade::store_pixel(fp, idx, color);    // TGAImage::set, tgaimage.cpp:32-39
}
