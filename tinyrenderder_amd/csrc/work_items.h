// work_items.h — the contract between k_make_items, the raster kernels (k_raster, raster_user.h), the shade kernels (k_shade,
// shade_user.h), k_fold_stats and launch_raster, stated once.  Compiled for the host and the device, and by hiprtc under this name
// (user_shaders.cpp embeds it).  Plain integer functions: a kernel that calls them keeps the instructions it had with literals.
#pragma once
#include "trgl_device.h"

// A work item is one workgroup's job: one row of four 8x8 blocks of a tile that has triangles (up to four items per tile), or one
// whole tile that is only cleared.  As a uint4: x = the item word, [y, z) = the tile's slice of the sorted pair list (one dependent
// load less at the start of every raster wave), w = 0.  The item word:
//   bits 0-23 tile, bits 24-25 row of blocks inside the tile, bit 31: the tile has no triangles and is only cleared
#define TRGL_ITEM_CLEAR 0x80000000u
TRGL_HD uint32_t trgl_item_rows(uint32_t tile, uint32_t brow) { return tile | (brow << 24); }
TRGL_HD uint32_t trgl_item_clear(uint32_t tile) { return tile | TRGL_ITEM_CLEAR; }
TRGL_HD uint32_t trgl_item_tile(uint32_t item) { return item & 0xffffffu; }
TRGL_HD uint32_t trgl_item_brow(uint32_t item) { return (item >> 24) & 3u; }

// Which of the G items workgroup b of a raster kernel takes.  Workgroups are dealt round-robin to the 8 XCDs (each with its own L2):
// b runs on the XCD of b mod 8, and every XCD gets one contiguous eighth of the list, so that the four block rows of a tile - and its
// neighbours, which share triangles with it - read their list and records through the same L2.  (Placement is an observed property,
// used for speed only.)  The answer is workgroup-uniform: a kernel may leave on `false` ahead of a barrier.  G lives on the device, so
// the grid is sized for the most items a flush can have.  The shade kernels take item blockIdx.x of a grid of max_items as it is.
TRGL_HD bool trgl_item_of_workgroup(uint32_t b, uint32_t G, uint32_t* g) {
    const uint32_t per = (G + 7u) >> 3, xj = b >> 3;
    *g = (b & 7u) * per + xj;
    return xj < per && *g < G;
}
TRGL_HD uint32_t trgl_item_grid(uint32_t max_items) { return ((max_items + 7u) / 8u) * 8u; }

// The partial a raster workgroup leaves for k_fold_stats, our_gl.cpp:194-198 over the item's pixels: four 64-bit words, 16-byte
// aligned - fragments written, smallest and largest depth key (zkey), 0.  An item without fragments leaves the neutral keys.
enum : int { TRGL_ITEM_STATS_WORDS = 4, TRGL_ITEM_FRAGS = 0, TRGL_ITEM_KMIN = 1, TRGL_ITEM_KMAX = 2 };
#define TRGL_ITEM_KMIN_NONE 0xffffffffffffffffull
#define TRGL_ITEM_KMAX_NONE 0ull
#ifdef __HIPCC__
__device__ __forceinline__ void trgl_item_stats_store(unsigned long long* partial, unsigned long long frags, unsigned long long kmin, unsigned long long kmax) {
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(partial);
    dst[0] = make_ulonglong2(frags, kmin); dst[1] = make_ulonglong2(kmax, 0ull);
}
#endif
