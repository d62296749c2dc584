// kernels_items.hip — the bookkeeping either side of the raster kernel of a flush: k_make_items turns the per-tile slices of the sorted
// pair list into the work items k_raster (or a user kind's raster kernel) takes one per workgroup, and k_fold_stats folds the partials
// those workgroups leave, one per item, into the context's counters.  The contract of an item and of a partial is work_items.h's.
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "work_items.h"
#include "device_util.h"

namespace {

// Work items of the raster kernel (work_items.h).  Tiles outside the context's tile rows, empty tiles of a flush that
// does not start from clear, and block rows entirely outside the strip get no item.
__global__ __launch_bounds__(256) void k_make_items(FrameParams fp, const uint32_t* __restrict__ tile_start,
                                                    const uint32_t* __restrict__ tile_end,
                                                    uint4* __restrict__ items, uint32_t* __restrict__ n_items, TriRec* __restrict__ recs) {
    const int ntiles_strip = (fp.strip_ty1 - fp.strip_ty0) * fp.tiles_x;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    // The record behind the flush's last one belongs to no triangle: k_raster visits it when a cull round leaves an odd number of
    // survivors (its visit loop runs in pairs).  Its depth plane is +inf everywhere, so no pixel is in front of its stored depth and
    // the visit ends at its first test; should a pixel hold NaN (which lets every plane through), u.z = 1 > 0 = u.x + u.y fails coverage.
    if (k == 0 && fp.n_tris) {
        TriRec d;
        d.ax = d.ay = d.s0x = d.s0y = d.s1x = d.s1y = 0.0; d.c0 = __builtin_inf(); d.uz = 1.0; d.g1 = d.g2 = 0.0;
        d.ruz = 0.0; d.z0 = d.z1 = d.z2 = 0.0; d.bx0 = d.by0 = 1; d.bx1 = d.by1 = 0; d.color = 0; d.dl = 0;
        recs[fp.n_tris] = d;
    }
    uint32_t nb = 0, t = 0, rows = 0;          // rows: bit r set = block row r of the tile gets an item
    uint32_t beg = 0, end = 0;
    bool clear_only = false;
    if (k < ntiles_strip) {
        t = (uint32_t)(fp.strip_ty0 * fp.tiles_x + k);
        beg = tile_start[t]; end = tile_end[t];
        if (end <= beg) beg = end = 0;         // an empty tile: the last radix pass leaves it at [~0, 0)
        const uint32_t n = end - beg;
        const int ty = (int)(t / (uint32_t)fp.tiles_x);
        if ((n || fp.init_from_clear) && tile_row_owned(fp, ty)) {
            if (n) {
                for (int r = 0; r < 4; ++r) {
                    const int y0 = ty * TRGL_TILE + 8 * r, y1 = y0 + 7;
                    if (y0 < fp.H && y1 >= fp.strip_y0 && y0 < fp.strip_y1) rows |= 1u << r;
                }
                nb = (uint32_t)__popc(rows);
            } else { clear_only = true; nb = 1; }
        }
    }
    // wave-aggregated append (order of items is irrelevant)
    const uint32_t inc = trgl_dev::wave_incl_scan(nb);
    const int lane = threadIdx.x & 63;
    const uint32_t total = __shfl(inc, 63);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(n_items, total);
    base = __shfl(base, 63) + inc - nb;
    if (clear_only) items[base] = make_uint4(trgl_item_clear(t), 0u, 0u, 0u);
    else for (uint32_t r = 0; r < 4; ++r) if ((rows >> r) & 1u) items[base++] = make_uint4(trgl_item_rows(t, r), beg, end, 0u);
}

// after the raster kernel of a flush: fold the per-item partials into the context's counters (our_gl.cpp:194-198) and fix the
// sign of a zero z-range end (see DevStats).  FOLD_BLOCKS blocks take a slice each and add it with three atomics; the block
// that finishes last (a counter behind a device-scope fence) settles the per-flush state.  (One block walking 65536 partials
// took 39 us of a 2.9 ms frame.)
constexpr int FOLD_BLOCKS = 32;
__global__ __launch_bounds__(1024) void k_fold_stats(DevStats* __restrict__ s, uint32_t* __restrict__ n_items,
                                                     const unsigned long long* __restrict__ item_stats) {
    __shared__ unsigned long long sh[3][16];
    __shared__ bool s_last;
    const uint32_t n = *n_items;
    unsigned long long fr = 0, kmin = TRGL_ITEM_KMIN_NONE, kmax = TRGL_ITEM_KMAX_NONE;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long* partial = item_stats + (size_t)i * TRGL_ITEM_STATS_WORDS;
        const ulonglong2 a = reinterpret_cast<const ulonglong2*>(partial)[0];      // TRGL_ITEM_FRAGS, TRGL_ITEM_KMIN
        const unsigned long long c = partial[TRGL_ITEM_KMAX];
        fr += a.x; kmin = a.y < kmin ? a.y : kmin; kmax = c > kmax ? c : kmax;
    }
    for (int o = 32; o; o >>= 1) {                      // (one butterfly for the three, as in k_raster)
        fr += __shfl_xor(fr, o);
        unsigned long long a = __shfl_xor(kmin, o); kmin = a < kmin ? a : kmin;
        unsigned long long b = __shfl_xor(kmax, o); kmax = b > kmax ? b : kmax;
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { sh[0][w] = fr; sh[1][w] = kmin; sh[2][w] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
            fr += sh[0][k]; kmin = sh[1][k] < kmin ? sh[1][k] : kmin; kmax = sh[2][k] > kmax ? sh[2][k] : kmax;
        }
        if (fr) {       // items without fragments carry the neutral keys
            atomicAdd(&s->fragments, fr);
            atomicMin(&s->zmin_key, kmin);
            atomicMax(&s->zmax_key, kmax);
        }
        __threadfence();
        s_last = atomicAdd(&n_items[1], 1u) == gridDim.x - 1;       // n_items[1]: blocks of this launch that are done
    }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        if (!s->zero_locked && (s->zero_pos_key != TRGL_ZERO_KEY_EMPTY || s->zero_neg_key != TRGL_ZERO_KEY_EMPTY)) {
            s->zero_sign = s->zero_neg_key < s->zero_pos_key ? 1u : 0u;
            s->zero_locked = 1u;
        }
        s->literal_tris = 0; s->large_tris = 0;    // counted per flush (k_setup)
        s->zero_pos_key = TRGL_ZERO_KEY_EMPTY;
        s->zero_neg_key = TRGL_ZERO_KEY_EMPTY;
        n_items[0] = 0;         // every block read it before its atomic above; k_make_items of the next flush appends from 0
        n_items[1] = 0;
    }
}

}  // namespace

namespace trgl {

uint32_t owned_tiles(const FrameParams& fp) {
    if (fp.il_tiles == 0) return (uint32_t)((fp.strip_ty1 - fp.strip_ty0) * fp.tiles_x);
    return (uint32_t)(il_owned_below(fp, fp.tiles_y) * fp.tiles_x);
}

// at most four work items (rows of blocks) per owned tile
uint32_t raster_max_items(const FrameParams& fp) { return owned_tiles(fp) * 4u; }

void launch_make_items(hipStream_t s, const FrameParams& fp, int tiles, const uint32_t* tile_start, const uint32_t* tile_end, uint4* items,
                       uint32_t* n_items, TriRec* recs) {
    hipLaunchKernelGGL(k_make_items, dim3((tiles + 255) / 256), dim3(256), 0, s, fp, tile_start, tile_end, items, n_items, recs);
}

void launch_fold_stats(hipStream_t s, DevStats* stats, uint32_t* n_items, const unsigned long long* item_stats) {
    hipLaunchKernelGGL(k_fold_stats, dim3(FOLD_BLOCKS), dim3(1024), 0, s, stats, n_items, item_stats);
}

}  // namespace trgl
