// device_util.h — device helpers with users in more than one kernel file (a helper with one user lives in that user's file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trgl_dev {

// row m of a 4x4 matrix times (x, y, z, w) as geometry.h:122-127 sums it: left to right from 0 - the bits depend on the order
__device__ __forceinline__ double dot4(const double* m, double x, double y, double z, double w) {
    double sum = 0;
    sum += m[0] * x; sum += m[1] * y; sum += m[2] * z; sum += m[3] * w;
    return sum;
}

// inclusive prefix sum over the 64 lanes of a wave: lane l receives the sum over lanes 0 .. l
// (No wave_sum / wave_min / wave_max beside it: the xor butterflies of k_raster, k_fold_stats and k_zrange run their sum, minimum and
// maximum through ONE loop, and written as one call each they come out as other instructions.)
template <class T> __device__ __forceinline__ T wave_incl_scan(T v) {
    int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { T t = __shfl_up(v, o); if (lane >= o) v += t; }
    return v;
}

// exclusive prefix sum of one value per thread of a 256-thread block; the block's sum in *total (every thread).  smem: 4 words of LDS,
// which may still be read from an earlier call (hence the first barrier).
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* smem /*[4]*/, uint32_t* total) {
    uint32_t inc = wave_incl_scan(v);
    int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 63) smem[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { uint32_t s = smem[k]; if (k < w) base += s; tot += s; }
    *total = tot;
    return base + inc - v;
}

}  // namespace trgl_dev
