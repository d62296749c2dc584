// box_core.h — the box filter's definition (include/trgl.h, trgl_image_downsample) as the functions that the host path (trgl_host.cpp) and
// the kernel (kernels_resolve.hip) both compile: one rounding rule, one division.  Unsigned integer arithmetic throughout.
//   w2 = w / f, h2 = h / f;   dst(x, y, c) = (sum over j < f, i < f of src(x * f + i, y * f + j, c) + (f * f) / 2) / (f * f)
// Source columns >= w2 * f and rows >= h2 * f have no influence.  (f * f) / 2 is an integer division: an exact tie exists only for even f
// and rounds up.  f <= TRGL_MAX_BOX_FACTOR = 16: the largest sum, 256 * 255 = 65280, fits 16 bits, and so does every partial sum.
#pragma once
#include <stdint.h>
#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_BOX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_BOX_HD inline
#endif

namespace trgl {

// n / (f * f) as a multiplication: box_magic(f) = 2^32 / (f * f) + 1, and (n * magic) >> 32 == n / (f * f) for every n < 2^17 -
// the excess magic * f * f - 2^32 is at most f * f <= 256, so n times it stays below 2^32 (all of 65280 + 128 < 2^17).
// f in 2..16: with f = 1 the magic does not fit 32 bits, and the filter is the identity - both paths copy.
TRGL_BOX_HD uint32_t box_magic(int f) { return (uint32_t)(0x100000000ull / (uint32_t)(f * f)) + 1u; }
// the output byte of a block whose f * f bytes add up to `sum`
TRGL_BOX_HD uint32_t box_round(uint32_t sum, uint32_t half, uint32_t magic) { return (uint32_t)(((uint64_t)(sum + half) * magic) >> 32); }

}  // namespace trgl
