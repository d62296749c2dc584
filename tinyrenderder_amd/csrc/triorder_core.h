// triorder_core.h — the three depth expressions of trgl_triangle_depths (include/trgl.h) as the functions that the host loop
// (trgl_host.cpp) and the kernel (kernels_triorder.hip) both compile: a fold over the clip w of a group's vertices in memory order,
// then bit 63 of the result flipped as an integer (NaNs included: trgl_depth_order sorts them by their sign).
// fp64, contraction off; no fmin / fmax (they differ on NaNs and on signed zeros).  Which NaN an addition returns is decided here in
// integers, not by the adder: x86 and gfx950 differ in it (inf - inf is a negative NaN on one and a positive one on the other).
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define TRGL_TRIORDER_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_TRIORDER_HD inline
#endif

namespace trgl {

TRGL_TRIORDER_HD uint64_t tri_f64_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, sizeof(b)); return b; }
TRGL_TRIORDER_HD double tri_bits_f64(uint64_t b) { double x; __builtin_memcpy(&x, &b, sizeof(x)); return x; }

// acc + w rounded to fp64.  A NaN result: acc with its quiet bit set when acc is a NaN, else w with its quiet bit set when w is one,
// else (+inf + -inf) the NaN 0xFFF8000000000000.
TRGL_TRIORDER_HD double tri_depth_add(double acc, double w) {
    const double r = acc + w;
    if (r == r) return r;
    const uint64_t quiet = uint64_t(1) << 51;
    if (acc != acc) return tri_bits_f64(tri_f64_bits(acc) | quiet);
    if (w != w) return tri_bits_f64(tri_f64_bits(w) | quiet);
    return tri_bits_f64(0xFFF8000000000000ull);
}

// the value of the fold once it has seen w_0 (mode: TRGL_TRI_DEPTH_CENTROID 0, NEAREST 1, FARTHEST 2)
TRGL_TRIORDER_HD double tri_depth_first(int mode, double w0) { return mode == 0 ? tri_depth_add(0.0, w0) : w0; }
// one step of the fold, w = w_v for v >= 1
TRGL_TRIORDER_HD double tri_depth_step(int mode, double acc, double w) {
    if (mode == 0) return tri_depth_add(acc, w);
    if (mode == 1) return (w < acc) ? w : acc;
    return (acc < w) ? w : acc;
}
// the 64 bits of the depth: those of the folded value with the sign bit flipped
TRGL_TRIORDER_HD uint64_t tri_depth_bits(double acc) { return tri_f64_bits(acc) ^ (uint64_t(1) << 63); }

}  // namespace trgl
