// skin_core.h — the definitions of trgl_skin_stage and trgl_pose_palette (include/trgl.h) as the functions that the host loops
// (trgl_host.cpp) and the kernels (kernels_skin.hip) both compile, and the one statement of the reference's operator* of two
// mat<4,4> (geometry.h:196-205) that those and trgl_draw_instanced's model_view * M_i (kernels_instance.hip) share.
// fp64, every operation rounded, contraction off.  A computed double that is a NaN is stored as 0x7FF8000000000000 (the STORED NaNs
// rule of the sprite stage: x86 and gfx950 differ in the NaN an operation generates and in the payload that survives).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define TRGL_SKIN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_SKIN_HD inline
#endif

namespace trgl {

TRGL_SKIN_HD double skin_canon(double x) {
    if (x == x) return x;
    const uint64_t b = 0x7FF8000000000000ull;
    double r; __builtin_memcpy(&r, &b, sizeof(r));
    return r;
}

// Element (r, c) of A * B, both row-major 4x4 (geometry.h:196-205): from 0.0, k ascending, one rounding per product and per sum
TRGL_SKIN_HD double mat4_mul_elem(const double* A, const double* B, int r, int c) {
    double sum = 0.0;
    sum += A[4 * r + 0] * B[0 + c]; sum += A[4 * r + 1] * B[4 + c]; sum += A[4 * r + 2] * B[8 + c]; sum += A[4 * r + 3] * B[12 + c];
    return sum;
}
// out = A * B; out aliases neither
TRGL_SKIN_HD void mat4_mul(const double* A, const double* B, double* out) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = mat4_mul_elem(A, B, r, c);
}

// dot<4> of a matrix row with (x, y, z, w) (geometry.h:123-127, 187-192): from 0.0, four products added in order
TRGL_SKIN_HD double skin_dot4(const double* row, double x, double y, double z, double w) {
    double sum = 0.0;
    sum += row[0] * x; sum += row[1] * y; sum += row[2] * z; sum += row[3] * w;
    return sum;
}

// The blended matrix B (rows 0 .. 2, 12 doubles) starts as +0.0 and takes one influence at a time, k ascending: B += w * M's rows 0 .. 2
TRGL_SKIN_HD void skin_blend_zero(double* B) { for (int e = 0; e < 12; ++e) B[e] = 0.0; }
TRGL_SKIN_HD void skin_blend_add(double* B, double w, const double* M) { for (int e = 0; e < 12; ++e) B[e] = B[e] + w * M[e]; }

// B * (x, y, z, 1): the skinned position, as stored
TRGL_SKIN_HD void skin_position(const double* B, double x, double y, double z, double* out) {
    for (int r = 0; r < 3; ++r) out[r] = skin_canon(skin_dot4(B + 4 * r, x, y, z, 1.0));
}

// normalized(B * (dx, dy, dz, 0)) (geometry.h:136-140), as stored: a length of exactly 0 returns the vector, else three divisions
TRGL_SKIN_HD void skin_direction(const double* B, double dx, double dy, double dz, double* out) {
    double d[3];
    for (int r = 0; r < 3; ++r) d[r] = skin_dot4(B + 4 * r, dx, dy, dz, 0.0);
    double sum = 0.0;
    sum += d[0] * d[0]; sum += d[1] * d[1]; sum += d[2] * d[2];
    const double length = sqrt(sum);
    const bool zero = length == 0.0;
    for (int r = 0; r < 3; ++r) out[r] = skin_canon(zero ? d[r] : d[r] / length);
}

// the offsets of the flagged directions in the reference's Vertex (model.h:14-20): normal, tangent, bitangent
TRGL_SKIN_HD int skin_dir_offset(int which) { return which == 0 ? 3 : which == 1 ? 8 : 11; }

// parents[j] names a joint below j; anything else that is not -1 is refused on the host and a root on the device
TRGL_SKIN_HD bool pose_parent_below(int32_t parent, uint32_t j) { return parent >= 0 && (uint32_t)parent < j; }

}  // namespace trgl
