// scene_core.h — AABB::transform (geometry.h:297-327) and Frustum::intersects (our_gl.cpp:264-280) as the functions that the
// single-box calls and the host loops (trgl_host.cpp) and the kernels (kernels_scene.hip) all compile: one statement of the
// arithmetic behind trgl_aabb_transform, trgl_frustum_intersects, trgl_instance_boxes and trgl_frustum_boxes.
// fp64, contraction off; no fmin / fmax (they differ on NaNs and on signed zeros).
#pragma once

#if defined(__HIP__)
#define TRGL_SCENE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_SCENE_HD inline
#endif

namespace trgl {

// std::min(a, b) = (b < a) ? b : a and std::max(a, b) = (a < b) ? b : a with a the running bound: what decides NaNs and signed zeros
TRGL_SCENE_HD double keep_min(double bound, double p) { return p < bound ? p : bound; }
TRGL_SCENE_HD double keep_max(double bound, double p) { return bound < p ? p : bound; }
// dot<n> (geometry.h:122-127): summed left to right from 0
TRGL_SCENE_HD double dot3_from_zero(const double* a, double x, double y, double z) { double sum = 0; sum += a[0] * x; sum += a[1] * y; sum += a[2] * z; return sum; }

// AABB::transform: box = min.xyz then max.xyz, m row-major, out = min.xyz then max.xyz.  out may not alias box or m.
TRGL_SCENE_HD void aabb_transform_core(const double* box, const double* m, double* out) {
    double lo[3] = { 1e9, 1e9, 1e9 }, hi[3] = { -1e9, -1e9, -1e9 };             // geometry.h:309-310
    for (int i = 0; i < 8; ++i) {                                               // :300-307: corner i takes max.x for bit 0, max.y for bit 1, max.z for bit 2
        const double x = (i & 1) ? box[3] : box[0], y = (i & 2) ? box[4] : box[1], z = (i & 4) ? box[5] : box[2];
        double t[4];
        for (int row = 0; row < 4; ++row) {                                     // :314, mat * vec4(corner, 1.0): one dot<4> per row
            double sum = 0;
            sum += m[4 * row] * x; sum += m[4 * row + 1] * y; sum += m[4 * row + 2] * z; sum += m[4 * row + 3] * 1.0;
            t[row] = sum;
        }
        for (int a = 0; a < 3; ++a) {
            const double pos = t[a] / t[3];                                     // :315, no guard
            lo[a] = keep_min(lo[a], pos);                                       // :317-319
            hi[a] = keep_max(hi[a], pos);                                       // :321-323
        }
    }
    for (int a = 0; a < 3; ++a) { out[a] = lo[a]; out[3 + a] = hi[a]; }
}

// Frustum::intersects: planes = 6 x (nx, ny, nz, d), box = min.xyz then max.xyz
TRGL_SCENE_HD bool frustum_intersects_core(const double* planes, const double* box) {
    for (int i = 0; i < 6; ++i) {                                               // our_gl.cpp:265-278
        const double* pl = planes + 4 * i;
        double positive[3] = { box[0], box[1], box[2] };                        // :269
        for (int a = 0; a < 3; ++a) if (pl[a] >= 0) positive[a] = box[3 + a];   // :270-272
        if (dot3_from_zero(pl, positive[0], positive[1], positive[2]) + pl[3] < 0) return false;   // :275, Plane::distance
    }
    return true;
}

}  // namespace trgl
