// occlusion_core.h — the occlusion test's definition (include/trgl.h, trgl_occlusion_boxes_image, steps 1-6) as the functions that the
// host path (trgl_host.cpp) and the kernel (kernels_occlusion.hip) both compile: one corner transform, one fold over the corners, one
// decision.  Step 7 - is some depth of the rectangle above zq - is the caller's: a scan on the host, the two levels on the device.
// fp64, contraction off.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_OCCL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_OCCL_HD inline
#endif

namespace trgl {

// what the corners of a box fold to: the depth range, the screen extent, and whether a corner left the box undecided (steps 2, 3, a NaN
// screen coordinate of step 5)
struct OcclFold { double zmin, zmax, sx_min, sx_max, sy_min, sy_max; int undecided; };

TRGL_OCCL_HD bool occl_finite(double d) { return d - d == 0.0; }      // false for NaN and +-inf
TRGL_OCCL_HD double occl_dot4(const double* m, const double* p) {     // geometry.h:122-127: left to right from 0
    double sum = 0;
    sum += m[0] * p[0]; sum += m[1] * p[1]; sum += m[2] * p[2]; sum += m[3] * p[3];
    return sum;
}
// (int)double as the reference's x86-64 build executes it: NaN and out of range give INT_MIN
TRGL_OCCL_HD int occl_cast(double d) {
    if (!(d > -2147483649.0 && d < 2147483648.0)) return INT_MIN;
    return (int)d;
}

// Steps 1-3 and the screen position of step 5 for corner k of `box` (6 doubles); V: rows 0 and 1 of the viewport matrix.
TRGL_OCCL_HD OcclFold occl_corner(const double* M, const double* V, const double* box, int k) {
    const double p[4] = { (k & 1) ? box[3] : box[0], (k & 2) ? box[4] : box[1], (k & 4) ? box[5] : box[2], 1.0 };
    double clip[4], ndc[4];
    for (int r = 0; r < 4; ++r) clip[r] = occl_dot4(M + 4 * r, p);
    OcclFold f;
    f.undecided = !(clip[3] > 1e-12) ? 1 : 0;                                                    // step 2
    for (int r = 0; r < 4; ++r) ndc[r] = clip[r] / clip[3];                                      // step 3
    if (!(occl_finite(ndc[0]) && occl_finite(ndc[1]) && occl_finite(ndc[2]) && occl_finite(ndc[3]))) f.undecided = 1;
    const double sx = occl_dot4(V, ndc), sy = occl_dot4(V + 4, ndc);                             // step 5
    if (sx != sx || sy != sy) f.undecided = 1;
    f.zmin = f.zmax = ndc[2];
    f.sx_min = f.sx_max = sx; f.sy_min = f.sy_max = sy;
    return f;
}

// Two folds into one.  Once a fold is undecided its numbers no longer matter; of decided folds every number is finite or +-inf, never
// NaN, so minimum and maximum do not depend on the order the corners are merged in (but for the sign of a zero, which no later step sees).
TRGL_OCCL_HD OcclFold occl_merge(const OcclFold& a, const OcclFold& b) {
    OcclFold f;
    f.undecided = a.undecided | b.undecided;
    f.zmin = b.zmin < a.zmin ? b.zmin : a.zmin;         f.zmax = a.zmax < b.zmax ? b.zmax : a.zmax;
    f.sx_min = b.sx_min < a.sx_min ? b.sx_min : a.sx_min; f.sx_max = a.sx_max < b.sx_max ? b.sx_max : a.sx_max;
    f.sy_min = b.sy_min < a.sy_min ? b.sy_min : a.sy_min; f.sy_max = a.sy_max < b.sy_max ? b.sy_max : a.sy_max;
    return f;
}

// the rectangle of step 5, inclusive, and the depth of step 6 that a pixel has to exceed
struct OcclRect { int x0, x1, y0, y1; double zq; };

// Steps 4-6 on the fold of all 8 corners.  Returns the code, or -1 with *r filled: step 7 decides between HIDDEN and VISIBLE.
TRGL_OCCL_HD int occl_decide(const OcclFold& f, int w, int h, OcclRect* r) {
    if (f.undecided) return TRGL_OCCL_UNDECIDED;
    if (f.zmin > 1.0 || f.zmax < -1.0) return TRGL_OCCL_OUTSIDE;                                 // step 4
    const double fx1 = ceil(f.sx_max), fy1 = ceil(f.sy_max);
    if (fx1 >= 2147483648.0 || fy1 >= 2147483648.0) return TRGL_OCCL_UNDECIDED;                  // step 5: the cast would hide a far corner
    const int cx0 = occl_cast(floor(f.sx_min)), cx1 = occl_cast(fx1);
    const int cy0 = occl_cast(floor(f.sy_min)), cy1 = occl_cast(fy1);
    r->x0 = cx0 > 0 ? cx0 : 0; r->x1 = cx1 < w - 1 ? cx1 : w - 1;                                // our_gl.cpp:130-133
    r->y0 = cy0 > 0 ? cy0 : 0; r->y1 = cy1 < h - 1 ? cy1 : h - 1;
    if (r->x0 > r->x1 || r->y0 > r->y1) return TRGL_OCCL_OUTSIDE;
    const double Z = fabs(f.zmin) < fabs(f.zmax) ? fabs(f.zmax) : fabs(f.zmin);                  // step 6
    r->zq = f.zmin - Z * 0x1p-40;
    return -1;
}

}  // namespace trgl
