// sprite_core.h — the definitions of trgl_sprite_stage and trgl_line_stage (include/trgl.h) as the functions that the host loops
// (trgl_host.cpp) and the kernels (kernels_sprite.hip) both compile: one point or one segment becomes the four corners of a quad, and
// the quad's two output rows are read off those corners by one table.  fp64, every operation rounded, contraction off.
// A computed double that is a NaN is stored as 0x7FF8000000000000: x86 and gfx950 differ in the NaN an operation generates (inf - inf
// is negative on one, positive on the other) and in the operand whose payload survives, so the stored bits are decided here.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_SPRITE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_SPRITE_HD inline
#endif

namespace trgl {

// The quad of one primitive: corners k0 .. k3 (4 clip doubles each) and what its varyings hold: the first component of a vertex is ta at
// k0 and k3, tb at k1 and k2; the second is +0.0 at k0 and k1, `one` at k2 and k3.  A sprite has ta = 0, tb = 1, one = 1; an all-zero
// quad has zeros everywhere.
struct SpriteQuad { double k[16]; double ta, tb, one; };

TRGL_SPRITE_HD double sprite_canon(double x) {
    if (x == x) return x;
    const uint64_t b = 0x7FF8000000000000ull;
    double r; __builtin_memcpy(&r, &b, sizeof(r));
    return r;
}

// the reference's mat * vec for one row (geometry.h:123-127): summed from 0.0 in component order
TRGL_SPRITE_HD double sprite_dot(const double* row, double v0, double v1, double v2, double v3) {
    return (((0.0 + row[0] * v0) + row[1] * v1) + row[2] * v2) + row[3] * v3;
}

TRGL_SPRITE_HD void sprite_quad_zero(SpriteQuad* q) {
    for (int e = 0; e < 16; ++e) q->k[e] = 0.0;
    q->ta = q->tb = q->one = 0.0;
}

// the corner signs of k0 .. k3: x (-, +, +, -), y (-, -, +, +)
TRGL_SPRITE_HD bool quad_plus_x(int corner) { return corner == 1 || corner == 2; }
TRGL_SPRITE_HD bool quad_plus_y(int corner) { return corner >= 2; }

// Point p of size s
TRGL_SPRITE_HD void sprite_quad(const trgl_sprite_params& P, double px, double py, double pz, double s, SpriteQuad* q) {
    double e[4];
    for (int r = 0; r < 4; ++r) e[r] = sprite_dot(P.model_view + 4 * r, px, py, pz, 1.0);
    const double h = 0.5 * s;
    if (P.mode == TRGL_SPRITE_VIEW) {
        for (int k = 0; k < 4; ++k) {
            const double x = quad_plus_x(k) ? e[0] + h : e[0] - h, y = quad_plus_y(k) ? e[1] + h : e[1] - h;
            for (int r = 0; r < 4; ++r) q->k[4 * k + r] = sprite_canon(sprite_dot(P.projection + 4 * r, x, y, e[2], e[3]));
        }
    } else {
        double c[4];
        for (int r = 0; r < 4; ++r) c[r] = sprite_dot(P.projection + 4 * r, e[0], e[1], e[2], e[3]);
        const double hx = (h * P.scale[0]) * c[3], hy = (h * P.scale[1]) * c[3];
        for (int k = 0; k < 4; ++k) {
            q->k[4 * k + 0] = sprite_canon(quad_plus_x(k) ? c[0] + hx : c[0] - hx);
            q->k[4 * k + 1] = sprite_canon(quad_plus_y(k) ? c[1] + hy : c[1] - hy);
            q->k[4 * k + 2] = sprite_canon(c[2]);
            q->k[4 * k + 3] = sprite_canon(c[3]);
        }
    }
    q->ta = 0.0; q->tb = 1.0; q->one = 1.0;
}

TRGL_SPRITE_HD double line_lerp(double in, double out, double t) { return in + t * (out - in); }

// Segment a -> b.  k0 = A-, k1 = B-, k2 = B+, k3 = A+.
TRGL_SPRITE_HD void line_quad(const trgl_line_params& P, double a0, double a1, double a2, double b0, double b1, double b2, SpriteQuad* q) {
    double ea[4], eb[4], ca[4], cb[4];
    for (int r = 0; r < 4; ++r) { ea[r] = sprite_dot(P.model_view + 4 * r, a0, a1, a2, 1.0); eb[r] = sprite_dot(P.model_view + 4 * r, b0, b1, b2, 1.0); }
    for (int r = 0; r < 4; ++r) { ca[r] = sprite_dot(P.projection + 4 * r, ea[0], ea[1], ea[2], ea[3]); cb[r] = sprite_dot(P.projection + 4 * r, eb[0], eb[1], eb[2], eb[3]); }
    double ta = 0.0, tb = 1.0;
    const bool a_in = ca[3] >= P.w_min, b_in = cb[3] >= P.w_min;      // (a NaN is not inside)
    // (one exit: a quad that comes out all-zero is computed like any other and zeroed as it is stored)
    if (a_in != b_in) {
        // from the inside endpoint toward the outside one, whichever of the two that is (selects, not pointers: the arrays stay in registers)
        const double d_in = (a_in ? ca[3] : cb[3]) - P.w_min, d_out = (a_in ? cb[3] : ca[3]) - P.w_min;
        const double t = d_in / (d_in - d_out);
        for (int r = 0; r < 4; ++r) {
            const double v = line_lerp(a_in ? ca[r] : cb[r], a_in ? cb[r] : ca[r], t);
            cb[r] = a_in ? v : cb[r]; ca[r] = a_in ? ca[r] : v;
        }
        const double tv = line_lerp(a_in ? ta : tb, a_in ? tb : ta, t);
        tb = a_in ? tv : tb; ta = a_in ? ta : tv;
    }
    const double ax = ca[0] / ca[3], ay = ca[1] / ca[3], bx = cb[0] / cb[3], by = cb[1] / cb[3];
    const double dx = (bx - ax) * P.half_extent[0], dy = (by - ay) * P.half_extent[1];
    const double len = sqrt(dx * dx + dy * dy);
    const bool live = (a_in || b_in) && len > 0.0 && len - len == 0.0;
    const double hw = 0.5 * P.width;
    const double ox = ((-dy / len) * hw) / P.half_extent[0], oy = ((dx / len) * hw) / P.half_extent[1];
    for (int k = 0; k < 4; ++k) {
        const double* c = (k == 0 || k == 3) ? ca : cb;
        const bool plus = k >= 2;
        q->k[4 * k + 0] = live ? sprite_canon(plus ? c[0] + ox * c[3] : c[0] - ox * c[3]) : 0.0;
        q->k[4 * k + 1] = live ? sprite_canon(plus ? c[1] + oy * c[3] : c[1] - oy * c[3]) : 0.0;
        q->k[4 * k + 2] = live ? sprite_canon(c[2]) : 0.0;
        q->k[4 * k + 3] = live ? sprite_canon(c[3]) : 0.0;
    }
    q->ta = live ? sprite_canon(ta) : 0.0; q->tb = live ? sprite_canon(tb) : 0.0; q->one = live ? 1.0 : 0.0;
}

// ---- the two output rows of a quad: triangle 0 is (k0, k1, k2), triangle 1 is (k0, k2, k3) ----
TRGL_SPRITE_HD int quad_corner(int tri, int slot) { return slot == 0 ? 0 : slot + tri; }
// double r (0 .. 23) of the quad's two clip rows: its index into SpriteQuad::k
TRGL_SPRITE_HD int quad_clip_index(int r) {
    const int tri = r >= 12 ? 1 : 0, s = r - 12 * tri;
    return 4 * quad_corner(tri, s >> 2) + (s & 3);
}
// double c (0 .. 5) of the varyings row of triangle `tri`: 0 ta, 1 tb, 2 +0.0, 3 `one`
TRGL_SPRITE_HD int quad_vary_sel(int tri, int c) {
    const int k = quad_corner(tri, c >> 1);
    if ((c & 1) == 0) return (k == 0 || k == 3) ? 0 : 1;
    return k >= 2 ? 3 : 2;
}
TRGL_SPRITE_HD double quad_vary(double ta, double tb, double one, int sel) { return sel == 0 ? ta : sel == 1 ? tb : sel == 2 ? 0.0 : one; }

}  // namespace trgl
