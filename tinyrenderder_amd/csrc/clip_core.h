// clip_core.h — the clip stage's definition (include/trgl.h, trgl_clip_stage) as the functions that the host path (trgl_host.cpp) and the
// kernels (kernels_clip.hip) both compile: one classification, one table of output slots, one interpolation.  fp64, contraction off.
#pragma once
#include <stdint.h>
#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_CLIP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_CLIP_HD inline
#endif

namespace trgl {

// What becomes of a triangle.  ONE + i: only vertex i is inside (one output); TWO + i: only vertex i is outside (two outputs).
enum : int { CLIP_DROP = 0, CLIP_PASS = 1, CLIP_ONE = 2, CLIP_TWO = 5 };
TRGL_CLIP_HD int clip_outputs(int code) { return code == CLIP_DROP ? 0 : code >= CLIP_TWO ? 2 : 1; }

TRGL_CLIP_HD bool clip_finite(double d) { return d - d == 0.0; }      // false for NaN and +-inf

// The signed distances of a triangle's vertices (tri: 12 doubles) and its class.  t[0], t[1]: the two intersection parameters of a cut
// triangle, each from the inside vertex toward the outside one: ONE + i: t(i->j), t(i->k); TWO + i: t(j->i), t(k->i); (i, j, k) a rotation.
TRGL_CLIP_HD int clip_classify(const double* tri, const double* p, double t[2]) {
    double d[3];
    bool finite = true;
    int inside = 0;
    for (int v = 0; v < 3; ++v) {
        const double* q = tri + 4 * v;
        d[v] = ((p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]) + p[3] * q[3];
        finite = finite && clip_finite(d[v]);
        inside |= (d[v] >= 0.0 ? 1 : 0) << v;                   // -0.0 is inside
    }
    t[0] = t[1] = 0.0;
    if (!finite || inside == 7) return CLIP_PASS;
    if (inside == 0) return CLIP_DROP;
    const bool one = inside == 1 || inside == 2 || inside == 4;
    const int odd = one ? inside : 7 ^ inside;                  // the bit of the odd vertex
    const int i = odd == 1 ? 0 : odd == 2 ? 1 : 2, j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
    if (one) { t[0] = d[i] / (d[i] - d[j]); t[1] = d[i] / (d[i] - d[k]); return CLIP_ONE + i; }
    t[0] = d[j] / (d[j] - d[i]); t[1] = d[k] / (d[k] - d[i]);
    return CLIP_TWO + i;
}

// Slot s of output `which` of a cut triangle: vertex *a when *a == *b, else the point from *a toward *b at t[*tsel].
TRGL_CLIP_HD void clip_slot(int code, int which, int s, int* a, int* b, int* tsel) {
    const bool one = code < CLIP_TWO;
    const int i = code - (one ? CLIP_ONE : CLIP_TWO), j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
    const int rel = s == i ? 0 : s == j ? 1 : 2;
    *tsel = 0;
    if (one) {
        *a = i; *b = rel == 0 ? i : rel == 1 ? j : k; *tsel = rel == 2 ? 1 : 0;
    } else if (which == 0) {
        if (rel == 0) { *a = j; *b = i; } else { *a = *b = rel == 1 ? j : k; }
    } else {
        if (rel == 0) { *a = k; *b = i; *tsel = 1; } else if (rel == 1) { *a = j; *b = i; } else { *a = *b = k; }
    }
}

TRGL_CLIP_HD double clip_lerp(double a, double b, double t) { return a + t * (b - a); }

// One output's 12 clip doubles
TRGL_CLIP_HD void clip_emit_clip(const double* tri, int code, int which, const double t[2], double* out) {
    if (code == CLIP_PASS) { for (int e = 0; e < 12; ++e) out[e] = tri[e]; return; }
    for (int s = 0; s < 3; ++s) {
        int a, b, ts;
        clip_slot(code, which, s, &a, &b, &ts);
        for (int e = 0; e < 4; ++e) out[4 * s + e] = a == b ? tri[4 * a + e] : clip_lerp(tri[4 * a + e], tri[4 * b + e], t[ts]);
    }
}

// Varying slot c of a triangle: vertex `s` of an attribute of `comp` components (the same component of vertex v sits at
// c + (v - s) * comp), or s < 0 for a per-triangle constant.
struct ClipSlotInfo { int8_t s; uint8_t comp; };
struct ClipTable { ClipSlotInfo slot[TRGL_MAX_USER_VARY]; };

// Varying slot c of one output
TRGL_CLIP_HD double clip_emit_vary(const double* vary, int c, ClipSlotInfo info, int code, int which, const double t[2]) {
    if (code == CLIP_PASS || info.s < 0) return vary[c];
    int a, b, ts;
    clip_slot(code, which, info.s, &a, &b, &ts);
    const double va = vary[c + (a - info.s) * (int)info.comp];
    return a == b ? va : clip_lerp(va, vary[c + (b - info.s) * (int)info.comp], t[ts]);
}

// The table of an attribute list over K varyings; false for a list include/trgl.h calls invalid
inline bool clip_table(const trgl_clip_attr* attrs, int n_attrs, int K, ClipTable* tab) {
    if (K < 0 || K > TRGL_MAX_USER_VARY || n_attrs < 0 || n_attrs > TRGL_MAX_CLIP_ATTRS || (n_attrs && !attrs)) return false;
    for (int c = 0; c < TRGL_MAX_USER_VARY; ++c) { tab->slot[c].s = -1; tab->slot[c].comp = 0; }
    for (int a = 0; a < n_attrs; ++a) {
        const int64_t off = attrs[a].offset, comp = attrs[a].components;
        if (off < 0 || comp < 1 || off + 3 * comp > K) return false;
        for (int e = 0; e < 3 * (int)comp; ++e) {
            ClipSlotInfo& si = tab->slot[off + e];
            if (si.s >= 0) return false;                        // two attributes overlap
            si.s = (int8_t)(e / (int)comp); si.comp = (uint8_t)comp;
        }
    }
    return true;
}

}  // namespace trgl
