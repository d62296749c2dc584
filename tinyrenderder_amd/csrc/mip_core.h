// mip_core.h — mip chains, the filtered samplers and the level of detail (include/trgl.h, "Mipmapped textures") as the functions that
// the host paths (trgl_host.cpp), the kernels (kernels_mip.hip) and the user shaders' prelude (user_prelude.h, compiled at run time)
// all compile: one definition of every size, offset and rounding.  New work, the reference has no mipmaps.
// Unsigned integer arithmetic and fp64 without contraction; every written operation is rounded once, in the written order.  No libm
// call whose result could differ between host and device: floor, comparisons and bit patterns only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_MIP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_MIP_HD inline
#endif

namespace trgl {

// ---- sizes and layouts ----------------------------------------------------------------------------------------------------------------
// side of level l of a texture whose level 0 has side s: max(1, s_{l-1} / 2) applied l times = max(1, s >> l)
TRGL_MIP_HD int mip_side(int s, int l) { const int v = l < 31 ? s >> l : 0; return v > 0 ? v : 1; }
// L = 1 + floor(log2(max(w, h))), w, h >= 1
TRGL_MIP_HD int mip_levels(int w, int h) { int m = w > h ? w : h, L = 1; while (m > 1) { m >>= 1; ++L; } return L; }
TRGL_MIP_HD size_t mip_level_bytes(int w, int h, int bpp, int l) { return (size_t)mip_side(w, l) * (size_t)mip_side(h, l) * (size_t)bpp; }
// the packed buffer of trgl_mip_layout: level 1 at 0, every level at the next multiple of 16 behind its predecessor; l >= 1
TRGL_MIP_HD size_t mip_packed_offset(int w, int h, int bpp, int l) {
    size_t o = 0;
    for (int k = 1; k < l; ++k) o += (mip_level_bytes(w, h, bpp, k) + 15) & ~(size_t)15;
    return o;
}
// a texture slot's allocation: level 0, its 8 zero bytes, then every further level at the next multiple of 16 behind its
// predecessor's 4 zero bytes (the samplers' tail rule: a texel is one 4-byte load).  Offset of level l >= 1 from level 0; with
// l = L the bytes of the whole allocation.
TRGL_MIP_HD size_t mip_slot_offset(int w, int h, int bpp, int l) {
    size_t o = (mip_level_bytes(w, h, bpp, 0) + 8 + 15) & ~(size_t)15;
    for (int k = 1; k < l; ++k) o += (mip_level_bytes(w, h, bpp, k) + 4 + 15) & ~(size_t)15;
    return o;
}

// ---- the chain's arithmetic: one texel channel of level l + 1 from fx * fy bytes of level l (fx, fy in {1, 2}) ------------------------
TRGL_MIP_HD uint32_t mip_round(uint32_t sum, uint32_t n) { return n == 4 ? (sum + 2u) >> 2 : n == 2 ? (sum + 1u) >> 1 : sum; }

// ---- samplers -------------------------------------------------------------------------------------------------------------------------
// an image and its further levels: `chain` + the offset of level l (slot: mip_slot_offset from level 0 itself; else mip_packed_offset)
struct MipView { const uint8_t* level0; const uint8_t* chain; int w, h, bpp, levels; bool slot; };
struct MipTexel { uint32_t bgra; int bytespp; };

TRGL_MIP_HD const uint8_t* mip_level_ptr(const MipView& v, int l) {
    if (l == 0) return v.level0;
    return v.chain + (v.slot ? mip_slot_offset(v.w, v.h, v.bpp, l) : mip_packed_offset(v.w, v.h, v.bpp, l));
}
// the texel at p, bytes at and above bpp zero.  Device: ONE unaligned 4-byte load (4 readable bytes follow every level of a slot).
TRGL_MIP_HD uint32_t mip_texel(const uint8_t* p, int bpp) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return bpp >= 4 ? v : v & ((1u << (8 * bpp)) - 1u);
#else
    uint32_t v = 0;
    for (int i = 0; i < bpp; ++i) v |= (uint32_t)p[i] << (8 * i);
    return v;
#endif
}
// (int)double as x86-64 executes it: out of range and NaN -> INT_MIN (shade_common.h: tex_fetch)
TRGL_MIP_HD int mip_cvtt(double d) {
    if (!(d > -2147483649.0 && d < 2147483648.0)) return -2147483647 - 1;
    return (int)d;
}
TRGL_MIP_HD int mip_iclamp(int v, int lo, int hi) { return v < lo ? lo : hi < v ? hi : v; }
TRGL_MIP_HD int mip_clamp_level(const MipView& v, int level) { return mip_iclamp(level, 0, v.levels - 1); }

// trgl_sample2D_level: tex_fetch's rule on level `level` (clamped)
TRGL_MIP_HD MipTexel mip_sample_level(const MipView& v, const double uv[2], int level) {
    const int l = mip_clamp_level(v, level);
    const int wl = mip_side(v.w, l), hl = mip_side(v.h, l);
    const int x = mip_iclamp(mip_cvtt(uv[0] * wl), 0, wl - 1);
    const int y = mip_iclamp(mip_cvtt(uv[1] * hl), 0, hl - 1);
    return MipTexel{ mip_texel(mip_level_ptr(v, l) + ((size_t)x + (size_t)y * wl) * v.bpp, v.bpp), v.bpp };
}
// one axis of the bilinear footprint: the two clamped texels and the weight of the second in 1/256
TRGL_MIP_HD void mip_axis(double t, int size, int* a, int* b, uint32_t* f) {
    double u = t * (double)size - 0.5;
    if (!(u >= -1.0)) u = -1.0;
    if (u > (double)size) u = (double)size;
    const double fl = __builtin_floor(u);
    const int x0 = (int)fl;
    *f = (uint32_t)(int)((u - fl) * 256.0);
    *a = mip_iclamp(x0, 0, size - 1);
    *b = mip_iclamp(x0 + 1, 0, size - 1);
}
// trgl_sample2D_linear
TRGL_MIP_HD MipTexel mip_sample_linear(const MipView& v, const double uv[2], int level) {
    const int l = mip_clamp_level(v, level);
    const int wl = mip_side(v.w, l), hl = mip_side(v.h, l);
    int xa, xb, ya, yb; uint32_t fx, fy;
    mip_axis(uv[0], wl, &xa, &xb, &fx);
    mip_axis(uv[1], hl, &ya, &yb, &fy);
    const uint8_t* p = mip_level_ptr(v, l);
    const size_t ra = (size_t)ya * wl, rb = (size_t)yb * wl;
    const uint32_t caa = mip_texel(p + (ra + xa) * v.bpp, v.bpp), cba = mip_texel(p + (ra + xb) * v.bpp, v.bpp);
    const uint32_t cab = mip_texel(p + (rb + xa) * v.bpp, v.bpp), cbb = mip_texel(p + (rb + xb) * v.bpp, v.bpp);
    uint32_t out = 0;
    for (int s = 0; s < 32; s += 8) {
        const uint32_t top = ((caa >> s) & 255u) * (256u - fx) + ((cba >> s) & 255u) * fx;
        const uint32_t bot = ((cab >> s) & 255u) * (256u - fx) + ((cbb >> s) & 255u) * fx;
        out |= ((top * (256u - fy) + bot * fy + 32768u) >> 16) << s;
    }
    return MipTexel{ out, v.bpp };
}
// trgl_sample2D_trilinear
TRGL_MIP_HD MipTexel mip_sample_trilinear(const MipView& v, const double uv[2], double lod) {
    double lam = lod;
    if (!(lam > 0.0)) lam = 0.0;
    if (lam > (double)(v.levels - 1)) lam = (double)(v.levels - 1);
    const int l0 = (int)lam;
    const uint32_t t = (uint32_t)(int)((lam - (double)l0) * 256.0);
    const int l1 = l0 + 1 < v.levels - 1 ? l0 + 1 : v.levels - 1;
    const MipTexel a = mip_sample_linear(v, uv, l0);
    if (t == 0) return a;
    const MipTexel b = mip_sample_linear(v, uv, l1);
    uint32_t out = 0;
    for (int s = 0; s < 32; s += 8)
        out |= ((((a.bgra >> s) & 255u) * (256u - t) + ((b.bgra >> s) & 255u) * t + 128u) >> 8) << s;
    return MipTexel{ out, v.bpp };
}
// mode 0 level, 1 linear, 2 trilinear (trgl_selftest_sampler_lod, trgl_image_sample); in modes 0 and 1 lod is converted to int
TRGL_MIP_HD MipTexel mip_sample_mode(const MipView& v, const double uv[2], double lod, int mode) {
    if (mode == 2) return mip_sample_trilinear(v, uv, lod);
    const int level = mip_cvtt(lod);
    return mode == 1 ? mip_sample_linear(v, uv, level) : mip_sample_level(v, uv, level);
}

// ---- level of detail ------------------------------------------------------------------------------------------------------------------
TRGL_MIP_HD uint64_t mip_f64_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, sizeof(b)); return b; }
TRGL_MIP_HD double mip_bits_f64(uint64_t b) { double x; __builtin_memcpy(&x, &b, sizeof(x)); return x; }
TRGL_MIP_HD bool mip_finite(double x) { return ((mip_f64_bits(x) >> 52) & 0x7ffu) != 0x7ffu; }

// trgl_mip_lod: half the piecewise-linear log2 of r = texels per pixel
TRGL_MIP_HD double mip_lod(const double bar[3], const double k[4], int tex_w, int tex_h) {
    const double wp = (bar[0] * k[1] + bar[1] * k[2]) + bar[2] * k[3];
    const double r = (((k[0] * wp) * wp) * wp) * ((double)tex_w * (double)tex_h);
    if (!(r > 1.0)) return 0.0;
    const uint64_t b = mip_f64_bits(r);
    if (b == 0x7ff0000000000000ull) return 64.0;
    const int e = (int)((b >> 52) & 0x7ffu) - 1023;
    const double m = (double)(b & 0x000fffffffffffffull) * 2.220446049250313e-16;      // 2^-52, exact
    return 0.5 * ((double)e + m);
}

// trgl_lod_stage for one triangle: vp the 16 doubles of the Viewport, c its 12 clip doubles, uv its u0 v0 u1 v1 u2 v2; out (c, W0, W1, W2)
TRGL_MIP_HD void mip_lod_constants(const double* vp, const double* c, const double* uv, double out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0.0;
    bool ok = true;
    double sx[3], sy[3], q[3], U[3], V[3];
    for (int i = 0; i < 3; ++i) {
        const double W = c[4 * i + 3];
        if (!(W > 1e-12)) ok = false;
        double n[4];
        for (int k = 0; k < 4; ++k) { n[k] = c[4 * i + k] / W; if (!mip_finite(n[k])) ok = false; }
        double s = 0; s += vp[0] * n[0]; s += vp[1] * n[1]; s += vp[2] * n[2]; s += vp[3] * n[3]; sx[i] = s;
        s = 0; s += vp[4] * n[0]; s += vp[5] * n[1]; s += vp[6] * n[2]; s += vp[7] * n[3]; sy[i] = s;
        if (!mip_finite(sx[i]) || !mip_finite(sy[i])) ok = false;
        q[i] = 1.0 / W; U[i] = uv[2 * i] * q[i]; V[i] = uv[2 * i + 1] * q[i];
    }
    if (!ok) return;
    const double e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
    const double A = e1x * e2y - e1y * e2x;
    if (A == 0) return;
    double d1, d2;
    d1 = U[1] - U[0]; d2 = U[2] - U[0]; const double gxU = d1 * e2y - d2 * e1y, gyU = d2 * e1x - d1 * e2x;
    d1 = V[1] - V[0]; d2 = V[2] - V[0]; const double gxV = d1 * e2y - d2 * e1y, gyV = d2 * e1x - d1 * e2x;
    d1 = q[1] - q[0]; d2 = q[2] - q[0]; const double gxq = d1 * e2y - d2 * e1y, gyq = d2 * e1x - d1 * e2x;
    const double N = (U[0] * (gxV * gyq - gyV * gxq) - V[0] * (gxU * gyq - gyU * gxq)) + q[0] * (gxU * gyV - gyU * gxV);
    const double cc = mip_bits_f64(mip_f64_bits(N) & 0x7fffffffffffffffull) / (A * A);
    if (!mip_finite(cc)) return;
    out[0] = cc; out[1] = c[3]; out[2] = c[7]; out[3] = c[11];
}

}  // namespace trgl
