// shade_common.h — device code shared by k_raster / k_shade (kernels_raster.hip) and the kernels of user shaders, which hiprtc
// compiles at run time from shade_user.h and raster_user.h (user_shaders.cpp embeds this file as text).  One copy of the samplers,
// of the division by u.z, of the per-pixel prologue of deferred shading and of the store of a cleared tile; the work items these
// kernels take are work_items.h's.
#pragma once
#include "trgl_device.h"
#include "work_items.h"

namespace trgl_shade {

__device__ __forceinline__ int iclamp(int v, int lo, int hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }

// ---- samplers: model.cpp:415-459 + TGAImage::get tgaimage.cpp:24-30 ----------------------------
struct Color { uint32_t bgra; int bytespp; };   // TGAColor (tgaimage.h:29-31), bgra[0] in the low byte

// (TX: pointer to DevTexture in the generic or in the constant address space - k_shade reads descriptors through scalar loads)
template <class TX>
__device__ __forceinline__ TX tex_slot(TX tex, int slot) {
    if (slot < 0 || slot >= TRGL_MAX_TEXTURES) return nullptr;
    if (!tex[slot].data || tex[slot].w <= 0) return nullptr;
    return &tex[slot];
}
// TGAImage::get at the clamped texel (model.cpp:420-425 etc.): ONE unaligned 4-byte load per texel (the device copy
// of every texture is padded by 4 bytes), masked to bpp bytes = TGAColor(p, bpp) with the rest 0 (tgaimage.h:46-50).
template <class TX>
__device__ __forceinline__ uint32_t tex_fetch_raw(TX t, const double* uv) {
    int x = iclamp(x86_cvttsd2si(uv[0] * t->w), 0, t->w - 1);
    int y = iclamp(x86_cvttsd2si(uv[1] * t->h), 0, t->h - 1);
    const uint8_t* p = t->data + ((size_t)x + (size_t)y * t->w) * t->bpp;
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
template <class TX>
__device__ __forceinline__ uint32_t tex_mask(TX t) { return t->bpp >= 4 ? 0xffffffffu : ((1u << (8 * t->bpp)) - 1u); }
template <class TX>
__device__ __forceinline__ Color tex_fetch(TX t, const double* uv) {
    return Color{ tex_fetch_raw(t, uv) & tex_mask(t), t->bpp };
}

// a / uz, correctly rounded, for the per-triangle constant uz with ruz = RN(1/uz) (Markstein):
// q0 = RN(a*ruz) is within 2 ulp of a/uz; one FMA residual step makes q1 faithful (error < 1 ulp),
// and for a faithful q1 the second step q1 + (a - uz*q1)*ruz rounds to RN(a/uz) exactly.
// Valid when nothing over/underflows: only used for "well scaled" triangles (see k_setup).
__device__ __forceinline__ double div_by_uz(double a, double uz, double ruz) {
    const double q0 = a * ruz;
    const double e0 = __builtin_fma(-q0, uz, a);
    const double q1 = __builtin_fma(e0, ruz, q0);
    const double e1 = __builtin_fma(-q1, uz, a);
    return __builtin_fma(e1, ruz, q1);
}

// The per-pixel prologue of the shade kernels, for pixel (x, y) whose owner's record r (TriRec) and 1/w (TriW rw) were read from
// the visibility buffer's id: barycentric() of our_gl.cpp:77-86 with exactly the operations of the scan (same bits), then the
// perspective correction of :168-185 into pc[3].  (A macro, not a function: an inlined function's control flow is simplified
// before it is inlined, and k_shade<PHONG|EYE> would no longer be, instruction for instruction, the kernels they were.)
#define TRGL_OWNER_BARYCENTRICS(r, rw, x, y, pc)                                                                       \
    do {                                                                                                               \
        const double pxc = (double)(x) + 0.5, pyc = (double)(y) + 0.5;                                                 \
        const double s0z = (r).ax - pxc, s1z = (r).ay - pyc;                                                           \
        const double ux = (r).s0y * s1z - s0z * (r).s1y;                                                               \
        const double uy = s0z * (r).s1x - (r).s0x * s1z;                                                               \
        const double us = ux + uy;                                                                                     \
        double b0, b1, b2;                                                                                             \
        if ((r).ruz != 0.0) {                                                                                          \
            b0 = 1.0 - trgl_shade::div_by_uz(us, (r).uz, (r).ruz); b1 = trgl_shade::div_by_uz(uy, (r).uz, (r).ruz);    \
            b2 = trgl_shade::div_by_uz(ux, (r).uz, (r).ruz);                                                           \
        } else {                                                                                                       \
            b0 = 1.0 - us / (r).uz; b1 = uy / (r).uz; b2 = ux / (r).uz;                                                \
        }                                                                                                              \
        const double denom = b0 * (rw).iw0 + b1 * (rw).iw1 + b2 * (rw).iw2;               /* our_gl.cpp:172-174 */     \
        if (fabs(denom) < 1e-15) { (pc)[0] = b0; (pc)[1] = b1; (pc)[2] = b2; }            /* :177-185 */               \
        else { (pc)[0] = (b0 * (rw).iw0) / denom; (pc)[1] = (b1 * (rw).iw1) / denom; (pc)[2] = (b2 * (rw).iw2) / denom; } \
    } while (0)

// TGAImage::set (tgaimage.cpp:32-39) of a packed colour; bpp is 1, 3 or 4 (trgl_create)
__device__ __forceinline__ void store_pixel(const FrameParams& fp, size_t idx, uint32_t color) {
    uint8_t* dst = fp.fb + idx * fp.bpp;
    if (fp.bpp == 3) { dst[0] = (uint8_t)color; dst[1] = (uint8_t)(color >> 8); dst[2] = (uint8_t)(color >> 16); }
    else if (fp.bpp == 4) *reinterpret_cast<uint32_t*>(dst) = color;
    else dst[0] = (uint8_t)color;
}

// Rows of a cleared tile without triangles: the clear values, row-contiguous (this is the whole kernel on a clear-only frame, the
// "framebuffer + z write-out" figure of BASELINE.json).  Wave w of the workgroup stores rows [py0 + 8 w, py0 + 8 w + 7].
__device__ __forceinline__ void clear_rows(const FrameParams& fp, int lane, int px0, int y0, int y1) {
    const int xa1 = min(px0 + TRGL_TILE - 1, fp.W - 1);
    const bool full_x = (px0 + TRGL_TILE - 1) <= xa1;
    // z: 16 B per lane, 4 rows per store instruction
    if (full_x && (fp.W & 1) == 0) {
        for (int r4 = 0; r4 < 8; r4 += 4) {
            const int x = px0 + ((lane & 15) << 1), y = y0 + r4 + (lane >> 4);
            if (y <= y1) {
                typedef double nt_d2 __attribute__((ext_vector_type(2)));
                nt_d2 nv = { fp.clear_z, fp.clear_z };
                __builtin_nontemporal_store(nv, reinterpret_cast<nt_d2*>(&fp.zb[(size_t)x + (size_t)y * fp.W]));
            }
        }
    } else {
        for (int r2 = 0; r2 < 8; r2 += 2) {
            const int x = px0 + (lane & 31), y = y0 + r2 + (lane >> 5);
            if (x <= xa1 && y <= y1) fp.zb[(size_t)x + (size_t)y * fp.W] = fp.clear_z;
        }
    }
    // colour: 4 pixels per lane (12 B for RGB, 16 B for RGBA), 8 rows per store instruction
    if (full_x && (fp.W & 3) == 0 && (fp.bpp == 3 || fp.bpp == 4)) {
        const int x = px0 + ((lane & 7) << 2), y = y0 + (lane >> 3);
        if (y <= y1) {
            const uint32_t c = fp.clear_color;
            const size_t idx = (size_t)x + (size_t)y * fp.W;
            if (fp.bpp == 4) {
                *reinterpret_cast<uint4*>(fp.fb + idx * 4) = make_uint4(c, c, c, c);
            } else {
                uint32_t* dst = reinterpret_cast<uint32_t*>(fp.fb + idx * 3);
                dst[0] = (c & 0xffffffu) | (c << 24); dst[1] = ((c >> 8) & 0xffffu) | (c << 16); dst[2] = ((c >> 16) & 0xffu) | (c << 8);
            }
        }
    } else {
        for (int r2 = 0; r2 < 8; r2 += 2) {
            const int x = px0 + (lane & 31), y = y0 + r2 + (lane >> 5);
            if (x <= xa1 && y <= y1) {
                const uint32_t c = fp.clear_color;
                uint8_t* dst = fp.fb + ((size_t)x + (size_t)y * fp.W) * fp.bpp;
                for (int i = 0; i < fp.bpp; ++i) dst[i] = (uint8_t)(c >> (8 * i));
            }
        }
    }
    if (fp.idbuf) {
        for (int r2 = 0; r2 < 8; r2 += 2) {
            const int x = px0 + (lane & 31), y = y0 + r2 + (lane >> 5);
            if (x <= xa1 && y <= y1) fp.idbuf[(size_t)x + (size_t)y * fp.W] = 0xffffffffu;
        }
    }
}

}  // namespace trgl_shade
