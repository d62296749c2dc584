// kernels_mip.hip — mip chains of images in HBM, the per-triangle level-of-detail constants, and the self-test of the filtered samplers
// (include/trgl.h, "Mipmapped textures": trgl_image_mipmaps, trgl_texture_mipmaps, trgl_lod_stage, trgl_selftest_sampler_lod), gfx950.
// New work, the reference has no mipmaps.  Every size, offset and rounding is mip_core.h's, which the host paths compile too.
//
//   k_mip_chain  Level l + k of a texel depends only on the 2^k-aligned block of level l, so a workgroup takes one MIP_TILE x MIP_TILE
//                block of a source level and leaves that block's part of the next MIP_STEP levels, without a byte of another block.
//     staging    the block's bytes, read once: a thread owns 16 consecutive bytes of a block row and reads the ALIGNED 16-byte word that
//                holds the first of them and, unless it sits at the word's start, the next word, and shifts the pair into place (a row
//                starts at any byte: bpp 3, odd widths, a caller's pointer).  The first word always holds a byte of the level; the second
//                is read only when it starts before the 16-byte boundary that ends the level.  One 16-byte LDS store per thread and word.
//     levels     level k of the block from level k - 1 in LDS, whole dwords at a time.  A thread takes one unit: 4 output bytes (bpp 1
//                and 4) or 6 (bpp 3: two texels), whose 8 or 12 source bytes per row are two or three aligned LDS dwords.  It adds the
//                two rows as packed 16-bit sums (even and odd bytes apart), adds the texel pairs, rounds, and leaves the unit in LDS for
//                level k + 1 as one dword or three 16-bit stores.  Behind the barrier the level goes out: four bytes that begin at a
//                4-byte boundary of the DESTINATION, funnel-shifted from the two LDS dwords that hold them, so whole groups leave as
//                aligned dwords and the ragged ends of a row as single bytes.  Nothing outside the level's bytes is written: padding
//                between levels, the zero tails of a slot and a caller's guard bytes survive.  One barrier per level (the store of
//                level k and the compute of level k + 1 both only read level k); a block's levels shrink by four each.
//     LDS        rows of level k lie (MIP_TILE >> k) * 4 bytes apart whatever bpp is: 21.4 KiB a workgroup, seven workgroups a CU.
//                Consecutive lanes read consecutive 8- or 12-byte units of a row and write consecutive dwords: no bank is hit twice
//                by a group of lanes except through the 12-byte stride of bpp 3 (two-way at worst).
//     launches   levels 1 .. MIP_STEP from level 0 in one launch, then one launch per further MIP_STEP levels from the last level
//                written (stream order); those are tiny.  A block the image's edge cuts has fewer texels at every level (none at all
//                once its first texel lies outside the level); a side of 1 stays 1 and is copied (fx or fy = 1).
//   k_lod_stage  one thread per triangle: 12 clip doubles and 6 uv doubles in, 4 doubles out, 8-byte accesses (nothing wider is assumed).
//   k_selftest_sampler_lod  the prelude's own functions (user_prelude.h) on given uv and lod, as a user shader would call them.
// No atomics.
#include <hip/hip_runtime.h>
#include "launch.h"
#include "mip_core.h"
#include "user_prelude.h"

namespace {

using namespace trgl;

constexpr int MIP_STEP = 6, MIP_TILE = 64, MIP_THREADS = 256;
static_assert(MIP_TILE == 1 << MIP_STEP, "a block shrinks to one texel in MIP_STEP levels");
constexpr int mip_lds_pitch(int k) { return (MIP_TILE >> k) * 4; }
// (+ 32: a unit or a shifted dword at the end of the last level's row reaches a few bytes past it; they hold nothing and stay in the array)
constexpr int mip_lds_bytes() { int o = 0; for (int k = 0; k <= MIP_STEP; ++k) o += mip_lds_pitch(k) * (MIP_TILE >> k); return ((o + 15) & ~15) + 32; }
constexpr int MIP_LDS = mip_lds_bytes();
static_assert(MIP_LDS <= 64 * 1024, "LDS");

struct MipArgs {
    const uint8_t* src; uint8_t* dst[MIP_STEP];      // the source level and the nlev levels behind it
    uintptr_t src_end16;                             // the 16-byte boundary at or behind the source level's last byte
    int32_t sw, sh, bpp, nlev, nbx;                  // the source level's size; blocks along x
};

// the 16 bytes at a (any address, a byte of the level) from one or two aligned 16-byte words
__device__ __forceinline__ uint4 load16_shifted(const uint8_t* a, uintptr_t end16) {
    const uint32_t p = (uint32_t)(uintptr_t)a & 15u;
    const uint4* wp = reinterpret_cast<const uint4*>(a - p);
    const uint4 A = wp[0];
    uint4 B = make_uint4(0, 0, 0, 0);
    if (p != 0 && (uintptr_t)(wp + 1) < end16) B = wp[1];
    const bool s8 = (p & 8u) != 0, s4 = (p & 4u) != 0;
    const uint32_t t0 = s8 ? A.z : A.x, t1 = s8 ? A.w : A.y, t2 = s8 ? B.x : A.z, t3 = s8 ? B.y : A.w, t4 = s8 ? B.z : B.x, t5 = s8 ? B.w : B.y;
    const uint32_t u0 = s4 ? t1 : t0, u1 = s4 ? t2 : t1, u2 = s4 ? t3 : t2, u3 = s4 ? t4 : t3, u4 = s4 ? t5 : t4;
    const uint32_t sh = (p & 3u) * 8u;
    return make_uint4(__funnelshift_r(u0, u1, sh), __funnelshift_r(u1, u2, sh), __funnelshift_r(u2, u3, sh), __funnelshift_r(u3, u4, sh));
}

// BPP: bytes per texel.  A unit of the compute step: `bytes` output bytes - whole texels - whose 2 * bytes source bytes per row are whole dwords.
template <int BPP> struct MipUnit { static constexpr int bytes = BPP == 3 ? 6 : 4, texels = bytes / BPP, src_dwords = bytes / 2; };

template <int BPP>
__global__ __launch_bounds__(MIP_THREADS) void k_mip_chain(MipArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[MIP_LDS];
    constexpr int U = MipUnit<BPP>::bytes, UT = MipUnit<BPP>::texels, ND = MipUnit<BPP>::src_dwords;
    const uint32_t tid = threadIdx.x;
    const int bx = (int)(blockIdx.x % (uint32_t)a.nbx), by = (int)(blockIdx.x / (uint32_t)a.nbx);
    const int x0 = bx * MIP_TILE, y0 = by * MIP_TILE;
    {   // the block of the source level: lh rows of lw * BPP bytes
        const int lw = min(MIP_TILE, a.sw - x0), lh = min(MIP_TILE, a.sh - y0);
        const size_t row = (size_t)a.sw * BPP;
        const uint32_t nwords = ((uint32_t)(lw * BPP) + 15u) >> 4;
        const uint8_t* base = a.src + (size_t)y0 * row + (size_t)x0 * BPP;
        for (uint32_t i = tid; i < (uint32_t)lh * nwords; i += MIP_THREADS) {
            const uint32_t r = i / nwords, k = i - r * nwords;
            *reinterpret_cast<uint4*>(lds + r * mip_lds_pitch(0) + k * 16) = load16_shifted(base + (size_t)r * row + (size_t)k * 16, a.src_end16);
        }
    }
    __syncthreads();
    int pw = a.sw, ph = a.sh;                        // the size of level k - 1
    int offP = 0;                                    // where its block lies in LDS
    for (int k = 1; k <= a.nlev; ++k) {
        const int fx = pw >= 2 ? 2 : 1, fy = ph >= 2 ? 2 : 1;
        const int cw = pw >= 2 ? pw >> 1 : 1, ch = ph >= 2 ? ph >> 1 : 1;
        const int tile = MIP_TILE >> k;              // >= 1
        const int cx0 = x0 >> k, cy0 = y0 >> k;
        const int clw = min(tile, cw - cx0), clh = min(tile, ch - cy0);
        if (clw <= 0 || clh <= 0) break;             // (uniform) no texel of this level, nor of a later one, belongs to the block
        const int pitchP = mip_lds_pitch(k - 1), pitchC = tile * 4;
        const int offC = offP + pitchP * (MIP_TILE >> (k - 1));
        const uint32_t nsum = (uint32_t)(fx * fy);
        {   // compute: a thread takes one unit - ND dwords of each source row - and leaves its U bytes in LDS.  Units per row are a power
            // of two (the tile's texels over UT); a unit the block's edge cuts makes bytes nobody reads, from bytes inside the array.
            const int ushift = 31 - __builtin_clz((unsigned)max(1, tile / UT));
            const uint32_t nunits = (uint32_t)(clw + UT - 1) / UT;
            for (uint32_t i = tid; i < ((uint32_t)clh << ushift); i += MIP_THREADS) {
                const uint32_t y = i >> ushift, u = i & ((1u << ushift) - 1u);
                if (u >= nunits) continue;
                const uint32_t* s0 = reinterpret_cast<const uint32_t*>(lds + offP + (y * (uint32_t)fy) * (uint32_t)pitchP + u * (2 * U));
                uint32_t v[4 * ND];                  // the vertical sums of the unit's 2 * U source bytes
#pragma unroll
                for (int j = 0; j < ND; ++j) {
                    const uint32_t d0 = s0[j];
                    uint32_t e = d0 & 0x00ff00ffu, o = (d0 >> 8) & 0x00ff00ffu;
                    if (fy == 2) { const uint32_t d1 = s0[j + pitchP / 4]; e += d1 & 0x00ff00ffu; o += (d1 >> 8) & 0x00ff00ffu; }
                    v[4 * j] = e & 0xffffu; v[4 * j + 1] = o & 0xffffu; v[4 * j + 2] = e >> 16; v[4 * j + 3] = o >> 16;
                }
                uint32_t out[U];
#pragma unroll
                for (int b = 0; b < U; ++b) {
                    const int first = (b / BPP) * 2 * BPP + b % BPP;      // the byte of texel 2 * (b / BPP), channel b % BPP
                    out[b] = mip_round(fx == 2 ? v[first] + v[first + BPP] : v[b], nsum);
                }
                uint8_t* c = lds + offC + y * (uint32_t)pitchC + u * U;
                if (U == 4) *reinterpret_cast<uint32_t*>(c) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
                else {
#pragma unroll
                    for (int b = 0; b < U; b += 2) *reinterpret_cast<uint16_t*>(c + b) = (uint16_t)(out[b] | (out[b + 1] << 8));
                }
            }
        }
        __syncthreads();
        {   // store: four bytes that begin at a 4-byte boundary of the destination, from the two LDS dwords that hold them
            const uint32_t nb = (uint32_t)(clw * BPP);
            const size_t crow = (size_t)cw * BPP;
            uint8_t* D = a.dst[k - 1] + (size_t)cy0 * crow + (size_t)cx0 * BPP;
            const uint32_t G = (nb + 6u) >> 2;       // groups of four bytes a row has at most, whatever its first byte's address
            const uint32_t gmagic = 65536u / G + 1u; // i / G for i < 65536 / G (here i < 32 * 33)
            for (uint32_t i = tid; i < (uint32_t)clh * G; i += MIP_THREADS) {
                const uint32_t y = (i * gmagic) >> 16, g = i - y * G;
                uint8_t* Dr = D + (size_t)y * crow;
                const int o0 = (int)(g * 4u) - (int)((uintptr_t)Dr & 3u);
                if (o0 >= (int)nb) continue;
                const uint32_t* cwords = reinterpret_cast<const uint32_t*>(lds + offC + y * (uint32_t)pitchC);
                const int q = o0 >> 2;               // -1 for the group that begins before the row: those bytes are not stored
                const uint32_t v = __funnelshift_r(cwords[q], cwords[q + 1], (uint32_t)(o0 & 3) * 8u);
                if (o0 >= 0 && o0 + 4 <= (int)nb) *reinterpret_cast<uint32_t*>(Dr + o0) = v;
                else {
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (o0 + m >= 0 && o0 + m < (int)nb) Dr[o0 + m] = (uint8_t)(v >> (8 * m));
                }
            }
        }
        pw = cw; ph = ch; offP = offC;
    }
}

struct LodArgs { double vp[8]; const double* clip; double* vary; uint32_t n; int32_t K, uv_off, out_off; };

__global__ __launch_bounds__(256) void k_lod_stage(LodArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n) return;
    double c[12], uv[6], out[4];
    const double* cp = a.clip + (size_t)t * 12;
    double* vp = a.vary + (size_t)t * (size_t)a.K;
#pragma unroll
    for (int i = 0; i < 12; ++i) c[i] = cp[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) uv[i] = vp[a.uv_off + i];
    mip_lod_constants(a.vp, c, uv, out);
#pragma unroll
    for (int i = 0; i < 4; ++i) vp[a.out_off + i] = out[i];
}

__global__ void k_selftest_sampler_lod(const DevTexture* __restrict__ tex, int slot, const double* __restrict__ uv, const double* __restrict__ lod,
                                       int mode, unsigned long long n, uint8_t* __restrict__ out) {
    const unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    trgl_frag_in in;
    in.bar[0] = in.bar[1] = in.bar[2] = 0.0; in.vary = nullptr; in.u = nullptr; in.color = 0; in.tex = tex; in.dst = 0;
    trgl_texel c;
    if (mode == 2) c = trgl_sample2D_trilinear(in, slot, uv + 2 * i, lod[i]);
    else if (mode == 1) c = trgl_sample2D_linear(in, slot, uv + 2 * i, mip_cvtt(lod[i]));
    else c = trgl_sample2D_level(in, slot, uv + 2 * i, mip_cvtt(lod[i]));
    for (int k = 0; k < 4; ++k) out[5 * i + k] = (uint8_t)(c.bgra >> (8 * k));
    out[5 * i + 4] = (uint8_t)c.bytespp;
}

}  // namespace

namespace trgl {

hipError_t launch_mip_chain(hipStream_t s, const uint8_t* level0, int w, int h, int bpp, uint8_t* chain, bool slot_layout) {
    const int L = mip_levels(w, h);
    for (int base = 0; base < L - 1; base += MIP_STEP) {
        auto off = [&](int l) { return slot_layout ? mip_slot_offset(w, h, bpp, l) : mip_packed_offset(w, h, bpp, l); };
        MipArgs a;
        a.src = base == 0 ? level0 : chain + off(base);
        a.sw = mip_side(w, base); a.sh = mip_side(h, base); a.bpp = bpp;
        a.nlev = L - 1 - base < MIP_STEP ? L - 1 - base : MIP_STEP;
        for (int k = 0; k < MIP_STEP; ++k) a.dst[k] = k < a.nlev ? chain + off(base + 1 + k) : nullptr;
        a.src_end16 = ((uintptr_t)a.src + (size_t)a.sw * a.sh * bpp + 15) & ~(uintptr_t)15;
        a.nbx = (a.sw + MIP_TILE - 1) / MIP_TILE;
        const int nby = (a.sh + MIP_TILE - 1) / MIP_TILE;
        const dim3 grid((unsigned)a.nbx * (unsigned)nby), block(MIP_THREADS);
        if (bpp == 4) hipLaunchKernelGGL(k_mip_chain<4>, grid, block, 0, s, a);
        else if (bpp == 3) hipLaunchKernelGGL(k_mip_chain<3>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_mip_chain<1>, grid, block, 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_lod_stage(hipStream_t s, const double viewport[16], const double* clip, double* vary, uint32_t n, int K, int uv_offset, int out_offset) {
    LodArgs a;
    for (int i = 0; i < 8; ++i) a.vp[i] = viewport[i];
    a.clip = clip; a.vary = vary; a.n = n; a.K = K; a.uv_off = uv_offset; a.out_off = out_offset;
    hipLaunchKernelGGL(k_lod_stage, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

void launch_selftest_sampler_lod(hipStream_t s, const DevTexture* tex, int slot, const double* uv, const double* lod, int mode, unsigned long long n, uint8_t* out) {
    if (n) hipLaunchKernelGGL(k_selftest_sampler_lod, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tex, slot, uv, lod, mode, n, out);
}

}  // namespace trgl
