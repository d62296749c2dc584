// kernels_selftest.hip — device self-tests (trgl_selftest_division, trgl_selftest_sampler): the two exactness shortcuts of the pixel
// loop against the hardware's IEEE division, and the samplers' index math on given uv.
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "shade_common.h"

namespace {
using namespace trgl_shade;

// ---- self-test of the two exactness shortcuts, against the hardware's IEEE division ------------------
__device__ __forceinline__ unsigned long long sm64(unsigned long long& st) {
    unsigned long long z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double mk_double(unsigned long long mant, int exp2, bool neg) {
    unsigned long long bits = (mant & 0x000fffffffffffffull) | ((unsigned long long)(exp2 + 1023) << 52) | (neg ? 0x8000000000000000ull : 0ull);
    return __longlong_as_double((long long)bits);
}
__global__ void k_selftest_division(unsigned long long n_per_thread, unsigned long long seed, unsigned long long* mismatches) {
    unsigned long long st = seed + 0x1000003ull * (blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x);
    unsigned long long bad = 0;
    for (unsigned long long it = 0; it < n_per_thread; ++it) {
        unsigned long long r0 = sm64(st), r1 = sm64(st), r2 = sm64(st);
        int mode = (int)(r2 & 7);
        int eb = (int)((r2 >> 8) % 440) - 40;           // |uz| in [2^-40, 2^400): the well-scaled range
        int ea = (int)((r2 >> 24) % 700) - 350;
        unsigned long long mb = r1;
        if (mode == 1) mb = 0x000fffffffffffffull;                       // all-ones significand
        if (mode == 2) mb = 0x000fffffffffffffull ^ (1ull << (r1 % 52));  // one zero bit
        if (mode == 3) mb = 0;                                           // power of two
        double uz = mk_double(mb, eb, true);                             // u.z < 0
        double a = mk_double(r0, ea, (r2 >> 40) & 1);
        if (mode >= 4 && mode <= 6) {
            // numerator chosen so that a/uz lies next to a rounding midpoint: a = RN(uz * (q + ulp(q)/2 * (1 +- tiny)))
            double q = mk_double(r0, ea - eb, (r2 >> 41) & 1);
            double half_ulp = mk_double(0, ea - eb - 53, false);
            a = __builtin_fma(uz, q, uz * half_ulp);
            if (mode == 5) a = __longlong_as_double(__double_as_longlong(a) + 1);
            if (mode == 6) a = __longlong_as_double(__double_as_longlong(a) - 1);
        }
        if (mode == 7) a = (r2 >> 42) & 1 ? 0.0 : -0.0;
        double ruz = 1.0 / uz;
        double ref = a / uz, got = div_by_uz(a, uz, ruz);
        if (__double_as_longlong(ref) != __double_as_longlong(got)) ++bad;
        // sign shortcuts of the coverage test
        if ((ref < 0) != (a > 0.0)) ++bad;
        if (((1.0 - ref) < 0) != (a < uz)) ++bad;
        // numerator right next to uz, where 1 - q changes sign
        double a2 = __longlong_as_double(__double_as_longlong(uz) + (long long)(r1 % 5) - 2);
        double ref2 = a2 / uz;
        if (__double_as_longlong(ref2) != __double_as_longlong(div_by_uz(a2, uz, ruz))) ++bad;
        if (((1.0 - ref2) < 0) != (a2 < uz)) ++bad;
    }
    if (bad) atomicAdd(mismatches, bad);
}

// ---- self-test of the samplers' index math: tex_fetch on given uv (the fixtures come from the compiled reference's
// IShader::sample2D, tests/golden/sampler_golden.npz) ---------------------------------------------------------------
__global__ void k_selftest_sampler(const DevTexture* __restrict__ tex, int slot, const double* __restrict__ uv, unsigned long long n,
                                   uint8_t* __restrict__ out) {
    const unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevTexture* t = tex_slot(tex, slot);
    Color c = t ? tex_fetch(t, uv + 2 * i) : Color{ 0xffffffffu, 4 };        // a missing map samples as opaque white (model.cpp:416-418)
    for (int k = 0; k < 4; ++k) out[5 * i + k] = (uint8_t)(c.bgra >> (8 * k));
    out[5 * i + 4] = (uint8_t)c.bytespp;
}

}  // namespace

namespace trgl {

void launch_selftest_division(hipStream_t s, unsigned long long n_per_thread, unsigned long long seed, unsigned long long* mismatches) {
    hipLaunchKernelGGL(k_selftest_division, dim3(1024), dim3(256), 0, s, n_per_thread, seed, mismatches);
}

void launch_selftest_sampler(hipStream_t s, const DevTexture* tex, int slot, const double* uv, unsigned long long n, uint8_t* out) {
    if (n) hipLaunchKernelGGL(k_selftest_sampler, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tex, slot, uv, n, out);
}

}  // namespace trgl
