// weld_core.h — the definitions of trgl_mesh_weld (include/trgl.h, "mesh welding") as the functions that the host loop (trgl_host.cpp)
// and the kernels (kernels_weld.hip) both compile: the compared value q of a key component, the comparison of two keys and the hash
// that brings identical keys together.
// fp64, every operation rounded, contraction off, IEEE division.  No double computed here is stored: only comparisons and hashes leave.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/trgl.h"

#if defined(__HIP__)
#define TRGL_WELD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRGL_WELD_HD inline
#endif

namespace trgl {

constexpr uint32_t WELD_NONE = 0xFFFFFFFFu;      // a firsts_out word behind the last vertex; indices_out of an index that names no vertex

// the compared value of a key component x: x itself, or the number of its grid cell
TRGL_WELD_HD double weld_q(double x, double cell) {
    if (cell == 0.0) return x;
    const double t = x / cell;
    const double s = t + 0.5;
    return floor(s);
}

// the keys of the records ru and rv (their first doubles) are identical: IEEE == on every component's q
TRGL_WELD_HD bool weld_identical(const double* ru, const double* rv, int key_offset, int key_count, double cell) {
    for (int a = 0; a < key_count; ++a)
        if (!(weld_q(ru[key_offset + a], cell) == weld_q(rv[key_offset + a], cell))) return false;
    return true;
}

TRGL_WELD_HD uint64_t weld_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The hash of a record's key: over the 64 bits of every q, a zero of either sign as +0.0 - what == takes for equal hashes alike.  (A
// key with a NaN is identical to nothing, so what it hashes to decides nothing.)
TRGL_WELD_HD uint64_t weld_hash(const double* r, int key_offset, int key_count, double cell) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int a = 0; a < key_count; ++a) {
        const double q = weld_q(r[key_offset + a], cell);
        uint64_t w = 0;
        if (!(q == 0.0)) memcpy(&w, &q, sizeof(w));
        h = weld_mix(h ^ w) + 0x9E3779B97F4A7C15ull;
    }
    return h;
}

// the low `bits` bits of a hash (0 .. 64): what the device path sorts by (trgl_debug_weld_hash_bits)
TRGL_WELD_HD uint64_t weld_hash_low(uint64_t h, int bits) { return bits >= 64 ? h : (bits <= 0 ? 0ull : h & ((1ull << bits) - 1ull)); }

}  // namespace trgl
