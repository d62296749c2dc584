// lod_core.h — the definitions of trgl_mesh_clean and trgl_mesh_simplify (include/trgl.h, "mesh levels of detail") as the functions
// that the host loops (trgl_host.cpp) and the kernels (kernels_lod.hip) both compile: the class of a face, its canonical triple, the hash
// that brings equal triples together and the arithmetic of a cell's mean.
// fp64, every operation rounded, contraction off, IEEE division.
#pragma once
#include <stdint.h>

#include "weld_core.h"

namespace trgl {

constexpr uint32_t LOD_NONE = 0xFFFFFFFFu;

enum LodFaceClass : uint32_t { LOD_FACE_CANDIDATE = 0, LOD_FACE_INVALID = 1, LOD_FACE_DEGENERATE = 2 };

// invalid: an index that names no vertex (compared before any index becomes an address); degenerate: two equal indices; else a candidate,
// which is kept unless an earlier candidate has its canonical triple
TRGL_WELD_HD uint32_t lod_face_class(uint32_t a, uint32_t b, uint32_t c, uint32_t n_vertices) {
    if (a >= n_vertices || b >= n_vertices || c >= n_vertices) return LOD_FACE_INVALID;
    if (a == b || b == c || c == a) return LOD_FACE_DEGENERATE;
    return LOD_FACE_CANDIDATE;
}

// the rotation of (a, b, c) that puts the smallest index first: orientation kept, so a mirrored face has another triple
struct LodTriple { uint32_t x, y, z; };
TRGL_WELD_HD LodTriple lod_canonical(uint32_t a, uint32_t b, uint32_t c) {
    if (a <= b && a <= c) return LodTriple{ a, b, c };
    if (b <= a && b <= c) return LodTriple{ b, c, a };
    return LodTriple{ c, a, b };
}
TRGL_WELD_HD bool lod_same_triple(const LodTriple& p, const LodTriple& q) { return p.x == q.x && p.y == q.y && p.z == q.z; }

// the hash of a canonical triple
TRGL_WELD_HD uint64_t lod_face_hash(const LodTriple& t) {
    uint64_t h = weld_mix(0x9E3779B97F4A7C15ull ^ (((uint64_t)t.x << 32) | (uint64_t)t.y)) + 0x9E3779B97F4A7C15ull;
    return weld_mix(h ^ (uint64_t)t.z);
}
// what a face that is no candidate sorts by: it is identical to nothing, so its own number spreads it over the runs
TRGL_WELD_HD uint64_t lod_dropped_hash(uint32_t face) { return weld_mix(~(uint64_t)face); }

// The mean of a cell: s starts as the first referenced member's value, the others are added in ascending old number, each sum rounded;
// then one IEEE division by the count (count >= 2: a single member keeps its bits and is never divided).
TRGL_WELD_HD double lod_mean_add(double s, double x) { return s + x; }
TRGL_WELD_HD double lod_mean_div(double s, uint32_t count) { return s / (double)count; }

}  // namespace trgl
