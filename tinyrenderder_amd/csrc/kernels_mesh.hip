// kernels_mesh.hip — Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388) for an
// indexed mesh in HBM, in place and bit for bit.
//
// The reference adds a face's vector to its three vertices face by face, so the sum at a vertex is a serial chain of fp64 additions in
// corner order (corner = 3 * face + k) that starts at +0.0.  fp64 addition is not associative: a scatter with atomics, or any reduction
// in the order the GPU happens to schedule, gives other bits.  Here every chain is walked by one thread in the reference's order:
//   1. k_mesh_need         any vertex with norm(field) < 0.001?  (an OR: order-free, one integer atomic per block)
//   2. k_face_vectors      one thread per face: its vector (and for tangents its skip flag) to scratch - computed once, not three
//                          times - and the corner numbers 3f, 3f + 1, 3f + 2
//   3. a stable sort of the corner numbers by indices[corner] (hipcub radix sort over the bits n_vertices - 1 needs: integers only)
//   4. k_vertex_finish     one thread per vertex: lower bound of its number in the sorted keys, then its corners front to back, each
//                          face vector added to a sum that starts at +0.0; the per-vertex finish; plain stores
// Kernels 2 and 4 read the flag of kernel 1 and leave when nothing is needed: the host never looks at it.  The sort between them is
// the library's and runs either way, on scratch only.
// What the reference sums into Vertex::bitangent (model.cpp:359,365-367) is overwritten at every vertex by :381 or :385 before anything
// reads it, so it is not computed here.
//
// Also Model::computeAABB (model.cpp:15-40) over the vertices of such a mesh: k_mesh_bounds + k_mesh_bounds_fold, at the end of the file.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "launch.h"

namespace {

// dot<3> summed from 0 in component order, then sqrt (geometry.h:123-133)
__device__ __forceinline__ double norm3(const double (&v)[3]) {
    double sum = 0;
    sum += v[0] * v[0]; sum += v[1] * v[1]; sum += v[2] * v[2];
    return sqrt(sum);
}
// normalized (geometry.h:136-140): a zero vector comes back unchanged
__device__ __forceinline__ void normalize3(double (&v)[3]) {
    const double length = norm3(v);
    if (length == 0) return;
    v[0] = v[0] / length; v[1] = v[1] / length; v[2] = v[2] / length;
}

// Grid-stride over the vertices, four vertices = twelve independent 8-byte loads in flight per thread (records are only 8-byte
// aligned: no wider loads).  A vertex past the end stands as (1, 0, 0), which needs nothing; a NaN length compares false.
constexpr int MA_UNROLL = 4;
__global__ __launch_bounds__(256) void k_mesh_need(const double* __restrict__ vertices, int stride, int field, uint64_t n, uint32_t* __restrict__ flag) {
    bool need = false;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += MA_UNROLL * step) {
        double p[MA_UNROLL][3];
#pragma unroll
        for (int u = 0; u < MA_UNROLL; ++u) {
            const uint64_t j = i + u * step;
            const double* rec = vertices + (j < n ? j : i) * (uint64_t)stride + field;
#pragma unroll
            for (int a = 0; a < 3; ++a) p[u][a] = j < n ? rec[a] : (a == 0 ? 1.0 : 0.0);
        }
#pragma unroll
        for (int u = 0; u < MA_UNROLL; ++u) need |= norm3(p[u]) < 0.001;                    // model.cpp:272 / :321
    }
    if (__syncthreads_or(need) && threadIdx.x == 0) atomicOr(flag, 1u);
}

// One thread per face.  fvec[3f..3f+2]: cross(v1 - v0, v2 - v0) (model.cpp:293-299), or the face's tangent (:347-358) with
// skip[f] = fabs(r) < 1e-8 (:354; false for a NaN r).  A skipped face's vector is still stored; nothing reads it.
template <bool TANGENTS>
__global__ __launch_bounds__(256) void k_face_vectors(const double* __restrict__ vertices, int stride, const uint32_t* __restrict__ indices, uint32_t nfaces,
                                                      const uint32_t* __restrict__ flag, double* __restrict__ fvec, uint8_t* __restrict__ skip,
                                                      uint32_t* __restrict__ corners) {
    if (!*flag) return;
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nfaces) return;
    const double* r0 = vertices + (uint64_t)indices[3 * f] * (uint64_t)stride;
    const double* r1 = vertices + (uint64_t)indices[3 * f + 1] * (uint64_t)stride;
    const double* r2 = vertices + (uint64_t)indices[3 * f + 2] * (uint64_t)stride;
    double e1[3], e2[3], out[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double p0 = r0[a]; e1[a] = r1[a] - p0; e2[a] = r2[a] - p0; }
    if (TANGENTS) {
        const double u0 = r0[6], v0 = r0[7];
        const double duv1x = r1[6] - u0, duv1y = r1[7] - v0, duv2x = r2[6] - u0, duv2y = r2[7] - v0;   // :350-351
        const double r = duv1x * duv2y - duv2x * duv1y;                                     // :353
        skip[f] = fabs(r) < 1e-8;                                                           // :354
        const double invr = 1.0 / r;                                                        // :356
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = (e1[a] * duv2y - e2[a] * duv1y) * invr;        // :358
    } else {
        out[0] = e1[1] * e2[2] - e1[2] * e2[1];                                             // geometry.h:143-149
        out[1] = e1[2] * e2[0] - e1[0] * e2[2];
        out[2] = e1[0] * e2[1] - e1[1] * e2[0];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) fvec[3 * f + a] = out[a];
#pragma unroll
    for (int k = 0; k < 3; ++k) corners[3 * f + k] = (uint32_t)(3 * f + k);
}

// One thread per vertex (grid-stride).  keys: indices[corner] in stable sorted order, sorted_corners: the corner of each.  The chain of
// additions at a vertex is serial by definition: a segment is never split across lanes; four corners' loads are in flight at a time
// and their vectors are then added in order.
constexpr int VF_UNROLL = 4;
template <bool TANGENTS>
__global__ __launch_bounds__(256) void k_vertex_finish(double* __restrict__ vertices, int stride, uint64_t nverts, const uint32_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ sorted_corners, uint64_t ncorners, const double* __restrict__ fvec,
                                                       const uint8_t* __restrict__ skip, const uint32_t* __restrict__ flag) {
    if (!*flag) return;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nverts; v += step) {
        uint64_t lo = 0, hi = ncorners;                                     // the first corner of vertex v, or where it would be
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint64_t)keys[mid] < v) lo = mid + 1; else hi = mid;
        }
        double sum[3] = { 0.0, 0.0, 0.0 };                                  // model.cpp:284 / :333: the chain starts at +0.0
        bool more = true;
        for (uint64_t j = lo; more && j < ncorners; j += VF_UNROLL) {
            bool live[VF_UNROLL];
            double fv[VF_UNROLL][3];
#pragma unroll
            for (int u = 0; u < VF_UNROLL; ++u) {
                const bool in = j + u < ncorners;
                const uint64_t jc = in ? j + u : j;
                more = more && in && (uint64_t)keys[jc] == v;
                live[u] = more;
                const uint64_t f = sorted_corners[jc] / 3;
                if (TANGENTS) live[u] = more && !skip[f];                   // :354 `continue`
#pragma unroll
                for (int a = 0; a < 3; ++a) fv[u][a] = fvec[3 * f + a];
            }
#pragma unroll
            for (int u = 0; u < VF_UNROLL; ++u)
                if (live[u]) { sum[0] = sum[0] + fv[u][0]; sum[1] = sum[1] + fv[u][1]; sum[2] = sum[2] + fv[u][2]; }   // :302-304 / :361-363
        }
        double* rec = vertices + v * (uint64_t)stride;
        if (TANGENTS) {
            double normal[3] = { rec[3], rec[4], rec[5] };
            double tangent[3] = { 1, 0, 0 }, bitangent[3] = { 0, 1, 0 };    // :384-385
            if (norm3(sum) > 0.001 && norm3(normal) > 0.001) {              // :372
                double n[3] = { normal[0], normal[1], normal[2] };
                normalize3(n);                                              // :374
                normalize3(sum);                                            // :375
                double d = 0;
                d += n[0] * sum[0]; d += n[1] * sum[1]; d += n[2] * sum[2];
#pragma unroll
                for (int a = 0; a < 3; ++a) tangent[a] = sum[a] - n[a] * d; // :378
                normalize3(tangent);
                bitangent[0] = normal[1] * tangent[2] - normal[2] * tangent[1];             // :381: the stored normal, not n
                bitangent[1] = normal[2] * tangent[0] - normal[0] * tangent[2];
                bitangent[2] = normal[0] * tangent[1] - normal[1] * tangent[0];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) { rec[8 + a] = tangent[a]; rec[11 + a] = bitangent[a]; }
        } else {
            const double length = norm3(sum);
            if (length > 0.001) { sum[0] = sum[0] / length; sum[1] = sum[1] / length; sum[2] = sum[2] / length; }   // :309-310 (length != 0)
            else { sum[0] = 0; sum[1] = 0; sum[2] = 1; }                    // :313
#pragma unroll
            for (int a = 0; a < 3; ++a) rec[3 + a] = sum[a];
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
// bits of the largest vertex number (at least 1, at most 32: an index has no more)
int key_bits(uint64_t nverts) {
    const uint64_t top = nverts - 1 > 0xffffffffull ? 0xffffffffull : nverts - 1;
    int bits = 1;
    while (bits < 32 && (top >> bits)) ++bits;
    return bits;
}

struct Carve { uint32_t* flag; double* fvec; uint32_t* corners; uint32_t* keys; uint32_t* sorted_corners; uint8_t* skip; size_t sort_off; };
Carve carve(void* scratch, uint32_t nfaces) {
    char* p = (char*)scratch;
    const size_t nc = 3 * (size_t)nfaces;
    Carve c;
    size_t off = 0;
    c.flag = (uint32_t*)(p + off); off += 256;
    c.fvec = (double*)(p + off); off += align256(nc * sizeof(double));
    c.corners = (uint32_t*)(p + off); off += align256(nc * sizeof(uint32_t));
    c.keys = (uint32_t*)(p + off); off += align256(nc * sizeof(uint32_t));
    c.sorted_corners = (uint32_t*)(p + off); off += align256(nc * sizeof(uint32_t));
    c.skip = (uint8_t*)(p + off); off += align256(nfaces);
    c.sort_off = off;
    return c;
}

hipError_t sort_corners(void* tmp, size_t& tmp_bytes, const uint32_t* indices, const Carve& c, uint32_t nfaces, uint64_t nverts, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, indices, c.keys, (const uint32_t*)c.corners, c.sorted_corners,
                                              3 * (size_t)nfaces, 0, key_bits(nverts), s);
}

// ---- Model::computeAABB (model.cpp:15-40) ---------------------------------------------------------------------------
// The reference's loop is `min = std::min(min, p)` = (p < min) ? p : min and `max = std::max(max, p)` = (max < p) ? p : max from
// 1e9 / -1e9: a NaN never replaces a bound, and of two values that compare equal - only +0.0 and -0.0 differ in bits - the one met
// first stays.  So a bound is the first vertex, in vertex order, that holds the smallest (largest) value: the reduction carries
// (value, vertex index) and prefers the lower index among equal values, which makes it associative and commutative - the result is
// the sequential loop's whatever the order in which lanes, waves and blocks are combined.  The start value carries the index ~0:
// a vertex that equals it has the same bits.  Slots 0..2 are minima, 3..5 maxima.
using trgl::BoundsPartial;
__device__ __forceinline__ bool bounds_better(int k, double vb, unsigned long long ib, double va, unsigned long long ia) {
    return (k < 3 ? vb < va : vb > va) || (vb == va && ib < ia);
}

// wave (xor butterfly: every lane ends with the same six pairs), then the block's four waves through LDS; the result is thread 0's
__device__ __forceinline__ void bounds_block_reduce(double (&v)[6], unsigned long long (&ix)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int o = 32; o; o >>= 1) {
            const double ov = __shfl_xor(v[k], o);
            const unsigned long long oi = __shfl_xor(ix[k], o);
            if (bounds_better(k, ov, oi, v[k], ix[k])) { v[k] = ov; ix[k] = oi; }
        }
    __shared__ double s_v[4][6];
    __shared__ unsigned long long s_i[4][6];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { s_v[threadIdx.x >> 6][k] = v[k]; s_i[threadIdx.x >> 6][k] = ix[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (bounds_better(k, s_v[w][k], s_i[w][k], v[k], ix[k])) { v[k] = s_v[w][k]; ix[k] = s_i[w][k]; }
    }
}

// Grid-stride over the vertices, four vertices = twelve independent 8-byte loads in flight per thread (positions are only 8-byte
// aligned: no wider loads).  A thread meets its vertices in rising order, so `<` alone keeps the first among equals here; a vertex
// past the end stands as NaN, which replaces nothing.  partials[blockIdx.x] leaves with plain stores: no atomics, no ordering
// between blocks.
constexpr int MB_UNROLL = 4;
__global__ __launch_bounds__(256) void k_mesh_bounds(const double* __restrict__ vertices, int stride, uint64_t n, BoundsPartial* __restrict__ partials) {
    double v[6] = { 1e9, 1e9, 1e9, -1e9, -1e9, -1e9 };                                  // model.cpp:21-22
    unsigned long long ix[6] = { ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull };
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += MB_UNROLL * step) {
        double p[MB_UNROLL][3];
#pragma unroll
        for (int u = 0; u < MB_UNROLL; ++u) {
            const uint64_t j = i + u * step;
            const double* rec = vertices + (j < n ? j : i) * (uint64_t)stride;
#pragma unroll
            for (int a = 0; a < 3; ++a) p[u][a] = j < n ? rec[a] : __builtin_nan("");
        }
#pragma unroll
        for (int u = 0; u < MB_UNROLL; ++u) {
            const uint64_t j = i + u * step;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (p[u][a] < v[a]) { v[a] = p[u][a]; ix[a] = j; }                      // :25-27
                if (v[3 + a] < p[u][a]) { v[3 + a] = p[u][a]; ix[3 + a] = j; }          // :29-31
            }
        }
    }
    bounds_block_reduce(v, ix);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { partials[blockIdx.x].v[k] = v[k]; partials[blockIdx.x].i[k] = ix[k]; }
    }
}

// one block: folds the partials and applies the margin once (model.cpp:35-36); out->v = min x, y, z, max x, y, z of localAABB
__global__ __launch_bounds__(256) void k_mesh_bounds_fold(const BoundsPartial* __restrict__ partials, uint32_t nparts, BoundsPartial* __restrict__ out) {
    double v[6] = { 1e9, 1e9, 1e9, -1e9, -1e9, -1e9 };
    unsigned long long ix[6] = { ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull };
    for (uint32_t b = threadIdx.x; b < nparts; b += 256)
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (bounds_better(k, partials[b].v[k], partials[b].i[k], v[k], ix[k])) { v[k] = partials[b].v[k]; ix[k] = partials[b].i[k]; }
    bounds_block_reduce(v, ix);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double margin = (v[3 + a] - v[a]) * 0.01;                             // :35
            out->v[a] = v[a] - margin; out->v[3 + a] = v[3 + a] + margin;               // :36
            out->i[a] = ix[a]; out->i[3 + a] = ix[3 + a];
        }
    }
}

}  // namespace

namespace trgl {

hipError_t mesh_attr_scratch_bytes(uint64_t nverts, uint32_t nfaces, size_t* bytes) {
    const Carve c = carve(nullptr, nfaces);
    size_t tmp = 0;
    if (nfaces) {
        const hipError_t e = sort_corners(nullptr, tmp, nullptr, c, nfaces, nverts, nullptr);
        if (e != hipSuccess) return e;
    }
    *bytes = c.sort_off + align256(tmp);
    return hipSuccess;
}

hipError_t launch_mesh_attr(hipStream_t s, bool tangents, double* vertices, int stride, uint64_t nverts, const uint32_t* indices, uint32_t nfaces,
                            void* scratch, size_t scratch_bytes, const uint32_t** flag) {
    const Carve c = carve(scratch, nfaces);
    *flag = c.flag;
    hipError_t e = hipMemsetAsync(c.flag, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint64_t per_block = 256ull * MA_UNROLL;
    const uint64_t want = (nverts + per_block - 1) / per_block;
    hipLaunchKernelGGL(k_mesh_need, dim3((uint32_t)(want < 2048 ? want : 2048)), dim3(256), 0, s, vertices, stride, tangents ? 8 : 3, nverts, c.flag);
    if (nfaces) {
        const dim3 fgrid((uint32_t)(((uint64_t)nfaces + 255) / 256));
        if (tangents) hipLaunchKernelGGL(k_face_vectors<true>, fgrid, dim3(256), 0, s, vertices, stride, indices, nfaces, c.flag, c.fvec, c.skip, c.corners);
        else hipLaunchKernelGGL(k_face_vectors<false>, fgrid, dim3(256), 0, s, vertices, stride, indices, nfaces, c.flag, c.fvec, c.skip, c.corners);
        size_t tmp = scratch_bytes - c.sort_off;
        e = sort_corners((char*)scratch + c.sort_off, tmp, indices, c, nfaces, nverts, s);
        if (e != hipSuccess) return e;
    }
    const uint64_t vblocks = (nverts + 255) / 256;
    const dim3 vgrid((uint32_t)(vblocks < (1u << 20) ? vblocks : (1u << 20)));
    const uint64_t ncorners = 3 * (uint64_t)nfaces;
    if (tangents) hipLaunchKernelGGL(k_vertex_finish<true>, vgrid, dim3(256), 0, s, vertices, stride, nverts, c.keys, c.sorted_corners, ncorners, c.fvec, c.skip, c.flag);
    else hipLaunchKernelGGL(k_vertex_finish<false>, vgrid, dim3(256), 0, s, vertices, stride, nverts, c.keys, c.sorted_corners, ncorners, c.fvec, c.skip, c.flag);
    return hipGetLastError();
}

void launch_mesh_bounds(hipStream_t s, const double* vertices, int stride, uint64_t n, BoundsPartial* scratch) {
    const uint64_t per_block = 256ull * MB_UNROLL;
    const uint64_t want = (n + per_block - 1) / per_block;
    const uint32_t blocks = (uint32_t)(want < MESH_BOUNDS_MAX_BLOCKS ? want : MESH_BOUNDS_MAX_BLOCKS);
    hipLaunchKernelGGL(k_mesh_bounds, dim3(blocks), dim3(256), 0, s, vertices, stride, n, scratch + 1);
    hipLaunchKernelGGL(k_mesh_bounds_fold, dim3(1), dim3(256), 0, s, scratch + 1, blocks, scratch);
}

}  // namespace trgl
