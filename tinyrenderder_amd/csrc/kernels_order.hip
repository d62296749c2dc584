// kernels_order.hip — depths of instances and the order to draw them in (include/trgl.h: trgl_instance_depths, trgl_depth_order), gfx950.
//
//   k_instance_depths : one thread per instance: row 2 of model_view * M_i (geometry.h:196-205), then its dot<4> with (point, 1)
//                       (geometry.h:123-127) - the dot4 calls k_inst_scatter makes for MV_i, for the one row that is needed (it takes all 16
//                       elements of M_i: 128 bytes read and 8 written per instance).
//   k_order_keys      : one thread per depth: the 64 bits of the double turned into an unsigned key that ascends with the order the
//                       header defines (sign bit set: all bits flipped; clear: the sign bit set), complemented for front to back, and
//                       the entry's own number beside it.
//   the sort          : hipcub::DeviceRadixSort::SortPairs over all 64 bits of those keys - least significant digit first, stable, so
//                       equal keys keep ascending numbers in either direction.  Integers only: no comparison of doubles takes part.
// fp64 in the reference's operation order, contraction off.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "launch.h"
#include "device_util.h"

namespace {

using trgl_dev::dot4;

struct DepthArgs { double row[4]; double point[3]; };      // row 2 of model_view; the mesh's point in model space

__global__ __launch_bounds__(256) void k_instance_depths(DepthArgs a, const double* __restrict__ instances, int inst_stride, uint32_t n,
                                                         double* __restrict__ depths) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* M = instances + (size_t)i * (size_t)inst_stride;
    double m[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = M[e];
    double r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = dot4(a.row, m[c], m[4 + c], m[8 + c], m[12 + c]);
    depths[i] = dot4(r, a.point[0], a.point[1], a.point[2], 1.0);
}

__global__ __launch_bounds__(256) void k_order_keys(const unsigned long long* __restrict__ depth_bits, uint32_t n, unsigned long long flip,
                                                    unsigned long long* __restrict__ keys, uint32_t* __restrict__ numbers) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = depth_bits[i];
    keys[i] = (b ^ ((b >> 63) ? ~0ull : 1ull << 63)) ^ flip;
    numbers[i] = i;
}

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

struct Carve { unsigned long long* keys; unsigned long long* sorted_keys; uint32_t* numbers; size_t sort_off; };
Carve carve(void* scratch, uint32_t n) {
    char* p = (char*)scratch;
    Carve c;
    size_t off = 0;
    c.keys = (unsigned long long*)(p + off); off += align256((size_t)n * sizeof(unsigned long long));
    c.sorted_keys = (unsigned long long*)(p + off); off += align256((size_t)n * sizeof(unsigned long long));
    c.numbers = (uint32_t*)(p + off); off += align256((size_t)n * sizeof(uint32_t));
    c.sort_off = off;
    return c;
}

hipError_t sort_keys(void* tmp, size_t& tmp_bytes, const Carve& c, uint32_t n, uint32_t* order, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const unsigned long long*)c.keys, c.sorted_keys, (const uint32_t*)c.numbers, order,
                                              (size_t)n, 0, 64, s);
}

}  // namespace

namespace trgl {

void launch_instance_depths(hipStream_t s, const double model_view[16], const double point[3], const double* instances, int inst_stride,
                            uint32_t n, double* depths) {
    DepthArgs a;
    for (int e = 0; e < 4; ++e) a.row[e] = model_view[8 + e];
    for (int e = 0; e < 3; ++e) a.point[e] = point[e];
    hipLaunchKernelGGL(k_instance_depths, dim3((n + 255) / 256), dim3(256), 0, s, a, instances, inst_stride, n, depths);
}

hipError_t depth_order_scratch_bytes(uint32_t n, size_t* bytes) {
    const Carve c = carve(nullptr, n);
    size_t tmp = 0;
    const hipError_t e = sort_keys(nullptr, tmp, c, n, nullptr, nullptr);
    if (e != hipSuccess) return e;
    *bytes = c.sort_off + align256(tmp);
    return hipSuccess;
}

hipError_t launch_depth_order(hipStream_t s, const double* depths, uint32_t n, bool front_to_back, void* scratch, size_t scratch_bytes,
                              uint32_t* order) {
    const Carve c = carve(scratch, n);
    if (scratch_bytes < c.sort_off) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_order_keys, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(depths), n,
                       front_to_back ? ~0ull : 0ull, c.keys, c.numbers);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tmp = scratch_bytes - c.sort_off;
    return sort_keys((char*)scratch + c.sort_off, tmp, c, n, order, s);
}

}  // namespace trgl
