// kernels_scene.hip — world boxes of instances and frustum codes of boxes (include/trgl.h: trgl_instance_boxes, trgl_frustum_boxes), gfx950.
//
//   k_instance_boxes : one thread per instance: AABB::transform (geometry.h:297-327) of the instance's local box under its matrix -
//                      the 16 doubles of M_i (128 contiguous bytes at a stride of inst_stride * 8, as k_instance_depths reads them) and,
//                      with a strided local array, 6 more; 48 bytes written.  A lane's 128 bytes are one or two cache lines that no other
//                      lane needs, so staging a block's matrices through LDS would change the order the lines are asked for, not their
//                      number; the simple form is kept (profiles/instance_cull_probe_summary.txt has its time against a copy).
//   k_frustum_boxes  : one thread per box: Frustum::intersects (our_gl.cpp:264-280) of 48 bytes against the six planes of the kernel
//                      argument, then the lane's own code byte.  SET stores VISIBLE or OUTSIDE; MERGE stores OUTSIDE where the box is
//                      culled and touches nothing else, so a kept byte is neither read nor written.
// Both bodies are scene_core.h's, the ones the host paths compile.  fp64, IEEE division, contraction off (-ffp-contract=off in the
// Makefile's FLAGS); no fmin / fmax.  A thread whose number is >= n returns before it forms an address.
#include <hip/hip_runtime.h>
#include "../../include/trgl.h"
#include "launch.h"
#include "scene_core.h"

namespace {

struct LocalBox { double v[6]; };        // the one local box of a call with local_stride == 0
struct Planes { double v[24]; };

__global__ __launch_bounds__(256) void k_instance_boxes(LocalBox one, const double* __restrict__ local_boxes, int local_stride,
                                                        const double* __restrict__ instances, int inst_stride, uint32_t n,
                                                        double* __restrict__ boxes_out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* M = instances + (size_t)i * (size_t)inst_stride;
    double m[16], box[6], out[6];
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = M[e];
    if (local_stride) {
        const double* L = local_boxes + (size_t)i * (size_t)local_stride;
#pragma unroll
        for (int e = 0; e < 6; ++e) box[e] = L[e];
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) box[e] = one.v[e];
    }
    trgl::aabb_transform_core(box, m, out);
    double* O = boxes_out + 6 * (size_t)i;
#pragma unroll
    for (int e = 0; e < 6; ++e) O[e] = out[e];
}

__global__ __launch_bounds__(256) void k_frustum_boxes(Planes planes, const double* __restrict__ boxes, uint32_t n, int merge,
                                                       uint8_t* __restrict__ codes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* B = boxes + 6 * (size_t)i;
    double box[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) box[e] = B[e];
    const bool hit = trgl::frustum_intersects_core(planes.v, box);
    if (!hit) codes[i] = TRGL_OCCL_OUTSIDE;
    else if (!merge) codes[i] = TRGL_OCCL_VISIBLE;
}

}  // namespace

namespace trgl {

void launch_instance_boxes(hipStream_t s, const double* local_boxes, int local_stride, const double* instances, int inst_stride,
                           uint32_t n, double* boxes_out) {
    LocalBox one = {};
    if (local_stride == 0) { for (int e = 0; e < 6; ++e) one.v[e] = local_boxes[e]; local_boxes = nullptr; }
    hipLaunchKernelGGL(k_instance_boxes, dim3((n + 255) / 256), dim3(256), 0, s, one, local_boxes, local_stride, instances, inst_stride, n, boxes_out);
}

void launch_frustum_boxes(hipStream_t s, const double planes[24], const double* boxes, uint32_t n, bool merge, uint8_t* codes) {
    Planes p;
    for (int e = 0; e < 24; ++e) p.v[e] = planes[e];
    hipLaunchKernelGGL(k_frustum_boxes, dim3((n + 255) / 256), dim3(256), 0, s, p, boxes, n, merge ? 1 : 0, codes);
}

}  // namespace trgl
