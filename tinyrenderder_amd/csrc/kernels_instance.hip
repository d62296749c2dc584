// kernels_instance.hip — the stages in front of an instanced draw (include/trgl.h: trgl_draw_instanced), gfx950.
//
//   k_inst_count       : a block takes INST_BLOCK consecutive instances, one visibility byte per lane; each wave makes one ballot of
//                        bit 0 and counts it, and the block leaves its number of drawn instances in blk[block].
//   k_inst_scan_chunks : the lower level of the scan - block c turns the INST_SCAN_CHUNK entries blk[c * INST_SCAN_CHUNK ..) into their
//                        exclusive prefix sums, in place, and leaves their total in chunk[c].
//   k_inst_scan_top    : the upper level - one block turns chunk[] into its exclusive prefix sums, INST_SCAN_CHUNK entries per round
//                        with the running total carried over, and leaves the grand total in *total.
//   k_inst_scatter     : the blocks of k_inst_count make their ballots again; a drawn instance's slot is chunk[block / INST_SCAN_CHUNK]
//                        + blk[block] + the counts of the waves before its own + the set bits below its lane, so slots ascend with the
//                        instance number and no atomic decides where anything goes.  The lane writes list[slot] and, for the built-in
//                        vertex stage, MV = model_view * M of its instance (128 bytes): the vertex kernel then reads a finished matrix
//                        instead of doing the 4x4 product once per face-vertex.
//   k_inst_count_ordered, k_inst_scatter_ordered : the same two kernels over the POSITIONS of an order list (trgl_draw_instanced_ordered):
//                        lane p reads i = order[p] and its bit is i < n && (no visibility bytes || visible[i] & 1) - an entry out of range
//                        is never used as an index - and the scatter writes list[slot] = i and MV of instance i.  The scans between
//                        them, and everything behind the list, are the unordered call's.
//   k_inst_mv          : those matrices alone, for a list made elsewhere (on the host) or for a call without visibility bytes.
//   k_instance_vertex_stage : k_vertex_stage (kernels_post.hip) over the FLATTENED faces 0 .. n_vis * nfaces.  Output face g is face
//                        g % nfaces of the mesh under slot g / nfaces (one 32-bit division per thread), so a block of 64 output faces spans
//                        as many instances as it takes - the meshes this is for are a 12-face box or a 2-face quad, and a block per
//                        instance would leave most of its lanes idle.  Block shape, LDS rows and 16-byte stores are k_vertex_stage's;
//                        the arithmetic is the same dot4 calls in the same order, with the matrix read from mv[slot].  The colour of an
//                        output triangle is written by the same kernel.
// fp64 in the reference's operation order, contraction off.
#include <hip/hip_runtime.h>
#include "trgl_device.h"
#include "launch.h"
#include "device_util.h"
#include "skin_core.h"

namespace {

using namespace trgl;
using trgl_dev::block_excl_scan;
using trgl_dev::dot4;

static_assert(INST_BLOCK == 256 && INST_SCAN_CHUNK == 256, "four waves per block: block_excl_scan, and the four wave counts below");

// the ballot of bit 0 over this lane's wave; *mine: this lane's own bit
__device__ __forceinline__ unsigned long long visible_ballot(const uint8_t* __restrict__ visible, uint32_t i, uint32_t n, bool* mine) {
    *mine = i < n && (visible[i] & 1u);
    return __ballot(*mine);
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_count(const uint8_t* __restrict__ visible, uint32_t n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    bool mine;
    const unsigned long long b = visible_ballot(visible, blockIdx.x * INST_BLOCK + threadIdx.x, n, &mine);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(INST_SCAN_CHUNK) void k_inst_scan_chunks(uint32_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ chunk) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * INST_SCAN_CHUNK + threadIdx.x;
    const uint32_t v = i < nblk ? blk[i] : 0;
    uint32_t sum;
    const uint32_t excl = block_excl_scan(v, s_w, &sum);
    if (i < nblk) blk[i] = excl;
    if (threadIdx.x == 0) chunk[blockIdx.x] = sum;
}

// (the drawn instances of a call are fewer than 2^31)
__global__ __launch_bounds__(INST_SCAN_CHUNK) void k_inst_scan_top(uint32_t* __restrict__ chunk, uint32_t nchunks, unsigned long long* __restrict__ total) {
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nchunks; base += INST_SCAN_CHUNK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nchunks ? chunk[i] : 0;
        uint32_t sum;
        const uint32_t excl = block_excl_scan(v, s_w, &sum);
        if (i < nchunks) chunk[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

struct Mat4 { double m[16]; };

// out = A * B as geometry.h:196-205 sums it: every element from 0.0, k ascending (skin_core.h's statement of it, shared with trgl_pose_palette)
__device__ __forceinline__ void write_mv(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ out) {
    double b[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) b[e] = B[e];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double row[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) row[c] = trgl::mat4_mul_elem(A, b, r, c);
        double2* o = reinterpret_cast<double2*>(out + 4 * r);             // (mv_out is 16-byte aligned: a device buffer of the context's)
        o[0] = make_double2(row[0], row[1]); o[1] = make_double2(row[2], row[3]);
    }
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_scatter(const uint8_t* __restrict__ visible, uint32_t n, const uint32_t* __restrict__ blk,
                                                             const uint32_t* __restrict__ chunk, uint32_t* __restrict__ list, Mat4 mvu,
                                                             const double* __restrict__ instances, int inst_stride, double* __restrict__ mv_out) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * INST_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool mine;
    const unsigned long long b = visible_ballot(visible, i, n, &mine);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!mine) return;
    uint32_t slot = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += s_w[w];
    list[slot] = i;
    if (mv_out) write_mv(mvu.m, instances + (size_t)i * (size_t)inst_stride, mv_out + 16 * (size_t)slot);
}

// the ballot of "drawn at this position" over this lane's wave; *mine: this lane's own bit, *inst: the instance its position names
__device__ __forceinline__ unsigned long long ordered_ballot(const uint32_t* __restrict__ order, const uint8_t* __restrict__ visible, uint32_t p,
                                                             uint32_t n_order, uint32_t n, bool* mine, uint32_t* inst) {
    const uint32_t i = p < n_order ? order[p] : 0xffffffffu;
    bool m = i < n;                                                       // (n < 2^31: a position past the list fails this too)
    if (m && visible) m = (visible[i] & 1u) != 0;
    *mine = m; *inst = i;
    return __ballot(m);
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_count_ordered(const uint32_t* __restrict__ order, uint32_t n_order, const uint8_t* __restrict__ visible,
                                                                   uint32_t n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[4];
    bool mine; uint32_t i;
    const unsigned long long b = ordered_ballot(order, visible, blockIdx.x * INST_BLOCK + threadIdx.x, n_order, n, &mine, &i);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_scatter_ordered(const uint32_t* __restrict__ order, uint32_t n_order, const uint8_t* __restrict__ visible,
                                                                     uint32_t n, const uint32_t* __restrict__ blk, const uint32_t* __restrict__ chunk,
                                                                     uint32_t* __restrict__ list, Mat4 mvu, const double* __restrict__ instances,
                                                                     int inst_stride, double* __restrict__ mv_out) {
    __shared__ uint32_t s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool mine; uint32_t i;
    const unsigned long long b = ordered_ballot(order, visible, blockIdx.x * INST_BLOCK + threadIdx.x, n_order, n, &mine, &i);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!mine) return;
    uint32_t slot = chunk[blockIdx.x / INST_SCAN_CHUNK] + blk[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += s_w[w];
    list[slot] = i;
    if (mv_out) write_mv(mvu.m, instances + (size_t)i * (size_t)inst_stride, mv_out + 16 * (size_t)slot);
}

__global__ __launch_bounds__(256) void k_inst_mv(const uint32_t* __restrict__ list, uint32_t n_vis, Mat4 mvu, const double* __restrict__ instances,
                                                 int inst_stride, double* __restrict__ mv_out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_vis) return;
    const uint32_t i = list ? list[j] : j;
    write_mv(mvu.m, instances + (size_t)i * (size_t)inst_stride, mv_out + 16 * (size_t)j);
}

struct InstanceVertexParams {
    double proj[16];
    const double* vertices; const uint32_t* indices;
    double* clip; double* vary;
    uint32_t nfaces; int32_t stride;
    InstanceParams i;
};

constexpr int VS_FACES = INST_VS_FACES;
__global__ __launch_bounds__(VS_FACES * 3) void k_instance_vertex_stage(InstanceVertexParams p) {
    __shared__ __attribute__((aligned(16))) double s_clip[VS_FACES * 12];
    __shared__ __attribute__((aligned(16))) double s_vary[VS_FACES * 24];
    const uint32_t f0 = blockIdx.x * VS_FACES;                        // (total <= 2^31 - 1: no 32-bit sum here wraps)
    const int f = threadIdx.x / 3, v = threadIdx.x - 3 * f;
    const uint32_t g = f0 + (uint32_t)f;
    const uint32_t nf_blk = p.i.total - f0 < (uint32_t)VS_FACES ? p.i.total - f0 : (uint32_t)VS_FACES;
    if (g < p.i.total) {
        const uint32_t slot = g / p.nfaces, face = g - slot * p.nfaces;
        const double* mv = p.i.mv + 16 * (size_t)slot;
        const double* vert = p.vertices + (size_t)p.indices[(uint64_t)face * 3 + (uint32_t)v] * p.stride;       // model.cpp:396-412
        const double px = vert[0], py = vert[1], pz = vert[2], nx = vert[3], ny = vert[4], nz = vert[5];
        double eye[4], nrm[3];
#pragma unroll
        for (int r = 0; r < 4; ++r) eye[r] = dot4(mv + 4 * r, px, py, pz, 1.0);                   // main.cpp:77-80
#pragma unroll
        for (int r = 0; r < 3; ++r) nrm[r] = dot4(mv + 4 * r, nx, ny, nz, 0.0);                   // main.cpp:83-86
        double* uv = s_vary + 24 * f;
        uv[2 * v] = vert[6]; uv[2 * v + 1] = vert[7];                                              // main.cpp:75
#pragma unroll
        for (int k = 0; k < 3; ++k) { uv[6 + 3 * v + k] = eye[k]; uv[15 + 3 * v + k] = nrm[k]; }  // main.cpp:81,87
#pragma unroll
        for (int r = 0; r < 4; ++r) s_clip[12 * f + 4 * v + r] = dot4(p.proj + 4 * r, eye[0], eye[1], eye[2], eye[3]);  // :89
        if (v == 0) {
            if (p.i.inst_colors) p.i.colors[g] = p.i.inst_colors[p.i.list ? p.i.list[slot] : slot];
            else if (p.i.face_colors) p.i.colors[g] = p.i.face_colors[face];
        }
    }
    __syncthreads();
    {
        const double2* sc = reinterpret_cast<const double2*>(s_clip);
        double2* gc = reinterpret_cast<double2*>(p.clip + 12 * (uint64_t)f0);
        for (uint32_t k = threadIdx.x; k < nf_blk * 6; k += VS_FACES * 3) gc[k] = sc[k];
        const double2* sv = reinterpret_cast<const double2*>(s_vary);
        double2* gv = reinterpret_cast<double2*>(p.vary + 24 * (uint64_t)f0);
        for (uint32_t k = threadIdx.x; k < nf_blk * 12; k += VS_FACES * 3) gv[k] = sv[k];
    }
}

}  // namespace

namespace trgl {

uint32_t inst_num_blocks(uint64_t n) { return (uint32_t)((n + INST_BLOCK - 1) / INST_BLOCK); }
size_t inst_scratch_words(uint64_t n) { const size_t nblk = inst_num_blocks(n); return 2 + nblk + (nblk + INST_SCAN_CHUNK - 1) / INST_SCAN_CHUNK; }

void launch_block_count_scan(hipStream_t s, uint32_t* blk, uint32_t nblk, uint32_t* chunk, unsigned long long* total) {
    const uint32_t nchunks = (nblk + INST_SCAN_CHUNK - 1) / INST_SCAN_CHUNK;
    hipLaunchKernelGGL(k_inst_scan_chunks, dim3(nchunks), dim3(INST_SCAN_CHUNK), 0, s, blk, nblk, chunk);
    hipLaunchKernelGGL(k_inst_scan_top, dim3(1), dim3(INST_SCAN_CHUNK), 0, s, chunk, nchunks, total);
}

static Mat4 mat4_of(const double m[16]) { Mat4 r; for (int e = 0; e < 16; ++e) r.m[e] = m[e]; return r; }

void launch_inst_compact(hipStream_t s, const uint8_t* visible, uint32_t n, uint32_t* scratch, uint32_t* list,
                         const double model_view[16], const double* instances, int inst_stride, double* mv_out) {
    const uint32_t nblk = inst_num_blocks(n);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* blk = scratch + 2; uint32_t* chunk = blk + nblk;
    Mat4 mvu; for (int e = 0; e < 16; ++e) mvu.m[e] = mv_out ? model_view[e] : 0.0;
    hipLaunchKernelGGL(k_inst_count, dim3(nblk), dim3(INST_BLOCK), 0, s, visible, n, blk);
    launch_block_count_scan(s, blk, nblk, chunk, total);
    hipLaunchKernelGGL(k_inst_scatter, dim3(nblk), dim3(INST_BLOCK), 0, s, visible, n, blk, chunk, list, mvu, instances, inst_stride, mv_out);
}

void launch_inst_compact_ordered(hipStream_t s, const uint32_t* order, uint32_t n_order, const uint8_t* visible, uint32_t n, uint32_t* scratch,
                                 uint32_t* list, const double model_view[16], const double* instances, int inst_stride, double* mv_out) {
    const uint32_t nblk = inst_num_blocks(n_order);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* blk = scratch + 2; uint32_t* chunk = blk + nblk;
    Mat4 mvu; for (int e = 0; e < 16; ++e) mvu.m[e] = mv_out ? model_view[e] : 0.0;
    hipLaunchKernelGGL(k_inst_count_ordered, dim3(nblk), dim3(INST_BLOCK), 0, s, order, n_order, visible, n, blk);
    launch_block_count_scan(s, blk, nblk, chunk, total);
    hipLaunchKernelGGL(k_inst_scatter_ordered, dim3(nblk), dim3(INST_BLOCK), 0, s, order, n_order, visible, n, blk, chunk, list, mvu, instances,
                       inst_stride, mv_out);
}

void launch_inst_mv(hipStream_t s, const uint32_t* list, uint32_t n_vis, const double model_view[16], const double* instances,
                    int inst_stride, double* mv_out) {
    hipLaunchKernelGGL(k_inst_mv, dim3((n_vis + 255) / 256), dim3(256), 0, s, list, n_vis, mat4_of(model_view), instances, inst_stride, mv_out);
}

void launch_instance_vertex_stage(hipStream_t s, const InstanceParams& ip, const double proj[16], const double* vertices, int stride,
                                  const uint32_t* indices, uint32_t nfaces, double* clip, double* vary) {
    InstanceVertexParams p;
    for (int e = 0; e < 16; ++e) p.proj[e] = proj[e];
    p.vertices = vertices; p.indices = indices; p.clip = clip; p.vary = vary; p.nfaces = nfaces; p.stride = stride; p.i = ip;
    hipLaunchKernelGGL(k_instance_vertex_stage, dim3((ip.total + VS_FACES - 1) / VS_FACES), dim3(VS_FACES * 3), 0, s, p);
}

}  // namespace trgl
