// vertex_user.h — the vertex-stage kernel of a user vertex shader (include/trgl.h, "User vertex shaders"), compiled by hiprtc behind
// the user's source, which defines trgl_vertex.  The shape of k_vertex_stage (kernels_post.hip): one thread per face-vertex, a block
// is TRGL_VS_FACES faces whose 96-byte clip rows and K-double varyings rows are assembled in LDS and leave as contiguous 16-byte
// stores.  What differs: K is the shader's (TRGL_USER_VARY, 0..64), the rows are zero before trgl_vertex runs (a slot no call writes
// reads back as 0, as the shader's zero-initialised member arrays would), and the three calls of a face write one shared row.
//
// Faces per block: 64.  At K = 64 a block holds 64 * (12 + 64) doubles = 38 KiB of LDS, so four blocks (twelve waves) share a CU's
// 160 KiB; 128 faces would be 76 KiB, beyond the 64 KiB a block may declare, and 32 faces would make blocks of one and a half waves.
// At K = 24 it is k_vertex_stage's 18 KiB.  64 * K is even for every K, so a full block's rows are whole 16-byte words and every
// block's first row is 16-byte aligned when the array is.
#pragma once
#include "user_prelude.h"

static_assert(__is_same(decltype(trgl_vertex(*(const trgl_vert_in*)nullptr, *(trgl_vert_out*)nullptr)), void),
              "trgl_vertex must be declared as: __device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out)");

constexpr int TRGL_VS_FACES = TRGL_VERTEX_USER_FACES;
constexpr int TRGL_VS_THREADS = TRGL_VS_FACES * 3;
constexpr int TRGL_VS_K = TRGL_USER_VARY;
static_assert(TRGL_VS_K >= 0 && TRGL_VS_K <= TRGL_MAX_USER_VARY, "TRGL_USER_VARY out of range");
static_assert(TRGL_VS_FACES * (12 + TRGL_MAX_USER_VARY) * sizeof(double) <= 40 * 1024, "four blocks per CU at K = 64");

extern "C" __global__ __launch_bounds__(TRGL_VS_THREADS)
void trgl_vertex_user(VertexUserParams p) {
    __shared__ __attribute__((aligned(16))) double s_clip[TRGL_VS_FACES * 12];
    __shared__ __attribute__((aligned(16))) double s_vary[TRGL_VS_K ? TRGL_VS_FACES * TRGL_VS_K : 2];     // (no array of size 0)
    const uint64_t f0 = (uint64_t)blockIdx.x * TRGL_VS_FACES;
    const uint64_t i = f0 * 3 + threadIdx.x;
    const bool live = i < (uint64_t)p.nfaces * 3;
    const uint32_t nf_blk = (uint32_t)(p.nfaces - f0 < (uint64_t)TRGL_VS_FACES ? p.nfaces - f0 : TRGL_VS_FACES);
    const uint32_t index = live ? p.indices[i] : 0u;                // (requested ahead of the zeroing)
    {
        double2* zc = reinterpret_cast<double2*>(s_clip);
        for (uint32_t k = threadIdx.x; k < TRGL_VS_FACES * 6; k += TRGL_VS_THREADS) zc[k] = make_double2(0.0, 0.0);
        double2* zv = reinterpret_cast<double2*>(s_vary);
        for (uint32_t k = threadIdx.x; k < TRGL_VS_FACES * TRGL_VS_K / 2; k += TRGL_VS_THREADS) zv[k] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (live) {
        const int f = threadIdx.x / 3, v = threadIdx.x - 3 * f;
        trgl_vert_in in;
        in.vertex = p.vertices + (size_t)index * (size_t)p.stride;   // model.cpp:396-412
        in.stride = p.stride;
        in.index = index;
        in.face = (int)(f0 + f);
        in.nth = v;
        in.u = &p.u;
        in.projection = p.proj;
        in.instance = 0u; in.inst = nullptr; in.inst_stride = 0;
        trgl_vert_out out;
        out.clip[0] = out.clip[1] = out.clip[2] = out.clip[3] = 0.0;
        out.vary = TRGL_VS_K ? s_vary + TRGL_VS_K * f : nullptr;
        trgl_vertex(in, out);                                        // our_gl.h:46; main.cpp:662: clip[v] = shader.vertex(face, v)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_clip[12 * f + 4 * v + r] = out.clip[r];
    }
    __syncthreads();
    {
        const double2* sc = reinterpret_cast<const double2*>(s_clip);
        double2* gc = reinterpret_cast<double2*>(p.clip + 12 * f0);
        for (uint32_t k = threadIdx.x; k < nf_blk * 6; k += TRGL_VS_THREADS) gc[k] = sc[k];
        if (TRGL_VS_K) {
            const uint32_t nd = nf_blk * TRGL_VS_K;                   // doubles of this block: odd only in a partial last block
            const double2* sv = reinterpret_cast<const double2*>(s_vary);
            double2* gv = reinterpret_cast<double2*>(p.vary + (uint64_t)TRGL_VS_K * f0);
            for (uint32_t k = threadIdx.x; k < nd / 2; k += TRGL_VS_THREADS) gv[k] = sv[k];
            if ((nd & 1u) && threadIdx.x == 0) p.vary[(uint64_t)TRGL_VS_K * f0 + nd - 1] = s_vary[nd - 1];
        }
    }
}

// The same stage over the flattened faces of an instanced call (include/trgl.h: trgl_draw_instanced): output face g of 0 .. i.total is
// face g % nfaces of the mesh under slot g / nfaces - one 32-bit division per thread, so a block of 64 output faces spans as many
// instances as it takes (a 12-face box: six of them).  Rows leave exactly as above; the output triangle's colour is written here too.
extern "C" __global__ __launch_bounds__(TRGL_VS_THREADS)
void trgl_vertex_user_instanced(VertexUserInstancedParams q) {
    __shared__ __attribute__((aligned(16))) double s_clip[TRGL_VS_FACES * 12];
    __shared__ __attribute__((aligned(16))) double s_vary[TRGL_VS_K ? TRGL_VS_FACES * TRGL_VS_K : 2];
    const VertexUserParams& p = q.v;
    const uint32_t f0 = blockIdx.x * TRGL_VS_FACES;                 // (total <= 2^31 - 1: no 32-bit sum here wraps)
    const int f = threadIdx.x / 3, v = threadIdx.x - 3 * f;
    const uint32_t g = f0 + (uint32_t)f;
    const bool live = g < q.i.total;
    const uint32_t nf_blk = q.i.total - f0 < (uint32_t)TRGL_VS_FACES ? q.i.total - f0 : (uint32_t)TRGL_VS_FACES;
    uint32_t slot = 0, face = 0, inst = 0, index = 0;
    if (live) {
        slot = g / p.nfaces; face = g - slot * p.nfaces;
        inst = q.i.list ? q.i.list[slot] : slot;
        index = p.indices[(uint64_t)face * 3 + (uint32_t)v];
    }
    {
        double2* zc = reinterpret_cast<double2*>(s_clip);
        for (uint32_t k = threadIdx.x; k < TRGL_VS_FACES * 6; k += TRGL_VS_THREADS) zc[k] = make_double2(0.0, 0.0);
        double2* zv = reinterpret_cast<double2*>(s_vary);
        for (uint32_t k = threadIdx.x; k < TRGL_VS_FACES * TRGL_VS_K / 2; k += TRGL_VS_THREADS) zv[k] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (live) {
        trgl_vert_in in;
        in.vertex = p.vertices + (size_t)index * (size_t)p.stride;
        in.stride = p.stride;
        in.index = index;
        in.face = (int)face;
        in.nth = v;
        in.u = &p.u;
        in.projection = p.proj;
        in.instance = inst;
        in.inst = q.i.instances ? q.i.instances + (size_t)inst * (size_t)q.i.inst_stride : nullptr;
        in.inst_stride = q.i.inst_stride;
        trgl_vert_out out;
        out.clip[0] = out.clip[1] = out.clip[2] = out.clip[3] = 0.0;
        out.vary = TRGL_VS_K ? s_vary + TRGL_VS_K * f : nullptr;
        trgl_vertex(in, out);
#pragma unroll
        for (int r = 0; r < 4; ++r) s_clip[12 * f + 4 * v + r] = out.clip[r];
        if (v == 0) {
            if (q.i.inst_colors) q.i.colors[g] = q.i.inst_colors[inst];
            else if (q.i.face_colors) q.i.colors[g] = q.i.face_colors[face];
        }
    }
    __syncthreads();
    {
        const double2* sc = reinterpret_cast<const double2*>(s_clip);
        double2* gc = reinterpret_cast<double2*>(p.clip + 12 * (uint64_t)f0);
        for (uint32_t k = threadIdx.x; k < nf_blk * 6; k += TRGL_VS_THREADS) gc[k] = sc[k];
        if (TRGL_VS_K) {
            const uint32_t nd = nf_blk * TRGL_VS_K;                   // odd only in a partial last block
            const double2* sv = reinterpret_cast<const double2*>(s_vary);
            double2* gv = reinterpret_cast<double2*>(p.vary + (uint64_t)TRGL_VS_K * f0);
            for (uint32_t k = threadIdx.x; k < nd / 2; k += TRGL_VS_THREADS) gv[k] = sv[k];
            if ((nd & 1u) && threadIdx.x == 0) p.vary[(uint64_t)TRGL_VS_K * f0 + nd - 1] = s_vary[nd - 1];
        }
    }
}
