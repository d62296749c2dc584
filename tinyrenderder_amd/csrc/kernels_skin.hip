// kernels_skin.hip — skeletal animation: linear blend skinning of a vertex array and the composition of joint hierarchies into
// palettes (include/trgl.h: trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned), gfx950.  The arithmetic is skin_core.h's.
//
// k_skin_stage<NI> streams.  A block owns `vb` consecutive vertices (SKIN_BLOCK, fewer when a record is wider than SKIN_TILE_DOUBLES /
// SKIN_BLOCK doubles) and up to SKIN_POSE_GROUP consecutive poses:
//   1. the block's records are contiguous memory: its lanes load them 16 bytes each (8 at a head or tail that is only 8-byte aligned)
//      into the LDS tile, whatever the record's size; lane p then takes vertex p's position and flagged directions out of the tile and
//      its NI joint numbers and weights from memory into registers - once for all poses;
//   2. per pose: the three used rows of every joint go to LDS when n_joints <= SKIN_LDS_JOINTS (else they are read through the cache:
//      same values, same order, same bits); lane p blends, transforms, and puts the results back into its record in the tile; the
//      lanes then store the tile to the pose's output, again as contiguous memory 16 bytes per lane.  The doubles that are only copied
//      never leave the tile.
// k_pose_palette_lds / _mem: 16 lanes per pose, one per element of a 4x4 product, POSE_GROUP poses per block of one wave; the joints
// are walked in order (the chain is sequential in j; `parents` is the same for every pose, so the block's control flow is uniform).
// Up to POSE_LDS_JOINTS joints a pose's matrices stay in LDS from the load of the local matrices to the store of the palette.
// No atomics.  Every vertex, pose or joint number is compared with its count before it becomes an address.
#include <hip/hip_runtime.h>
#include "launch.h"
#include "skin_core.h"

namespace {

using namespace trgl;

struct alignas(16) Pair { double a, b; };

// n doubles from memory to LDS / from LDS to memory, as contiguous memory: 16 bytes per lane, 8 at a head or tail (g: 8-byte aligned)
__device__ inline void tile_load(double* t, const double* g, uint32_t n) {
    const uint32_t head = (((uintptr_t)g & 15) != 0 && n) ? 1u : 0u;
    if (head && threadIdx.x == 0) t[0] = g[0];
    const uint32_t pairs = (n - head) >> 1;
    for (uint32_t i = threadIdx.x; i < pairs; i += SKIN_BLOCK) {
        const Pair v = *reinterpret_cast<const Pair*>(g + head + 2u * i);
        t[head + 2u * i] = v.a; t[head + 2u * i + 1u] = v.b;
    }
    if (((n - head) & 1u) && threadIdx.x == SKIN_BLOCK - 1) t[n - 1u] = g[n - 1u];
}
__device__ inline void tile_store(const double* t, double* g, uint32_t n) {
    const uint32_t head = (((uintptr_t)g & 15) != 0 && n) ? 1u : 0u;
    if (head && threadIdx.x == 0) g[0] = t[0];
    const uint32_t pairs = (n - head) >> 1;
    for (uint32_t i = threadIdx.x; i < pairs; i += SKIN_BLOCK)
        *reinterpret_cast<Pair*>(g + head + 2u * i) = Pair{ t[head + 2u * i], t[head + 2u * i + 1u] };
    if (((n - head) & 1u) && threadIdx.x == SKIN_BLOCK - 1) g[n - 1u] = t[n - 1u];
}

template <int NI>
__global__ __launch_bounds__(SKIN_BLOCK) void k_skin_stage(const SkinArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];      // the tile of vb records, then the staged palette rows
    double* tile = smem;
    double* pal = smem + skin_tile_doubles(a.vb, a.stride);
    const uint64_t vblock = blockIdx.x % a.n_vblocks, pgroup = blockIdx.x / a.n_vblocks;
    const uint64_t base = vblock * a.vb;
    const uint32_t nv = (uint32_t)(a.n - base < (uint64_t)a.vb ? a.n - base : (uint64_t)a.vb);
    const uint32_t S = a.stride, nd = nv * S, p = threadIdx.x;
    const uint64_t q0 = pgroup * SKIN_POSE_GROUP;
    const uint32_t nq = (uint32_t)(a.n_poses - q0 < (uint64_t)SKIN_POSE_GROUP ? a.n_poses - q0 : (uint64_t)SKIN_POSE_GROUP);
    const bool mine = p < nv, in_lds = a.n_joints <= (uint32_t)SKIN_LDS_JOINTS;

    tile_load(tile, a.vertices + base * S, nd);
    uint32_t jt[NI]; double w[NI];
    if (mine) {
        const uint16_t* jr = a.joints + (base + p) * NI;
        const double* wr = a.weights + (base + p) * NI;
#pragma unroll
        for (int k = 0; k < NI; ++k) { jt[k] = jr[k]; w[k] = wr[k]; }
    }
    __syncthreads();
    double* rec = tile + p * S;      // (used by lanes with a vertex only)
    double pos[3] = { 0.0, 0.0, 0.0 }, dir[3][3] = { { 0.0 } };
    if (mine) {
        pos[0] = rec[0]; pos[1] = rec[1]; pos[2] = rec[2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (a.flags & (1u << d)) { const double* s = rec + skin_dir_offset(d); dir[d][0] = s[0]; dir[d][1] = s[1]; dir[d][2] = s[2]; }
    }
    for (uint32_t qi = 0; qi < nq; ++qi) {
        const double* palette = a.palette + (q0 + qi) * a.palette_stride;
        if (in_lds)
            for (uint32_t i = p; i < a.n_joints * 12u; i += SKIN_BLOCK) { const uint32_t j = i / 12u; pal[i] = palette[16u * j + (i - 12u * j)]; }
        __syncthreads();      // the palette is staged, and the previous pose's stores have left the tile
        if (mine) {
            double B[12];
            skin_blend_zero(B);
#pragma unroll
            for (int k = 0; k < NI; ++k)
                if (jt[k] < a.n_joints) {
                    if (in_lds) skin_blend_add(B, w[k], pal + 12u * jt[k]);
                    else skin_blend_add(B, w[k], palette + 16u * (uint64_t)jt[k]);
                }
            double o[3];
            skin_position(B, pos[0], pos[1], pos[2], o);
            rec[0] = o[0]; rec[1] = o[1]; rec[2] = o[2];
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (a.flags & (1u << d)) {
                    skin_direction(B, dir[d][0], dir[d][1], dir[d][2], o);
                    double* s = rec + skin_dir_offset(d);
                    s[0] = o[0]; s[1] = o[1]; s[2] = o[2];
                }
        }
        __syncthreads();
        tile_store(tile, a.out + ((q0 + qi) * a.n + base) * S, nd);
    }
}

// One wave per block: the 16 lanes of a pose exchange matrix elements through LDS in program order - the LDS serves a wave's
// instructions in order, so an element stored by one instruction is there for a later one of the same wave, and an element read by
// one is read before a later one overwrites it.  (wave_barrier only keeps the compiler from moving LDS accesses across it.)
static_assert(POSE_BLOCK == 64, "k_pose_palette_lds exchanges through LDS without a barrier: a block must be one wave");

// Up to POSE_LDS_JOINTS joints.  The local matrices of the block's poses are loaded into LDS at once, become world matrices in place
// as the joints are walked, then palette matrices, and leave as they came: no access to memory waits inside the walk.
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_palette_lds(const PoseArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];      // [POSE_GROUP][n_joints][16]
    const uint32_t g = threadIdx.x >> 4, e = threadIdx.x & 15u, r = e >> 2, c = e & 3u, nj = a.n_joints;
    const uint64_t pose = (uint64_t)blockIdx.x * POSE_GROUP + g;
    const bool live = pose < a.n_poses;
    double* W = smem + (size_t)g * nj * 16;
    const int32_t* __restrict__ parents = a.parents;
    const double* __restrict__ ib = a.inverse_bind;
    if (live) {
        const double* __restrict__ loc = a.local + pose * a.local_stride;
        for (uint32_t j = 0; j < nj; ++j) W[16u * j + e] = loc[16u * j + e];
    }
    __builtin_amdgcn_wave_barrier();
    if (live) {      // (a pose past the end computes nothing; its lanes share no LDS with the others)
        for (uint32_t j = 0; j < nj; ++j) {
            const int32_t parent = parents[j];
            if (pose_parent_below(parent, j)) {      // (the same for every lane of the block)
                const double v = mat4_mul_elem(W + 16u * (uint32_t)parent, W + 16u * j, (int)r, (int)c);
                __builtin_amdgcn_wave_barrier();      // every element of local_j is read before one is overwritten
                W[16u * j + e] = v;
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (ib)
            for (uint32_t j = 0; j < nj; ++j) {
                const double v = mat4_mul_elem(W + 16u * j, ib + 16u * j, (int)r, (int)c);
                __builtin_amdgcn_wave_barrier();
                W[16u * j + e] = v;
                __builtin_amdgcn_wave_barrier();
            }
        double* __restrict__ out = a.palette + pose * a.palette_stride;
        for (uint32_t j = 0; j < nj; ++j) out[16u * j + e] = skin_canon(W[16u * j + e]);      // (the lane's own elements)
    }
}

// More joints than that: the world matrices go through the pose's own palette in memory, which only these 16 lanes touch.  A store, a
// fence and the block's barrier come before any load of it; the inverse bind matrices are applied in a second walk.
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_palette_mem(const PoseArgs a) {
    __shared__ __attribute__((aligned(16))) double L[POSE_GROUP * 16];      // local_j of the block's poses
    const uint32_t g = threadIdx.x >> 4, e = threadIdx.x & 15u, r = e >> 2, c = e & 3u, nj = a.n_joints;
    const uint64_t pose = (uint64_t)blockIdx.x * POSE_GROUP + g;
    const bool live = pose < a.n_poses;
    double* out = live ? a.palette + pose * a.palette_stride : nullptr;
    const double* loc = live ? a.local + pose * a.local_stride : nullptr;
    double next = live ? loc[e] : 0.0;
    for (uint32_t j = 0; j < nj; ++j) {
        const double le = next;
        if (live && j + 1 < nj) next = loc[16u * (j + 1) + e];
        const int32_t parent = a.parents[j];
        double v = le;
        if (pose_parent_below(parent, j)) {      // (the same for every lane of the block)
            L[16u * g + e] = le;
            __syncthreads();      // local_j is in LDS; the world matrices of the joints below j are in memory
            if (live) v = mat4_mul_elem(out + 16u * (uint32_t)parent, L + 16u * g, (int)r, (int)c);
            __syncthreads();
        }
        if (live) out[16u * j + e] = skin_canon(v);
        __threadfence();      // the store is done before the barrier that a load of it follows
    }
    if (!a.inverse_bind) return;
    __syncthreads();
    for (uint32_t j = 0; j < nj; ++j) {
        double v = 0.0;
        if (live) v = mat4_mul_elem(out + 16u * j, a.inverse_bind + 16u * j, (int)r, (int)c);
        __syncthreads();      // every lane has read world_j before its place takes palette_j
        if (live) out[16u * j + e] = skin_canon(v);
    }
}

template <int NI> void skin_launch(hipStream_t s, const SkinArgs& a, unsigned blocks) {
    const size_t lds = (skin_tile_doubles(a.vb, a.stride) + (a.n_joints <= (uint32_t)SKIN_LDS_JOINTS ? a.n_joints * 12u : 0u)) * sizeof(double);
    hipLaunchKernelGGL(k_skin_stage<NI>, dim3(blocks), dim3(SKIN_BLOCK), lds, s, a);
}

}  // namespace

namespace trgl {

void launch_skin_stage(hipStream_t s, const SkinArgs& a, int n_influences) {
    const unsigned blocks = (unsigned)(a.n_vblocks * ((a.n_poses + SKIN_POSE_GROUP - 1) / SKIN_POSE_GROUP));
    switch (n_influences) {
        case 1: skin_launch<1>(s, a, blocks); break;
        case 2: skin_launch<2>(s, a, blocks); break;
        case 3: skin_launch<3>(s, a, blocks); break;
        case 4: skin_launch<4>(s, a, blocks); break;
        case 5: skin_launch<5>(s, a, blocks); break;
        case 6: skin_launch<6>(s, a, blocks); break;
        case 7: skin_launch<7>(s, a, blocks); break;
        default: skin_launch<8>(s, a, blocks); break;
    }
}

void launch_pose_palette(hipStream_t s, const PoseArgs& a) {
    const unsigned blocks = (unsigned)((a.n_poses + POSE_GROUP - 1) / POSE_GROUP);
    if (a.n_joints <= (uint32_t)POSE_LDS_JOINTS)
        hipLaunchKernelGGL(k_pose_palette_lds, dim3(blocks), dim3(POSE_BLOCK), (size_t)POSE_GROUP * a.n_joints * 16 * sizeof(double), s, a);
    else
        hipLaunchKernelGGL(k_pose_palette_mem, dim3(blocks), dim3(POSE_BLOCK), 0, s, a);
}

}  // namespace trgl
