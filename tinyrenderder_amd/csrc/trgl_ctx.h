// trgl_ctx.h — the context behind the C ABI and what the library's own translation units share of it (private: neither installed
// nor embedded).  trgl_api.cpp owns the flush pipeline and its ordering rules; trgl_shader.cpp, the stage entry points
// (trgl_stage_*.cpp, which share trgl_stage.h on top of this file), trgl_passes.cpp and trgl_rccl.cpp reach the context through
// the few functions declared at the end; trgl_host.cpp (no HIP) does not include this file.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>
#include <string>
#include <vector>

#include "../../include/trgl.h"
#include "launch.h"
#include "trgl_device.h"

namespace trgl {
struct StageChunk { char* base; size_t cap, used; };

// the growth rule of most device buffers: 25 % + 1024 elements of headroom
inline size_t headroom(size_t need) { return need + need / 4 + 1024; }
// Device memory owned by the context (or by a caller's scope) and freed with it; `cap` counts elements.
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // (re)allocate `n` elements; the old contents are not kept (the stream is synchronised before they are freed)
    int alloc(trgl_ctx* c, size_t n);
    // at least `need` elements: `ncap` of them (by default headroom(need)) when the buffer has to grow
    int grow(trgl_ctx* c, size_t need, size_t ncap) { return need <= cap ? TRGL_OK : alloc(c, ncap); }
    int grow(trgl_ctx* c, size_t need) { return grow(c, need, headroom(need)); }
    // give the memory back before the owner goes (the stream is synchronised first)
    int release(trgl_ctx* c);
};

// a flush whose first half (setup + binning) has run and whose raster half is still to be launched (trgl_flush_begin)
// (builtin_shade: the flush has PHONG / EYE draws; user_kinds: bit i = it has draws of user kind TRGL_SHADER_USER_FIRST + i)
// direct: the binning queued by trgl_flush_begin reads k_setup's segments (seg); settled: the pair count has been looked at and the
// binning that leaves the lists is queued (settle_binning); fell_back: the direct path's kernels did nothing and k_expand's chain ran
struct PendingRaster { bool active = false; FrameParams fp; int flush_kind = 0; uint32_t cap = 0; int cur = 0; uint64_t N = 0;
                       bool builtin_shade = false; uint32_t user_kinds = 0;
                       bool direct = false, settled = false, fell_back = false; SegLayout seg{}; uint32_t nblk = 0; };
// What trgl_debug_read reports of a flush: the PendingRaster as trgl_flush_end left it (fp.zq_cull decided, cap the pair buffers' own)
// and the counts that came over from k_setup.  valid: from a complete flush until the next trgl_draw / trgl_clear.
struct Snapshot { bool valid = false; PendingRaster rp; uint64_t P = 0, literal_tris = 0, large_tris = 0; };
// a user shader registered on the context (trgl_register_shader_ex): its module and kernel - the shade kernel, or the raster kernel
// of a kind that may discard (TRGL_SHADER_MAY_DISCARD) - and the TRGL_SHADER_* flags it was registered with
struct UserKind { hipModule_t mod; hipFunction_t fn; int K; uint32_t flags; };
// a user vertex shader registered on the context (trgl_register_vertex_shader): its module and its vertex-stage kernel (vertex_user.h)
// (fn_inst: the kernel of the same module that trgl_draw_instanced runs)
struct UserVertex { hipModule_t mod; hipFunction_t fn; int K; hipFunction_t fn_inst; };
}  // namespace trgl
using namespace trgl;

struct trgl_ctx {
    int device = 0;
    int W = 0, H = 0, bpp = 0, tiles_x = 0, tiles_y = 0;
    hipStream_t stream = nullptr;       // the stream in use
    hipStream_t own_stream = nullptr;   // created with the context
    DevBuf<uint8_t> fb;
    DevBuf<double> zb;
    double vp[16];
    bool clear_pending = true;
    uint32_t clear_color = 0xff000000u;
    double clear_z = std::numeric_limits<double>::infinity();
    int strip_y0 = 0, strip_y1 = 0;
    int il_tiles = 0, il_world = 1, il_rank = 0;     // interleaved bands instead of one strip (trgl_set_interleave)

    DevTexture tex_host[TRGL_MAX_TEXTURES];
    size_t tex_cap[TRGL_MAX_TEXTURES] = {};      // bytes of each slot's allocation: a chain fits when mip_slot_offset(w, h, bpp, L) does
    DevBuf<DevTexture> tex_dev;

    std::vector<DrawDesc> draws;
    uint64_t queued_tris = 0;
    std::vector<StageChunk> stage;
    int stage_hold = 0;                 // >0 while a draw call has staged data that no DrawDesc references yet

    // per triangle of the flush (grown together, for N + 1 triangles: the record behind the last one is read by k_make_items)
    DevBuf<TriRec> recs; DevBuf<TriW> recs_w; DevBuf<uint32_t> cnt; DevBuf<uint2> tilebox;
    PendingRaster rp;
    hipEvent_t ev_pairs = nullptr;      // recorded behind the copy of the flush's pair count into pinned memory
    DevBuf<uint32_t> idbuf;             // visibility buffer of PHONG / EYE flushes, [H][W]
    DevBuf<BoundsPartial> bounds_scratch;   // trgl_mesh_bounds: the result + the per-block partials, allocated by the first call
    DevBuf<uint8_t> mesh_scratch;       // trgl_mesh_normals / trgl_mesh_tangents: flag, face vectors, sorted corners, the sort's own space; grows on demand
    DevBuf<double> zsnap[TRGL_MAX_Z_SNAPSHOTS];   // trgl_zbuffer_snapshot: [H][W] depths per slot in use
    // trgl_image_blur / trgl_framebuffer_blur: the weights of blur_radius (0: none) and the image between the two passes; grow on demand.
    // The weights travel through blur_w_pinned; ev_blur_w is recorded behind that copy, so that the next upload knows when it may rewrite it
    DevBuf<float> blur_weights; DevBuf<uint8_t> blur_tmp; int blur_radius = 0;
    float* blur_w_pinned = nullptr; size_t blur_w_pinned_cap = 0; hipEvent_t ev_blur_w = nullptr;
    DevBuf<uint32_t> clip_scratch;      // trgl_clip_stage and the clipped draws: the 8-byte count of outputs, then the words of the stage's scan; grows on demand
    DevBuf<uint8_t> resolve_tmp;        // trgl_framebuffer_resolve with a host dst: the filtered image on its way out; grows on demand
    DevBuf<uint8_t> shadow_tmp;         // trgl_shadow_mask / trgl_framebuffer_modulate with a host mask: the W * H bytes on their way; grows on demand
    // trgl_occlusion_boxes(_image): the two levels of block maxima over the depths, rebuilt by every call; host boxes and the codes for a
    // host array on their way; grow on demand
    DevBuf<double> occl_levels, occl_boxes; DevBuf<uint8_t> occl_codes;
    // trgl_draw_instanced / trgl_instance_stage: the 8-byte count of drawn instances and the words of the compaction's scan; the list of
    // drawn instances; model_view * M per drawn instance for the built-in stage.  Read by the stages the call queues; grow on demand
    DevBuf<uint32_t> inst_scratch, inst_list; DevBuf<double> inst_mv;
    // trgl_mesh_edges: the 8-byte count, keys and half-edge numbers with their sorted copies, the scan's words, the sort's own space;
    // trgl_edge_select with compaction: the 8-byte count, a byte per record, the scan's words.  Grows on demand
    DevBuf<uint8_t> edge_scratch;
    // trgl_subdiv_topology: two sort entries per edge record with their sorted copies and the sort's own space.  Grows on demand
    DevBuf<uint8_t> subdiv_scratch;
    // trgl_mesh_weld: the 8-byte count, hashes and vertex numbers with their sorted copies, representatives, new numbers, the map, the
    // scan's words, the sort's own space.  Grows on demand.  weld_hash_bits: the low bits of the hash in use (trgl_debug_weld_hash_bits)
    DevBuf<uint8_t> weld_scratch;
    int weld_hash_bits = 64;
    // trgl_mesh_clean: the two 8-byte counts, face hashes and numbers with their sorted copies, keep bytes, referenced words, the vertex map,
    // the two scans' words, the sort's own space.  lod_work: the arrays between the weld, the mean and the clean of trgl_mesh_simplify.
    // Both grow on demand.  lod_hash_bits: the low bits of the face hash in use (trgl_debug_lod_hash_bits)
    DevBuf<uint8_t> lod_scratch;
    DevBuf<uint8_t> lod_work;
    int lod_hash_bits = 64;
    DevBuf<uint8_t> order_scratch;      // trgl_depth_order: the keys, their sorted copy, the numbers 0 .. n-1, the sort's own space; grows on demand
    DevBuf<uint8_t> pp_out;            // trgl_postprocess: three [H][W][3] images + two 64-bit z-range keys, kept between calls
    DevBuf<uint32_t> blk_sums;          // pairs per setup block of 256 triangles
    DevBuf<uint32_t> chunk_off;         // pairs before every 16th setup block
    DevBuf<uint32_t> keys[2], vals[2]; DevBuf<uint16_t> bmask[2];     // (tile, triangle, block mask) pairs, ping-pong; grown together
    DevBuf<uint32_t> hist, scan_tmp;
    // The direct path of the binning: the segments k_setup writes its pairs to, the word k_chunk_spine sets when a
    // flush does not fit them (+ its pinned copy), and how the path is chosen: bin_mode 0 by the rule of seg_sizes(), 1 always k_expand's
    // chain, 2 always direct with bin_S / bin_G (trgl_debug_binning).  seg_hold: a flush fell back - k_expand's chain until a flush fits.
    DevBuf<uint32_t> seg_keys, seg_vals, seg_flag;
    uint32_t* seg_flag_pinned = nullptr;
    int bin_mode = 0; uint32_t bin_S = 0, bin_G = 0;
    bool seg_hold = false;
    // the grids of the radix scatters: at most radix_max_blocks blocks (0: as many as the device holds at once); radix_used: the grids
    // of the first and the last pass the last flush queued (trgl_debug_radix_blocks)
    uint32_t radix_max_blocks = 0, radix_used[2] = { 0, 0 };
    uint64_t rule_pairs = 0, rule_nblk = 0;     // pairs and setup blocks of the last flush that had triangles: a, the input of seg_sizes()
    DevBuf<uint32_t> tile_start;        // tile_start[bounds_half()] followed by tile_end[bounds_half()]: set together per flush (in 16-byte words)
    DevBuf<uint4> items; DevBuf<uint32_t> n_items;
    DevBuf<unsigned long long> item_stats;
    DevBuf<DrawDesc> draws_dev;
    DevBuf<DevStats> stats_dev;
    DevStats* stats_pinned = nullptr;

    uint64_t triangles_total = 0;       // our_gl.cpp:90 counts every call, host side
    Snapshot snap;                      // the last complete flush (all but `valid` outlives it: trgl_debug_binning, trgl_get_last_flush_info)

    bool profiling = false, events_pending = false;
    hipEvent_t ev[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    double phase_ms[TRGL_NUM_PHASES] = { 0, 0, 0, 0, 0 };
    uint64_t flushes_timed = 0;

    std::vector<UserKind> user;         // kind TRGL_SHADER_USER_FIRST + i is user[i]
    std::vector<UserVertex> vertex;     // vertex shader i of trgl_register_vertex_shader

    std::string err;

    size_t bounds_half() const { return ((size_t)tiles_x * tiles_y + 3) & ~size_t(3); }
    uint32_t* tile_end() const { return tile_start.p + bounds_half(); }
};

#define HIPCHK(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return TRGL_E_HIP;                                                                 \
        }                                                                                      \
    } while (0)

#define CHKCTX(ctx) do { if (!(ctx)) return TRGL_E_INVALID; if (hipSetDevice((ctx)->device) != hipSuccess) return TRGL_E_HIP; } while (0)

namespace trgl {
template <class T> int DevBuf<T>::release(trgl_ctx* c) {
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); p = nullptr; cap = 0; }
    return TRGL_OK;
}
template <class T> int DevBuf<T>::alloc(trgl_ctx* c, size_t n) {
    if (int r = release(c)) return r;
    HIPCHK(c, hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
    return TRGL_OK;
}

// pins the staged arrays of a draw call in progress: a flush it triggers does not recycle them
struct StageHold { trgl_ctx* c; explicit StageHold(trgl_ctx* x) : c(x) { ++c->stage_hold; } ~StageHold() { --c->stage_hold; } };

inline bool valid_mem_kind(int mem_kind) { return mem_kind == TRGL_MEM_HOST || mem_kind == TRGL_MEM_DEVICE; }
// neither a strip nor interleaved bands: every row of the framebuffer and the z-buffer is this context's
inline bool owns_whole_frame(const trgl_ctx* c) { return c->strip_y0 == 0 && c->strip_y1 == c->H && c->il_world <= 1; }
// the registered user kind `kind`; null for a built-in or unknown kind
inline const UserKind* user_kind(const trgl_ctx* c, int kind) {
    const int i = kind - TRGL_SHADER_USER_FIRST;
    return (kind >= TRGL_SHADER_USER_FIRST && i < (int)c->user.size()) ? &c->user[i] : nullptr;
}

// trgl_api.cpp
int fail(trgl_ctx* c, int code, const std::string& msg);     // the message goes to the context, or with c == nullptr to the global string
int end_pending_raster(trgl_ctx* c);        // the context's state is about to change: launch the raster half trgl_flush_begin left pending
int flush_sync(trgl_ctx* c);                // everything queued, done
int stage_alloc(trgl_ctx* c, size_t bytes, void** dev);      // device memory from the per-flush arena, 256-byte aligned
int stage_copy(trgl_ctx* c, const void* src, size_t bytes, void** dev);      // ... filled from host memory before the call returns
int kind_vary_count(const trgl_ctx* c, int kind);            // the varyings per triangle of a kind trgl_draw accepts, -1 for any other
int check_kind_uniforms(trgl_ctx* c, const char* who, int kind, const trgl_uniforms* u);     // what a kind needs of its uniforms
// trgl_host.cpp
const char* global_error();                 // what trgl_last_error(NULL) returns
void host_mesh_bounds(const double* vertices, int stride, uint64_t n, double out_min[3], double out_max[3]);      // n > 0
// normals (or tangents) of an indexed mesh in place, where a vertex lacks them: 1 generated, 0 left alone, -1 an index out of range
int host_mesh_attr(bool tangents, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces);
// the clip stage over host arrays (outputs with room for 2 n triangles); returns the number of output triangles
uint64_t host_clip_stage(const double plane[4], const ClipTable& tab, int K, const double* clip, const double* vary, const uint32_t* colors,
                         uint64_t n, double* clip_out, double* vary_out, uint32_t* colors_out);
// the codes of n boxes against a w x h depth image in host memory (depth is not read when w * h == 0)
void host_occlusion_boxes(const double* depth, int w, int h, const double viewport[16], const double view_proj[16],
                          const double* boxes, uint64_t n, uint8_t* codes);
// trgl_instance_depths and trgl_depth_order over host arrays (host_depth_order: false when it ran out of memory)
void host_instance_depths(const double model_view[16], const double point[3], const double* instances, int stride, uint64_t n, double* depths);
bool host_depth_order(const double* depths, uint64_t n, bool front_to_back, uint32_t* order);
// trgl_triangle_depths over host arrays (G groups of g triangles), and trgl_order_stage (every entry of the list checked: below G)
void host_triangle_depths(const double* clip, uint64_t G, uint32_t g, int mode, double* depths);
void host_order_stage(int K, const double* clip, const double* vary, const uint32_t* colors, const uint32_t* order, uint64_t n_order, uint32_t g,
                      double* clip_out, double* vary_out, uint32_t* colors_out);
// trgl_sprite_stage and trgl_line_stage over host arrays (vary_out null: no varyings; colors null: colors_out is not written; every
// index of a line list checked: below n_points)
void host_sprite_stage(const trgl_sprite_params& P, const double* points, int stride, const uint32_t* colors, uint64_t n,
                       double* clip_out, double* vary_out, uint32_t* colors_out);
void host_line_stage(const trgl_line_params& P, const double* points, int stride, const uint32_t* indices, const uint32_t* colors, uint64_t n,
                     double* clip_out, double* vary_out, uint32_t* colors_out);
// trgl_skin_stage and trgl_pose_palette over host arrays (every joint number and parent checked by the caller)
void host_skin_stage(const trgl_skin_params& P, const double* vertices, uint64_t n, const uint16_t* joints, const double* weights,
                     const double* palette, double* out);
void host_pose_palette(const int32_t* parents, const double* inverse_bind, uint32_t n_joints, const double* local, uint64_t local_stride,
                       uint64_t n_poses, double* palette, uint64_t palette_stride);
// trgl_mesh_edges over host arrays (every index checked by the caller: below n_vertices; returns the count) and trgl_edge_select (false,
// and nothing written, for a record out of range; *n_selected may be null).  Both may throw std::bad_alloc.
uint64_t host_mesh_edges(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, uint32_t* edges_out);
bool host_edge_select(const trgl_edge_params& P, const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                      const uint32_t* edges, uint64_t n_edges, uint8_t* codes_out, uint32_t* segments_out, uint32_t* colors_out, uint64_t* n_selected);
// trgl_subdiv_topology and trgl_subdiv_vertices over host arrays: false, and nothing written, for an entry the header refuses in host
// memory (an index, a record or a stencil word out of range, a pair that no record names).  The first may throw std::bad_alloc.
bool host_subdiv_topology(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t* edges, uint64_t n_edges,
                          uint32_t* indices_out, uint32_t* stencils_out);
bool host_subdiv_vertices(const trgl_subdiv_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* stencils, uint64_t n_edges,
                          double* out);
// trgl_mesh_weld over host arrays (every index checked by the caller: below n_vertices; 0 < n_vertices < 2^31; null outputs are not
// written; returns the count).  May throw std::bad_alloc.
uint64_t host_mesh_weld(const trgl_weld_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out);
// trgl_mesh_clean over host arrays (every index checked by the caller: below n_vertices; null outputs are not written; the vertex
// outputs only with TRGL_CLEAN_VERTICES); counts = { kept faces, kept vertices }.  May throw std::bad_alloc.
void host_mesh_clean(const trgl_clean_params& P, const uint32_t* indices, uint64_t n_faces, const double* vertices, uint64_t n_vertices,
                     uint32_t* indices_out, uint32_t* face_firsts_out, uint32_t* vremap_out, uint32_t* vfirsts_out, double* vertices_out,
                     uint64_t counts[2]);
// trgl_mesh_simplify over host arrays (as above; n_vertices > 0): host_mesh_weld, the means, host_mesh_clean.  May throw std::bad_alloc.
void host_mesh_simplify(const trgl_simplify_params& P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out, uint32_t* face_firsts_out,
                        uint64_t counts[2]);
// trgl_instance_boxes and trgl_frustum_boxes over host arrays (local_stride 0: one local box for every instance)
void host_instance_boxes(const double* local_boxes, int local_stride, const double* instances, int stride, uint64_t n, double* boxes_out);
void host_frustum_boxes(const double planes[24], const double* boxes, uint64_t n, bool merge, uint8_t* codes);
// the box filter of box_core.h over host images: dst (w / f) x (h / f) from src w x h; f in 1..TRGL_MAX_BOX_FACTOR, w / f and h / f >= 1
void host_box_filter(const uint8_t* src, int w, int h, int bpp, int f, uint8_t* dst);
// trgl_image_mipmaps and trgl_lod_stage over host arrays (mip_core.h): levels 1 .. L-1 into the packed layout; the four LOD doubles per row
void host_mipmaps(const uint8_t* src, int w, int h, int bpp, uint8_t* dst);
void host_lod_stage(const double viewport[16], const double* clip, double* vary, uint64_t n, int K, int uv_offset, int out_offset);
}  // namespace trgl
