// trgl_api.cpp — host side of the C ABI in include/trgl.h: context, HBM buffers, the flush pipeline.
//
// A flush runs, on the context's own HIP stream:
//   setup (per draw) -> scan(counts) -> expand -> stable radix passes by tile id -> bounds -> raster
// and is the batched equivalent of the reference's per-face loop of rasterize() calls
// (main.cpp:660-666): submission order is preserved per tile, so results are identical.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/trgl.h"
#include "launch.h"
#include "trgl_device.h"
#include "user_shaders.h"
#include "../shim/trgl_image.h"
#include "../shim/trgl_obj.h"

using namespace trgl;

static thread_local std::string g_create_error;
void trgl::set_global_error(const std::string& msg) { g_create_error = msg; }

struct StageChunk { char* base; size_t cap, used; };
struct trgl_ctx;

// the growth rule of most device buffers: 25 % + 1024 elements of headroom
static size_t headroom(size_t need) { return need + need / 4 + 1024; }
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
// ... and of the pair buffers: a multiple of 4 entries (k_radix_hist reads 16 bytes at a time, k_raster 4 entries), at most 0xffffe000 (grids are sized by
// cap + 4095 in 32 bits; a flush of 2^32 - 16 pairs and more is refused)
static size_t pair_capacity(size_t need) {
    const size_t ncap = (headroom(need) + 3) & ~size_t(3);
    return ncap > 0xffffe000ull ? 0xffffe000ull : ncap;
}

// a flush whose first half (setup + binning) has run and whose raster half is still to be launched (trgl_flush_begin)
// (builtin_shade: the flush has PHONG / EYE draws; user_kinds: bit i = it has draws of user kind TRGL_SHADER_USER_FIRST + i)
// direct: the binning queued by trgl_flush_begin reads k_setup's segments (seg); settled: the pair count has been looked at and the
// binning that leaves the lists is queued (settle_binning); fell_back: the direct path's kernels did nothing and k_expand's chain ran
struct PendingRaster { bool active = false; FrameParams fp; int flush_kind = 0; uint32_t cap = 0; int cur = 0; uint64_t N = 0;
                       bool builtin_shade = false; uint32_t user_kinds = 0;
                       bool direct = false, settled = false, fell_back = false; SegLayout seg{}; uint32_t nblk = 0; };
// a user shader registered on the context (trgl_register_shader_ex): its module and kernel - the shade kernel, or the raster kernel
// of a kind that may discard (TRGL_SHADER_MAY_DISCARD)
struct UserKind { hipModule_t mod; hipFunction_t fn; int K; bool may_discard; };
// a user vertex shader registered on the context (trgl_register_vertex_shader): its module and its vertex-stage kernel (vertex_user.h)
struct UserVertex { hipModule_t mod; hipFunction_t fn; int K; };

struct trgl_ctx {
    int device = 0;
    int num_cus = 256;          // multiProcessorCount of the device
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
    DevBuf<uint8_t> shadow_tmp;         // trgl_shadow_mask / trgl_framebuffer_modulate with a host mask: the W * H bytes on their way; grows on demand
    DevBuf<uint8_t> pp_out;             // trgl_postprocess: three [H][W][3] images + two 64-bit z-range keys, kept between calls
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
    uint64_t rule_pairs = 0, rule_nblk = 0;     // pairs and setup blocks of the last flush that had triangles: a, the input of seg_sizes()
    int last_direct = 0, last_fell_back = 0;
    DevBuf<uint32_t> tile_start;        // tile_start[bounds_half()] followed by tile_end[bounds_half()]: set together per flush (in 16-byte words)
    DevBuf<uint4> items; DevBuf<uint32_t> n_items;
    DevBuf<unsigned long long> item_stats;
    DevBuf<DrawDesc> draws_dev;
    DevBuf<DevStats> stats_dev;
    DevStats* stats_pinned = nullptr;

    uint64_t triangles_total = 0;       // our_gl.cpp:90 counts every call, host side
    uint64_t last_tris = 0, last_pairs = 0;
    // what trgl_debug_read reports of the last complete flush (valid until the next trgl_draw / trgl_clear)
    struct Snapshot { bool valid = false; FrameParams fp; uint64_t N = 0, P = 0, cap = 0, literal_tris = 0, large_tris = 0; int cur = 0;
                      int direct = 0, fell_back = 0; uint32_t seg_S = 0, seg_G = 0; } snap;

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

template <class T> int DevBuf<T>::alloc(trgl_ctx* c, size_t n) {
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); p = nullptr; cap = 0; }
    HIPCHK(c, hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
    return TRGL_OK;
}

template <class T> int DevBuf<T>::release(trgl_ctx* c) {
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); p = nullptr; cap = 0; }
    return TRGL_OK;
}

// pins the staged arrays of a draw call in progress: a flush it triggers does not recycle them
struct StageHold { trgl_ctx* c; explicit StageHold(trgl_ctx* x) : c(x) { ++c->stage_hold; } ~StageHold() { --c->stage_hold; } };

static int fail(trgl_ctx* c, int code, const char* msg) { c->err = msg; return code; }

static int reset_dev_stats(trgl_ctx* c) {
    DevStats s;
    s.fragments = 0;
    s.zmin_key = zkey(std::numeric_limits<double>::infinity());
    s.zmax_key = zkey(-std::numeric_limits<double>::infinity());
    s.min_x = INT32_MAX; s.min_y = INT32_MAX; s.max_x = INT32_MIN; s.max_y = INT32_MIN;
    s.pairs_total = 0; s.literal_tris = 0; s.large_tris = 0;
    s.zero_pos_key = s.zero_neg_key = TRGL_ZERO_KEY_EMPTY;
    s.zero_locked = 0; s.zero_sign = 0;
    for (int k = 0; k < 16; ++k) s.dbg[k] = 0;
    *c->stats_pinned = s;
    HIPCHK(c, hipMemcpyAsync(c->stats_dev.p, c->stats_pinned, sizeof(DevStats), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

// The context's state is about to change: launch the raster half that trgl_flush_begin left pending ...
static int end_pending_raster(trgl_ctx* c) { return c->rp.active ? trgl_flush_end(c) : TRGL_OK; }
// ... and submit the queued draws, which were made under the old state
static int flush_queued(trgl_ctx* c) { return c->draws.empty() ? TRGL_OK : trgl_flush(c); }
// everything queued, done
static int flush_sync(trgl_ctx* c) {
    int r = trgl_flush(c); if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

// the stream, the fixed-size buffers, the events and the initial state of a new context
static int init_ctx(trgl_ctx* c) {
    const size_t npx = (size_t)c->W * c->H;
    HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    int r;
    if ((r = c->fb.alloc(c, npx * c->bpp)) || (r = c->zb.alloc(c, npx)) || (r = c->tex_dev.alloc(c, TRGL_MAX_TEXTURES))) return r;
    HIPCHK(c, hipMemset(c->tex_dev.p, 0, sizeof(c->tex_host)));
    if ((r = c->tile_start.alloc(c, c->bounds_half() * 2 + 4))) return r;
    if ((r = c->n_items.alloc(c, 2))) return r;                    // work items of the flush
    HIPCHK(c, hipMemset(c->n_items.p, 0, 8));                       // k_fold_stats leaves it at 0 for the next flush
    if ((r = c->draws_dev.alloc(c, TRGL_MAX_DRAWS)) || (r = c->stats_dev.alloc(c, 1))) return r;
    HIPCHK(c, hipHostMalloc((void**)&c->stats_pinned, sizeof(DevStats)));
    if ((r = c->seg_flag.alloc(c, 4))) return r;
    HIPCHK(c, hipHostMalloc((void**)&c->seg_flag_pinned, 16));
    *c->seg_flag_pinned = 1;
    for (int i = 0; i < 6; ++i) HIPCHK(c, hipEventCreate(&c->ev[i]));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_pairs, hipEventDisableTiming));
    // init_viewport(0,0,W,H), our_gl.cpp:59-69
    trgl_init_viewport(c, 0, 0, c->W, c->H);
    return reset_dev_stats(c);
}

extern "C" {

const char* trgl_last_error(const trgl_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int trgl_create(int device, int width, int height, int bpp, trgl_ctx** out) {
    if (!out || width <= 0 || height <= 0 || width > 65535 || height > 65535 || !(bpp == 1 || bpp == 3 || bpp == 4)) {
        g_create_error = "trgl_create: bad arguments (width/height in 1..65535, bpp in {1,3,4})";
        return TRGL_E_INVALID;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return TRGL_E_HIP; }
    trgl_ctx* c = new trgl_ctx();
    c->device = device; c->W = width; c->H = height; c->bpp = bpp;
    c->tiles_x = (width + TRGL_TILE - 1) / TRGL_TILE;
    c->tiles_y = (height + TRGL_TILE - 1) / TRGL_TILE;
    c->strip_y0 = 0; c->strip_y1 = height;
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) c->num_cus = n; }
    std::memset(c->tex_host, 0, sizeof(c->tex_host));
    if (int r = init_ctx(c)) { g_create_error = c->err; trgl_destroy(c); return r; }
    *out = c;
    return TRGL_OK;
}

int trgl_destroy(trgl_ctx* c) {
    if (!c) return TRGL_E_INVALID;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& s : c->stage) (void)hipFree(s.base);
    for (int i = 0; i < TRGL_MAX_TEXTURES; ++i) if (c->tex_host[i].data) (void)hipFree((void*)c->tex_host[i].data);
    if (c->stats_pinned) (void)hipHostFree(c->stats_pinned);
    if (c->seg_flag_pinned) (void)hipHostFree(c->seg_flag_pinned);
    for (int i = 0; i < 6; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->ev_pairs) (void)hipEventDestroy(c->ev_pairs);
    if (c->ev_blur_w) (void)hipEventDestroy(c->ev_blur_w);
    if (c->blur_w_pinned) (void)hipHostFree(c->blur_w_pinned);
    for (auto& u : c->user) (void)hipModuleUnload(u.mod);
    for (auto& v : c->vertex) (void)hipModuleUnload(v.mod);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                   // (the device buffers free themselves)
    return TRGL_OK;
}

int trgl_set_viewport(trgl_ctx* c, const double m[16]) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (!m) return fail(c, TRGL_E_INVALID, "trgl_set_viewport: null matrix");
    if (std::memcmp(c->vp, m, sizeof(c->vp)) != 0 && (r = flush_queued(c))) return r;   // rasterize() reads Viewport at call time
    std::memcpy(c->vp, m, sizeof(c->vp));
    return TRGL_OK;
}

int trgl_init_viewport(trgl_ctx* c, int x, int y, int w, int h) {          // our_gl.cpp:59-69
    if (!c) return TRGL_E_INVALID;
    double m[16];
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) m[4 * r + k] = (r == k) ? 1.0 : 0.0;
    m[0] = w / 2.0; m[5] = h / 2.0; m[3] = x + w / 2.0; m[7] = y + h / 2.0; m[10] = 1.0; m[11] = 0.0;
    if (c->stream == nullptr || c->draws.empty()) { std::memcpy(c->vp, m, sizeof(m)); return TRGL_OK; }
    return trgl_set_viewport(c, m);
}

int trgl_clear(trgl_ctx* c, const uint8_t bgra[4], double z_clear) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if ((r = flush_queued(c))) return r;                                     // earlier draws come first
    static const uint8_t dflt[4] = { 0, 0, 0, 255 };                         // TGAColor(), tgaimage.h:33
    const uint8_t* p = bgra ? bgra : dflt;
    c->clear_color = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    c->clear_z = z_clear;
    c->clear_pending = true;
    c->snap.valid = false;
    return TRGL_OK;
}

int trgl_upload_texture(trgl_ctx* c, int slot, const uint8_t* texels, int w, int h, int bpp) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (slot < 0 || slot >= TRGL_MAX_TEXTURES) return fail(c, TRGL_E_INVALID, "trgl_upload_texture: bad slot");
    if ((r = flush_queued(c))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->tex_host[slot].data) { HIPCHK(c, hipFree((void*)c->tex_host[slot].data)); c->tex_host[slot] = DevTexture{ nullptr, 0, 0, 0, 0 }; }
    if (texels && w > 0 && h > 0) {
        if (!(bpp == 1 || bpp == 3 || bpp == 4)) return fail(c, TRGL_E_INVALID, "trgl_upload_texture: bpp must be 1, 3 or 4");
        uint8_t* d = nullptr; size_t bytes = (size_t)w * h * bpp;
        HIPCHK(c, hipMalloc((void**)&d, bytes + 8));         // +8: the samplers read each texel as one 4-byte load
        HIPCHK(c, hipMemset(d + bytes, 0, 8));
        HIPCHK(c, hipMemcpy(d, texels, bytes, hipMemcpyHostToDevice));
        c->tex_host[slot] = DevTexture{ d, w, h, bpp, 0 };
    }
    HIPCHK(c, hipMemcpy(c->tex_dev.p, c->tex_host, sizeof(c->tex_host), hipMemcpyHostToDevice));
    return TRGL_OK;
}

int trgl_set_strip(trgl_ctx* c, int y0, int y1) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (y0 < 0 || y1 > c->H || y0 > y1) return fail(c, TRGL_E_INVALID, "trgl_set_strip: need 0 <= y0 <= y1 <= H");
    if ((r = flush_queued(c))) return r;
    c->strip_y0 = y0; c->strip_y1 = y1;
    c->il_tiles = 0; c->il_world = 1; c->il_rank = 0;
    return TRGL_OK;
}

int trgl_set_interleave(trgl_ctx* c, int band_rows, int rank, int world) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (band_rows <= 0 || band_rows % TRGL_TILE || world < 1 || rank < 0 || rank >= world)
        return fail(c, TRGL_E_INVALID, "trgl_set_interleave: band_rows must be a positive multiple of 32, 0 <= rank < world");
    if ((r = flush_queued(c))) return r;
    c->strip_y0 = 0; c->strip_y1 = c->H;
    c->il_tiles = world > 1 ? band_rows / TRGL_TILE : 0; c->il_world = world; c->il_rank = rank;
    return TRGL_OK;
}

static int vary_count(int kind) {
    switch (kind) {
    case TRGL_SHADER_GOURAUD: return TRGL_VARY_GOURAUD;
    case TRGL_SHADER_PHONG: return TRGL_VARY_PHONG;
    case TRGL_SHADER_EYE: return TRGL_VARY_EYE;
    case TRGL_SHADER_CHECKER: return TRGL_VARY_CHECKER;
    default: return 0;
    }
}

// device memory from the per-flush arena; chunks live until the flush that uses them is done
static int stage_alloc(trgl_ctx* c, size_t bytes, void** dev) {
    size_t need = (bytes + 255) & ~size_t(255);
    StageChunk* ch = nullptr;
    for (auto& s : c->stage) if (s.cap - s.used >= need) { ch = &s; break; }
    if (!ch) {
        StageChunk s; s.cap = need > (size_t(64) << 20) ? need : (size_t(64) << 20); s.used = 0; s.base = nullptr;
        HIPCHK(c, hipMalloc((void**)&s.base, s.cap));
        c->stage.push_back(s); ch = &c->stage.back();
    }
    *dev = ch->base + ch->used; ch->used += need;
    return TRGL_OK;
}
// copy host data into the arena
static int stage_copy(trgl_ctx* c, const void* src, size_t bytes, void** dev) {
    int r = stage_alloc(c, bytes, dev); if (r) return r;
    HIPCHK(c, hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice));   // "copied before trgl_draw returns"
    return TRGL_OK;
}

// a registered user kind that may discard (its draws are rasterized by its own kernel, in flushes of their own)
static bool discarding_kind(const trgl_ctx* c, int kind) {
    return kind >= TRGL_SHADER_USER_FIRST && kind - TRGL_SHADER_USER_FIRST < (int)c->user.size() && c->user[kind - TRGL_SHADER_USER_FIRST].may_discard;
}

int trgl_draw(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* clip, const double* vary,
              const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const bool user = kind >= TRGL_SHADER_USER_FIRST && kind - TRGL_SHADER_USER_FIRST < (int)c->user.size();
    if ((kind < 0 || kind >= TRGL_NUM_SHADERS) && !user) return fail(c, TRGL_E_INVALID, "trgl_draw: unknown shader kind");
    if (n == 0) return TRGL_OK;
    c->snap.valid = false;
    if (!clip) return fail(c, TRGL_E_INVALID, "trgl_draw: clip is null");
    int K = user ? c->user[kind - TRGL_SHADER_USER_FIRST].K : vary_count(kind);
    if (K && !vary) return fail(c, TRGL_E_INVALID, "trgl_draw: this shader kind needs varyings");
    if ((kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE) && !u) return fail(c, TRGL_E_INVALID, "trgl_draw: PHONG/EYE need uniforms");
    if (kind == TRGL_SHADER_CHECKER && (!u || u->reserved < 1)) return fail(c, TRGL_E_INVALID, "trgl_draw: CHECKER needs uniforms with reserved = cells >= 1");
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return fail(c, TRGL_E_INVALID, "trgl_draw: bad mem_kind");
    if (c->queued_tris + n > 0xffffffffull && (r = trgl_flush(c))) return r;
    if (n > 0xffffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_draw: more than 2^32-1 triangles in one draw");

    const double* dclip = clip; const double* dvary = K ? vary : nullptr; const uint32_t* dcol = colors;
    StageHold hold(c);
    if (mem_kind == TRGL_MEM_HOST) {
        void* p = nullptr;
        if ((r = stage_copy(c, clip, n * 12 * sizeof(double), &p))) return r;
        dclip = (const double*)p;
        if (K) { if ((r = stage_copy(c, vary, n * K * sizeof(double), &p))) return r; dvary = (const double*)p; }
        if (colors) { if ((r = stage_copy(c, colors, n * sizeof(uint32_t), &p))) return r; dcol = (const uint32_t*)p; }
    }
    // a record addresses its triangle as (draw index, 24-bit index): split larger submissions
    for (uint64_t done = 0; done < n;) {
        uint64_t m = n - done; if (m > TRGL_DRAW_MAX_TRIS) m = TRGL_DRAW_MAX_TRIS;
        // a kind that may discard shares a flush only with draws of the same kind: its raster kernel runs the whole flush
        const bool kind_cut = !c->draws.empty() && c->draws.back().kind != kind && (discarding_kind(c, kind) || discarding_kind(c, c->draws.back().kind));
        if ((c->draws.size() >= TRGL_MAX_DRAWS || c->queued_tris + m > TRGL_FLUSH_MAX_TRIS || kind_cut) && (r = trgl_flush(c))) return r;
        DrawDesc d; std::memset(&d, 0, sizeof(d));
        d.n = (uint32_t)m; d.first = (uint32_t)c->queued_tris; d.kind = kind; d.K = K;
        if (u) d.u = *u; else { d.u.tex_diffuse = d.u.tex_normal = d.u.tex_specular = -1; }
        d.clip = dclip + done * 12;
        d.vary = dvary ? dvary + done * K : nullptr;
        d.colors = dcol ? dcol + done : nullptr;
        c->draws.push_back(d);
        c->queued_tris += m;
        done += m;
    }
    return TRGL_OK;
}

int trgl_draw_indexed(trgl_ctx* c, int kind, const trgl_uniforms* u, const double projection[16], const double* vertices,
                      int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const bool user24 = kind >= TRGL_SHADER_USER_FIRST && kind - TRGL_SHADER_USER_FIRST < (int)c->user.size() &&
                        c->user[kind - TRGL_SHADER_USER_FIRST].K == TRGL_VARY_PHONG;     // (its varyings: the PHONG layout)
    if (kind != TRGL_SHADER_PHONG && kind != TRGL_SHADER_EYE && !user24)
        return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: kind must be PHONG, EYE or a user kind registered with 24 varyings");
    if (!u || !projection || !vertices || !indices) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: null argument");
    if (stride < 8) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: vertex stride must be >= 8 doubles (pos3, normal3, uv2)");
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: bad mem_kind");
    if (n_faces == 0) return TRGL_OK;
    if (n_faces > 0xffffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, "trgl_draw_indexed: too many faces in one call");
    const double* dv = vertices; const uint32_t* di = indices;
    void* p = nullptr;
    StageHold hold(c);
    if (mem_kind == TRGL_MEM_HOST) {
        for (uint64_t k = 0; k < 3 * n_faces; ++k)
            if (indices[k] >= n_vertices) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: index out of range");
        if ((r = stage_copy(c, vertices, n_vertices * (size_t)stride * sizeof(double), &p))) return r;
        dv = (const double*)p;
        if ((r = stage_copy(c, indices, 3 * n_faces * sizeof(uint32_t), &p))) return r;
        di = (const uint32_t*)p;
    }
    double* clip = nullptr; double* vary = nullptr;
    if ((r = stage_alloc(c, n_faces * 12 * sizeof(double), &p))) return r;
    clip = (double*)p;
    if ((r = stage_alloc(c, n_faces * 24 * sizeof(double), &p))) return r;
    vary = (double*)p;
    launch_vertex_stage(c->stream, u->model_view, projection, dv, stride, di, (uint32_t)n_faces, clip, vary);
    HIPCHK(c, hipGetLastError());
    return trgl_draw(c, kind, u, clip, vary, nullptr, n_faces, TRGL_MEM_DEVICE);
}

void trgl_ssao_defaults(trgl_ssao_params* p) {      // main.cpp:317-321
    if (!p) return;
    p->num_directions = 8; p->steps_per_direction = 8; p->sample_radius = 16.0; p->occlusion_threshold = 1e-3; p->intensity = 0.35;
}

int trgl_postprocess(trgl_ctx* c, const trgl_ssao_params* params, uint8_t* zimg, uint8_t* ao, uint8_t* fin) {
    CHKCTX(c);
    trgl_ssao_params sp; trgl_ssao_defaults(&sp);
    if (params) sp = *params;
    if (sp.num_directions < 1 || sp.num_directions > 16 || sp.steps_per_direction < 1)
        return fail(c, TRGL_E_INVALID, "trgl_postprocess: 1..16 directions, >= 1 step");
    int r = flush_sync(c); if (r) return r;
    const size_t npx = (size_t)c->W * c->H;
    // three [H][W][3] images, each at a 16-byte boundary (the kernels store dwords: W * H need not be a multiple of 4), then the keys
    const size_t img = (npx * 3 + 15) & ~size_t(15);
    if ((r = c->pp_out.grow(c, img * 3 + 64))) return r;      // allocated once per context, not per call
    uint8_t* d_out = c->pp_out.p;
    unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(d_out + img * 3);
    uint8_t* d_z = d_out; uint8_t* d_ao = d_out + img; uint8_t* d_fin = d_out + img * 2;
    hipStream_t s = c->stream;
    if (zimg) launch_zimage(s, c->zb.p, c->W, c->H, d_keys, d_z);
    if (ao || fin) {
        double dx[16], dy[16];
        for (int d = 0; d < sp.num_directions; ++d) {         // main.cpp:333-334, host libm as in the reference
            double angle = 2.0 * 3.14159265358979323846 * d / sp.num_directions;
            dx[d] = std::cos(angle); dy[d] = std::sin(angle);
        }
        launch_ssao(s, c->zb.p, c->W, c->H, dx, dy, sp.num_directions, sp.steps_per_direction, sp.sample_radius,
                    sp.occlusion_threshold, sp.intensity, d_ao);
    }
    if (fin) {
        if (c->bpp < 3) return fail(c, TRGL_E_UNSUPPORTED, "trgl_postprocess: composite needs an RGB(A) framebuffer");
        launch_composite(s, c->fb.p, c->bpp, d_ao, c->W, c->H, d_fin);
    }
    HIPCHK(c, hipGetLastError());
    if (zimg) HIPCHK(c, hipMemcpyAsync(zimg, d_z, npx * 3, hipMemcpyDeviceToHost, s));
    if (ao) HIPCHK(c, hipMemcpyAsync(ao, d_ao, npx * 3, hipMemcpyDeviceToHost, s));
    if (fin) HIPCHK(c, hipMemcpyAsync(fin, d_fin, npx * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return TRGL_OK;
}

static int resolve_events(trgl_ctx* c) {
    if (!c->events_pending) return TRGL_OK;
    HIPCHK(c, hipEventSynchronize(c->ev[3]));
    float ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->phase_ms[TRGL_PHASE_SETUP] += ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->phase_ms[TRGL_PHASE_BIN] += ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); c->phase_ms[TRGL_PHASE_RASTER] += ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[3])); c->phase_ms[TRGL_PHASE_TOTAL] += ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[4], c->ev[5])); c->phase_ms[TRGL_PHASE_RASTER_KERNEL] += ms;
    c->flushes_timed++;
    c->events_pending = false;
    return TRGL_OK;
}

int trgl_flush(trgl_ctx* c) {
    CHKCTX(c);
    int r = trgl_flush_begin(c);
    return r ? r : trgl_flush_end(c);
}

// expand -> stable radix passes by tile id, the last of which leaves the per-tile bounds, for pair buffers of capacity `cap`.  All of
// it reads the pair count from device memory; when the count exceeds `cap` every kernel here does nothing.
// seg: the direct path - k_setup has left the pairs in its segments, no k_expand, and the first pass reads them from there.
static int queue_binning(trgl_ctx* c, const FrameParams& fp, uint32_t cap, int* cur_out, const SegLayout* seg) {
    hipStream_t s = c->stream;
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    const unsigned long long* pairs_dev = &c->stats_dev.p->pairs_total;
    int r;
    uint32_t blk_base = 0;
    const bool wide = ntiles > 65536;          // else tile id and block mask share one 32-bit sort word
    for (auto& d : c->draws) {
        if (seg) break;
        launch_expand(s, fp, d.first, d.n, c->tiles_x, c->cnt.p, c->blk_sums.p, c->chunk_off.p, blk_base, c->tilebox.p, c->keys[0].p, wide, c->vals[0].p,
                      c->bmask[0].p, pairs_dev, cap);
        blk_base += setup_num_blocks(d.n);
    }
    int key_bits = 1; while ((size_t(1) << key_bits) < ntiles) ++key_bits;
    int passes = (key_bits + 7) / 8;
    int bits_per = (key_bits + passes - 1) / passes;
    size_t hist_need = ((size_t)std::max(radix_num_workers(cap), seg ? seg_num_groups(*seg) : 0u) << bits_per) + 16;
    if ((r = c->hist.grow(c, hist_need))) return r;
    if ((r = c->scan_tmp.grow(c, 256 + 16))) return r;   // the digit totals of a pass (k_radix_scan_rows)
    int cur = 0;
    for (int ps = 0; ps < passes; ++ps) {
        const RadixPass rp{ c->keys[cur].p, c->vals[cur].p, c->bmask[cur].p, c->keys[cur ^ 1].p, c->vals[cur ^ 1].p, c->bmask[cur ^ 1].p,
                            c->tile_start.p, c->tile_end(), ps * bits_per, bits_per };
        launch_radix_pass(s, rp, wide, ps == passes - 1, pairs_dev, cap, c->hist.p, c->scan_tmp.p, ps == 0 ? seg : nullptr,
                          (seg && ps > 0) ? seg->flag : nullptr);
        cur ^= 1;
    }
    *cur_out = cur;
    return TRGL_OK;
}

// the six pair buffers grow together, to pair_capacity(need)
static int grow_pairs(trgl_ctx* c, size_t need) {
    const size_t ncap = pair_capacity(need);
    int r;
    for (int k = 0; k < 2; ++k)
        if ((r = c->keys[k].grow(c, need, ncap)) || (r = c->vals[k].grow(c, need, ncap)) || (r = c->bmask[k].grow(c, need, ncap))) return r;
    return TRGL_OK;
}

// The direct path's sizes for a flush expected to hold `avg` pairs per setup block, `chunk` pairs per block of the first radix pass:
// a segment of S = 1.5 avg + 128 slots, rounded up to a multiple of 64, and groups of G = 0.9 chunk / avg segments, at most 16 - the
// expected group then fills nine tenths of the radix block.  false: no such sizes (S beyond what k_setup's LDS holds, or groups of
// fewer than two blocks) - such a flush takes k_expand's chain from the start.
static bool seg_sizes(double avg, uint32_t chunk, uint32_t* S, uint32_t* G) {
    if (avg < 1.0) avg = 1.0;
    const uint64_t s = ((uint64_t)(avg * 1.5) + 128 + 63) & ~uint64_t(63);
    uint64_t g = (uint64_t)(0.9 * chunk / avg);
    if (g > 16) g = 16;
    if (s > 4096 || g < 2) return false;
    *S = (uint32_t)s; *G = (uint32_t)g;
    return true;
}
constexpr uint64_t SEG_MAX_BYTES = uint64_t(1) << 30;      // both segment buffers together; a flush that would need more takes k_expand's chain

// The pending flush's counts have reached pinned memory: queue again what the kernels queued by trgl_flush_begin left undone.  They did
// nothing when the pairs exceed the buffers (grown here, when may_grow) and, on the direct path, when the flush did not fit its
// segments or groups (k_chunk_spine's flag): that flush falls back to k_expand and the dense passes.  Shared by trgl_flush_end and
// trgl_debug_read (may_grow = false: a pending flush beyond the capacity stays as it is).  Also keeps the rule of the automatic
// choice: after a fallback the context stays on k_expand's chain until a flush's counts fit the sizes it would have been given.
static int settle_binning(trgl_ctx* c, bool may_grow) {
    PendingRaster& rp = c->rp;
    if (!rp.N || rp.settled) return TRGL_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_pairs));
    const unsigned long long P64 = c->stats_pinned->pairs_total;
    if (P64 > 0xffffe000ull) return TRGL_OK;              // (trgl_flush_end refuses the flush)
    const bool bad = *c->seg_flag_pinned != 0, over = P64 > rp.cap, fell = rp.direct && bad;
    if (over && !may_grow) return TRGL_OK;
    int r;
    if (over || fell) {
        if (over && (r = grow_pairs(c, (size_t)P64))) return r;
        if ((r = queue_binning(c, rp.fp, (uint32_t)c->keys[0].cap, &rp.cur, fell ? nullptr : (rp.direct ? &rp.seg : nullptr)))) return r;
        rp.cap = (uint32_t)c->keys[0].cap;
        if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    }
    if (c->bin_mode == 0) { if (fell) c->seg_hold = true; else if (!rp.direct && !bad) c->seg_hold = false; }
    rp.fell_back = fell; rp.settled = true;
    return TRGL_OK;
}

// what the kernels of the next flush need to know of the context's state
static FrameParams frame_params(const trgl_ctx* c) {
    FrameParams fp; std::memset(&fp, 0, sizeof(fp));
    fp.fb = c->fb.p; fp.zb = c->zb.p; fp.W = c->W; fp.H = c->H; fp.bpp = c->bpp;
    fp.tiles_x = c->tiles_x; fp.tiles_y = c->tiles_y;
    fp.strip_y0 = c->strip_y0; fp.strip_y1 = c->strip_y1;
    fp.strip_ty0 = c->strip_y0 / TRGL_TILE;
    fp.strip_ty1 = (c->strip_y1 + TRGL_TILE - 1) / TRGL_TILE;
    if (c->strip_y1 <= c->strip_y0) fp.strip_ty1 = fp.strip_ty0;
    fp.il_tiles = c->il_tiles; fp.il_world = c->il_world; fp.il_rank = c->il_rank;
    fp.init_from_clear = c->clear_pending ? 1 : 0;
    fp.n_tris = (uint32_t)c->queued_tris;
    fp.clear_color = c->clear_color; fp.clear_z = c->clear_z;
    std::memcpy(fp.vp, c->vp, sizeof(fp.vp));
    return fp;
}

// First half of a flush: per-triangle setup and the stable tile binning.  Touches neither the framebuffer nor the
// z-buffer, so a caller may let it overlap with whatever still reads them (bench.py: the RCCL gather of the
// previous frame's strips).  The host does not wait for anything here: the number of (tile, triangle) pairs stays on the
// device, the binning kernels are queued for the capacity the pair buffers already have (an earlier flush's count + 25 %,
// or 2 pairs per triangle the first time), and trgl_flush_end checks the count - which has reached pinned memory long
// before the binning is through - and queues them again in the rare case that the buffers were too small.
int trgl_flush_begin(trgl_ctx* c) {
    CHKCTX(c);
    if (c->rp.active) return TRGL_OK;
    if (c->draws.empty() && !c->clear_pending) return TRGL_OK;
    int r;
    if ((r = resolve_events(c))) return r;
    c->snap.valid = false;              // the buffers are about to be rewritten; trgl_debug_read reads the flush begun here
    const uint64_t N = c->queued_tris;
    hipStream_t s = c->stream;
    FrameParams fp = frame_params(c);

    int flush_kind = c->draws.empty() ? TRGL_SHADER_FLAT : c->draws[0].kind;     // one kind for the whole flush, or -1
    for (auto& d : c->draws) if (d.kind != flush_kind) flush_kind = -1;
    bool builtin_shade = false;
    uint32_t user_kinds = 0;           // (kinds that may discard are rasterized by their own kernel: no visibility buffer, no shade kernel)
    for (auto& d : c->draws) {
        if (d.kind == TRGL_SHADER_PHONG || d.kind == TRGL_SHADER_EYE) builtin_shade = true;
        if (d.kind >= TRGL_SHADER_USER_FIRST && !discarding_kind(c, d.kind)) user_kinds |= 1u << (d.kind - TRGL_SHADER_USER_FIRST);
        if (discarding_kind(c, d.kind) && d.kind != flush_kind) return fail(c, TRGL_E_STATE, "flush: a kind that may discard shares a flush with another kind");
    }
    if (builtin_shade || user_kinds) {                                            // shaded once per visible pixel (k_shade, shade_user.h)
        if ((r = c->idbuf.grow(c, (size_t)c->W * c->H))) return r;
        fp.idbuf = c->idbuf.p;
    }

    if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[0], s));
    uint32_t cap = 0;
    int cur = 0;
    if (N) {
        // the per-triangle buffers grow together (+ 1: the record behind the last one, k_make_items)
        const size_t tcap = headroom(N);
        if ((r = c->recs.grow(c, N + 1, tcap)) || (r = c->recs_w.grow(c, N + 1, tcap)) || (r = c->cnt.grow(c, N + 1, tcap)) ||
            (r = c->tilebox.grow(c, N + 1, tcap))) return r;
        if (c->keys[0].cap == 0 && (r = grow_pairs(c, (size_t)2 * N + 4096))) return r;      // first flush: a guess, checked in trgl_flush_end
        uint32_t nblk = 0;
        for (auto& d : c->draws) nblk += setup_num_blocks(d.n);
        if ((r = c->blk_sums.grow(c, (size_t)nblk + 16))) return r;
        if ((r = c->chunk_off.grow(c, (size_t)nblk / 16 + 16))) return r;
        cap = (uint32_t)c->keys[0].cap;
        // The path of the binning.  Automatic: direct with the sizes seg_sizes() gives for the pairs per setup block of the last flush
        // that had triangles (2 per triangle the first time), unless a flush fell back and none has fitted since (seg_hold) - then the
        // sizes are only checked.
        uint32_t S = 0, G = 0;
        bool direct = false;
        if ((size_t)c->tiles_x * c->tiles_y <= 65536) {
            if (c->bin_mode == 2) { S = c->bin_S; G = c->bin_G; direct = true; }
            else if (c->bin_mode == 0 && seg_sizes(c->rule_nblk ? (double)c->rule_pairs / (double)c->rule_nblk : 512.0, radix_chunk(cap), &S, &G))
                direct = !c->seg_hold && (uint64_t)nblk * S * 8 <= SEG_MAX_BYTES;      // (forced k_expand: S = 0, k_chunk_spine checks nothing)
        }
        if (direct && ((r = c->seg_keys.grow(c, (size_t)nblk * S + 4)) || (r = c->seg_vals.grow(c, (size_t)nblk * S + 4)))) return r;
        const SegLayout seg{ c->seg_keys.p, c->seg_vals.p, c->blk_sums.p, c->seg_flag.p, nblk, S, G };
        c->rp.direct = direct; c->rp.seg = seg; c->rp.nblk = nblk;
        {
            uint32_t blk_base = 0;
            for (size_t i = 0; i < c->draws.size(); ++i) {
                launch_setup(s, fp, c->draws[i], c->draws_dev.p, (int)i, c->draws[i].n, c->recs.p, c->recs_w.p, c->cnt.p, c->tilebox.p, c->stats_dev.p,
                             c->blk_sums.p, blk_base, direct ? &seg : nullptr);
                blk_base += setup_num_blocks(c->draws[i].n);
            }
        }
        if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[1], s));
        // (+ literal_tris, large_tris into pinned memory; the kernel also sets tile_start and tile_end to empty bounds)
        launch_chunk_spine(s, c->blk_sums.p, nblk, c->chunk_off.p, &c->stats_dev.p->pairs_total, &c->stats_pinned->pairs_total,
                           c->tile_start.p, c->bounds_half(), S, G, radix_chunk(cap), c->seg_flag.p, c->seg_flag_pinned);
        HIPCHK(c, hipEventRecord(c->ev_pairs, s));
        if ((r = queue_binning(c, fp, cap, &cur, direct ? &seg : nullptr))) return r;
    } else {
        c->rp.direct = false; c->rp.nblk = 0; c->rp.seg = SegLayout{};
        if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[1], s));
        HIPCHK(c, hipMemsetAsync(c->tile_start.p, 0, c->bounds_half() * 8, s));
    }
    if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[2], s));
    c->rp.active = true; c->rp.fp = fp; c->rp.flush_kind = flush_kind; c->rp.cap = cap; c->rp.cur = cur; c->rp.N = N;
    c->rp.builtin_shade = builtin_shade; c->rp.user_kinds = user_kinds;
    c->rp.settled = false; c->rp.fell_back = false;
    return TRGL_OK;
}

// Second half: the tile raster (and k_shade), the only part that reads or writes the framebuffer and the z-buffer.
int trgl_flush_end(trgl_ctx* c) {
    CHKCTX(c);
    if (!c->rp.active) return TRGL_OK;
    c->rp.active = false;
    int r;
    hipStream_t s = c->stream;
    FrameParams fp = c->rp.fp;
    const int flush_kind = c->rp.flush_kind;
    int cur = c->rp.cur;
    const uint64_t N = c->rp.N;
    uint32_t P = 0;
    if (N) {
        // the pair count was copied to pinned memory right after k_setup; the GPU is busy with the binning queued behind it
        HIPCHK(c, hipEventSynchronize(c->ev_pairs));
        const unsigned long long P64 = c->stats_pinned->pairs_total;
        if (P64 > 0xffffe000ull) {
            c->draws.clear(); c->queued_tris = 0;          // nothing of this flush was drawn (every binning kernel saw the overflow)
            return fail(c, TRGL_E_UNSUPPORTED, "flush: more than 2^32 triangle-tile pairs; submit in smaller batches");
        }
        P = (uint32_t)P64;
        if ((r = settle_binning(c, true))) return r;       // (the buffers were too small, or the direct path did not fit: binned again)
        cur = c->rp.cur;
    }
    // with no pairs every tile list is empty; the kernel must not (and does not) dereference these, but give it
    // valid addresses anyway
    const TriRec* recs_arg = c->recs.p ? c->recs.p : reinterpret_cast<const TriRec*>(c->tile_start.p);
    const uint32_t* vals_arg = (P && c->vals[cur].p) ? c->vals[cur].p : c->tile_start.p;
    const uint16_t* bmask_arg = (P && c->bmask[cur].p) ? c->bmask[cur].p : reinterpret_cast<const uint16_t*>(c->tile_start.p);
    // one work item (a workgroup of four block waves) per row of blocks of every owned tile
    const uint32_t max_items = raster_max_items(fp);
    if ((r = c->items.grow(c, (size_t)max_items + 64))) return r;
    if ((r = c->item_stats.grow(c, ((size_t)max_items + 64) * 4))) return r;
    // k_setup counted the triangles that are not well scaled (it came over with the pair count): without any, the kernel without the literal path
    const bool all_well_scaled = N == 0 || c->stats_pinned->literal_tris == 0;
    fp.zq_cull = (N != 0 && c->stats_pinned->large_tris != 0) ? 1 : 0;      // (k_setup counted them; the count came over with the pair count)
    UserShade user[TRGL_MAX_USER_SHADERS];
    int n_user = 0;
    for (int i = 0; i < (int)c->user.size(); ++i)
        if (c->rp.user_kinds >> i & 1u) user[n_user++] = UserShade{ c->user[i].fn, TRGL_SHADER_USER_FIRST + i };
    // a flush of a kind that may discard: its own raster kernel in place of k_raster
    const hipFunction_t user_raster = discarding_kind(c, flush_kind) ? c->user[flush_kind - TRGL_SHADER_USER_FIRST].fn : nullptr;
    launch_raster(s, fp, flush_kind, all_well_scaled, recs_arg, c->recs_w.p, vals_arg, bmask_arg, c->tile_start.p, c->tile_end(), c->draws_dev.p, c->tex_dev.p,
                  c->stats_dev.p, max_items, c->items.p, c->n_items.p, c->item_stats.p, c->rp.builtin_shade, user, n_user, user_raster,
                  c->profiling ? c->ev[4] : nullptr, c->profiling ? c->ev[5] : nullptr);
    if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[3], s)); c->events_pending = true; }
    HIPCHK(c, hipGetLastError());

    c->triangles_total += N;
    c->last_tris = N; c->last_pairs = P;
    if (N) { c->rule_pairs = P; c->rule_nblk = c->rp.nblk; }       // (a flush that only clears has no pairs per block: the rule keeps its input)
    c->last_direct = (N && c->rp.direct) ? 1 : 0; c->last_fell_back = (N && c->rp.fell_back) ? 1 : 0;
    c->snap.direct = c->last_direct; c->snap.fell_back = c->last_fell_back;
    c->snap.seg_S = N ? c->rp.seg.S : 0; c->snap.seg_G = N ? c->rp.seg.G : 0;
    c->snap.valid = true; c->snap.fp = fp; c->snap.N = N; c->snap.P = P; c->snap.cap = c->keys[0].cap; c->snap.cur = cur;
    c->snap.literal_tris = N ? c->stats_pinned->literal_tris : 0; c->snap.large_tris = N ? c->stats_pinned->large_tris : 0;
    c->clear_pending = false;
    bool had_stage = false;
    for (auto& ch : c->stage) if (ch.used) had_stage = true;
    c->draws.clear();
    c->queued_tris = 0;
    if (had_stage) {                       // staged data may be recycled only once the kernels are done ...
        HIPCHK(c, hipStreamSynchronize(s));
        if (!c->stage_hold)                // ... and not while a draw call in progress still owns staged arrays
            for (auto& ch : c->stage) ch.used = 0;
    }
    return TRGL_OK;
}

int trgl_register_shader_ex(trgl_ctx* c, const char* source, int n_varyings, uint32_t flags, int* kind) {
    CHKCTX(c);
    if (!kind) return fail(c, TRGL_E_INVALID, "trgl_register_shader: kind is null");
    if (c->user.size() >= TRGL_MAX_USER_SHADERS) return fail(c, TRGL_E_INVALID, "trgl_register_shader: TRGL_MAX_USER_SHADERS already registered");
    std::string log;
    const std::vector<char>* code = nullptr;
    if (int r = user_shader_code(source, n_varyings, flags, &log, &code)) { c->err = "trgl_register_shader: " + log; return r; }
    const bool may_discard = (flags & TRGL_SHADER_MAY_DISCARD) != 0;
    UserKind u{ nullptr, nullptr, n_varyings, may_discard };
    HIPCHK(c, hipModuleLoadData(&u.mod, code->data()));
    const hipError_t e = hipModuleGetFunction(&u.fn, u.mod, may_discard ? USER_RASTER_KERNEL : USER_SHADE_KERNEL);
    if (e != hipSuccess) {
        (void)hipModuleUnload(u.mod);
        c->err = std::string("hipModuleGetFunction: ") + hipGetErrorString(e);
        return TRGL_E_HIP;
    }
    c->user.push_back(u);
    *kind = TRGL_SHADER_USER_FIRST + (int)c->user.size() - 1;
    return TRGL_OK;
}

int trgl_register_shader(trgl_ctx* c, const char* source, int n_varyings, int* kind) {
    return trgl_register_shader_ex(c, source, n_varyings, 0u, kind);
}

// ---- user vertex shaders ------------------------------------------------------------------------------------------------
// the varyings per triangle of a kind trgl_draw accepts on this context, -1 for any other
static int kind_vary_count(const trgl_ctx* c, int kind) {
    if (kind >= 0 && kind < TRGL_NUM_SHADERS) return vary_count(kind);
    if (kind >= TRGL_SHADER_USER_FIRST && kind - TRGL_SHADER_USER_FIRST < (int)c->user.size()) return c->user[kind - TRGL_SHADER_USER_FIRST].K;
    return -1;
}

// The vertex stage of `vs` (-1: k_vertex_stage) over an indexed mesh in device memory, queued on the context's stream.  clip and
// vary (unused when K = 0) are 16-byte aligned; u == nullptr: zeros, texture slots -1.
static int queue_vertex_stage(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16], const double* dv, int stride,
                              const uint32_t* di, uint64_t n_faces, double* clip, double* vary) {
    if (vs < 0) {
        launch_vertex_stage(c->stream, u->model_view, projection, dv, stride, di, (uint32_t)n_faces, clip, vary);
        HIPCHK(c, hipGetLastError());
        return TRGL_OK;
    }
    VertexUserParams p; std::memset(&p, 0, sizeof(p));
    if (u) p.u = *u; else p.u.tex_diffuse = p.u.tex_normal = p.u.tex_specular = -1;
    std::memcpy(p.proj, projection, sizeof(p.proj));
    p.vertices = dv; p.indices = di; p.clip = clip; p.vary = vary; p.nfaces = (uint32_t)n_faces; p.stride = stride;
    void* args[] = { &p };
    const uint64_t blocks = (n_faces + TRGL_VERTEX_USER_FACES - 1) / TRGL_VERTEX_USER_FACES;
    HIPCHK(c, hipModuleLaunchKernel(c->vertex[vs].fn, (unsigned)blocks, 1, 1, TRGL_VERTEX_USER_FACES * 3, 1, 1, 0, c->stream, args, nullptr));
    return TRGL_OK;
}

// what trgl_draw_indexed_vs and trgl_vertex_stage check alike; K of the stage comes back in *K
static int check_vertex_call(trgl_ctx* c, const char* who, int vs, bool builtin_ok, const trgl_uniforms* u, const double* projection,
                             const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, int* K) {
    const std::string w(who);
    auto bad = [&](const char* msg) { c->err = w + ": " + msg; return TRGL_E_INVALID; };
    if (!((builtin_ok && vs == -1) || (vs >= 0 && vs < (int)c->vertex.size()))) return bad("unknown vertex shader");
    *K = vs < 0 ? TRGL_VARY_PHONG : c->vertex[vs].K;
    if (!projection || !vertices || !indices) return bad("null argument");
    if (vs < 0 && !u) return bad("the built-in vertex stage needs uniforms (model_view)");
    if (stride < (vs < 0 ? 8 : 1)) return bad(vs < 0 ? "vertex stride must be >= 8 doubles (pos3, normal3, uv2)" : "vertex stride must be >= 1");
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return bad("bad mem_kind");
    if (n_faces > 0xffffffffull / 3) { c->err = w + ": too many faces in one call"; return TRGL_E_UNSUPPORTED; }
    if (mem_kind == TRGL_MEM_HOST)
        for (uint64_t k = 0; k < 3 * n_faces; ++k)
            if (indices[k] >= n_vertices) return bad("index out of range");
    return TRGL_OK;
}

int trgl_register_vertex_shader(trgl_ctx* c, const char* source, int n_varyings, int* vs) {
    CHKCTX(c);
    if (!vs) return fail(c, TRGL_E_INVALID, "trgl_register_vertex_shader: vs is null");
    if (c->vertex.size() >= TRGL_MAX_USER_VERTEX_SHADERS) return fail(c, TRGL_E_INVALID, "trgl_register_vertex_shader: TRGL_MAX_USER_VERTEX_SHADERS already registered");
    std::string log;
    const std::vector<char>* code = nullptr;
    if (int r = user_vertex_shader_code(source, n_varyings, &log, &code)) { c->err = "trgl_register_vertex_shader: " + log; return r; }
    UserVertex v{ nullptr, nullptr, n_varyings };
    HIPCHK(c, hipModuleLoadData(&v.mod, code->data()));
    const hipError_t e = hipModuleGetFunction(&v.fn, v.mod, USER_VERTEX_KERNEL);
    if (e != hipSuccess) {
        (void)hipModuleUnload(v.mod);
        c->err = std::string("hipModuleGetFunction: ") + hipGetErrorString(e);
        return TRGL_E_HIP;
    }
    c->vertex.push_back(v);
    *vs = (int)c->vertex.size() - 1;
    return TRGL_OK;
}

int trgl_draw_indexed_vs(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16], const double* vertices,
                         int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, const uint32_t* colors, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = 0;
    if ((r = check_vertex_call(c, "trgl_draw_indexed_vs", vs, false, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &K))) return r;
    // (what trgl_draw would refuse is refused before the vertex stage is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: unknown shader kind");
    if (kind_K != K) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: the shader kind and the vertex shader differ in their number of varyings");
    if ((kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE) && !u) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: PHONG/EYE need uniforms");
    if (kind == TRGL_SHADER_CHECKER && (!u || u->reserved < 1)) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: CHECKER needs uniforms with reserved = cells >= 1");
    if (n_faces == 0) return TRGL_OK;
    const double* dv = vertices; const uint32_t* di = indices; const uint32_t* dcol = colors;
    void* p = nullptr;
    StageHold hold(c);
    if (mem_kind == TRGL_MEM_HOST) {
        if ((r = stage_copy(c, vertices, n_vertices * (size_t)stride * sizeof(double), &p))) return r;
        dv = (const double*)p;
        if ((r = stage_copy(c, indices, 3 * n_faces * sizeof(uint32_t), &p))) return r;
        di = (const uint32_t*)p;
        if (colors) { if ((r = stage_copy(c, colors, n_faces * sizeof(uint32_t), &p))) return r; dcol = (const uint32_t*)p; }
    }
    double* clip = nullptr; double* vary = nullptr;
    if ((r = stage_alloc(c, n_faces * 12 * sizeof(double), &p))) return r;
    clip = (double*)p;
    if (K) { if ((r = stage_alloc(c, n_faces * (size_t)K * sizeof(double), &p))) return r; vary = (double*)p; }
    if ((r = queue_vertex_stage(c, vs, u, projection, dv, stride, di, n_faces, clip, vary))) return r;
    return trgl_draw(c, kind, u, clip, vary, dcol, n_faces, TRGL_MEM_DEVICE);
}

int trgl_vertex_stage(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16], const double* vertices, int stride,
                      uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, double* clip_out, double* vary_out, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = 0;
    if ((r = check_vertex_call(c, "trgl_vertex_stage", vs, true, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &K))) return r;
    if (!clip_out || (K && !vary_out)) return fail(c, TRGL_E_INVALID, "trgl_vertex_stage: null output");
    if (n_faces == 0) return TRGL_OK;
    if (mem_kind == TRGL_MEM_DEVICE) {
        if (((uintptr_t)clip_out | (K ? (uintptr_t)vary_out : 0)) & 15) return fail(c, TRGL_E_INVALID, "trgl_vertex_stage: device outputs must be 16-byte aligned");
        return queue_vertex_stage(c, vs, u, projection, vertices, stride, indices, n_faces, clip_out, K ? vary_out : nullptr);
    }
    // host memory: through buffers of this call's own (nothing is left staged for a flush that may never come)
    DevBuf<double> d_v, d_clip, d_vary; DevBuf<uint32_t> d_i;
    if ((r = d_v.alloc(c, n_vertices * (size_t)stride)) || (r = d_i.alloc(c, 3 * n_faces)) || (r = d_clip.alloc(c, n_faces * 12)) ||
        (K && (r = d_vary.alloc(c, n_faces * (size_t)K)))) return r;
    HIPCHK(c, hipMemcpyAsync(d_v.p, vertices, n_vertices * (size_t)stride * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_i.p, indices, 3 * n_faces * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if ((r = queue_vertex_stage(c, vs, u, projection, d_v.p, stride, d_i.p, n_faces, d_clip.p, d_vary.p))) return r;
    HIPCHK(c, hipMemcpyAsync(clip_out, d_clip.p, n_faces * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (K) HIPCHK(c, hipMemcpyAsync(vary_out, d_vary.p, n_faces * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

int trgl_sync(trgl_ctx* c) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

int trgl_read_framebuffer(trgl_ctx* c, uint8_t* dst) {
    CHKCTX(c);
    if (!dst) return fail(c, TRGL_E_INVALID, "null destination");
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(dst, c->fb.p, (size_t)c->W * c->H * c->bpp, hipMemcpyDeviceToHost));
    return TRGL_OK;
}
int trgl_write_framebuffer(trgl_ctx* c, const uint8_t* src) {
    CHKCTX(c);
    if (!src) return fail(c, TRGL_E_INVALID, "null source");
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(c->fb.p, src, (size_t)c->W * c->H * c->bpp, hipMemcpyHostToDevice));
    return TRGL_OK;
}
int trgl_read_zbuffer(trgl_ctx* c, double* dst) {
    CHKCTX(c);
    if (!dst) return fail(c, TRGL_E_INVALID, "null destination");
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(dst, c->zb.p, (size_t)c->W * c->H * sizeof(double), hipMemcpyDeviceToHost));
    return TRGL_OK;
}
int trgl_write_zbuffer(trgl_ctx* c, const double* src) {
    CHKCTX(c);
    if (!src) return fail(c, TRGL_E_INVALID, "null source");
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(c->zb.p, src, (size_t)c->W * c->H * sizeof(double), hipMemcpyHostToDevice));
    return TRGL_OK;
}

int trgl_get_stats(trgl_ctx* c, trgl_stats* out) {
    CHKCTX(c);
    if (!out) return fail(c, TRGL_E_INVALID, "null stats");
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(c->stats_pinned, c->stats_dev.p, sizeof(DevStats), hipMemcpyDeviceToHost));
    const DevStats& s = *c->stats_pinned;
    out->triangles_rasterized = c->triangles_total;
    out->fragments_drawn = s.fragments;
    out->min_x = s.min_x; out->min_y = s.min_y; out->max_x = s.max_x; out->max_y = s.max_y;
    out->min_z = zkey_decode(s.zmin_key); out->max_z = zkey_decode(s.zmax_key);
    // +0.0 == -0.0: the reference keeps whichever zero it met first (std::min/max, our_gl.cpp:197-198)
    if (out->min_z == 0.0 && s.zero_locked) out->min_z = s.zero_sign ? -0.0 : 0.0;
    if (out->max_z == 0.0 && s.zero_locked) out->max_z = s.zero_sign ? -0.0 : 0.0;
    return TRGL_OK;
}

int trgl_reset_stats(trgl_ctx* c) {
    CHKCTX(c);
    int r = flush_sync(c); if (r) return r;
    c->triangles_total = 0;
    return reset_dev_stats(c);
}

int trgl_format_stats(const trgl_stats* s, char* buf, size_t buflen) {   // our_gl.cpp:205-209
    if (!s || !buf) return TRGL_E_INVALID;
    char lo[400], hi[400];      // "%f" of a double needs up to 317 characters
    if (std::isfinite(s->min_z)) std::snprintf(lo, sizeof lo, "%f", s->min_z); else std::snprintf(lo, sizeof lo, "inf");
    if (std::isfinite(s->max_z)) std::snprintf(hi, sizeof hi, "%f", s->max_z); else std::snprintf(hi, sizeof hi, "-inf");
    int n = std::snprintf(buf, buflen, "DEBUG: triangles=%llu fragments_drawn=%llu bbox=[%d,%d] - [%d,%d] z-range=[%s,%s]\n",
                          (unsigned long long)s->triangles_rasterized, (unsigned long long)s->fragments_drawn,
                          s->min_x, s->min_y, s->max_x, s->max_y, lo, hi);
    return (n < 0 || (size_t)n >= buflen) ? TRGL_E_INVALID : TRGL_OK;
}

// ---- scene logic around the draws (model.cpp:15-40, geometry.h:264-266,297-327, our_gl.cpp:212-280) ------------------------------
// std::min(a, b) = (b < a) ? b : a and std::max(a, b) = (a < b) ? b : a with a the running bound: what decides NaNs and signed zeros
static inline double keep_min(double bound, double p) { return p < bound ? p : bound; }
static inline double keep_max(double bound, double p) { return bound < p ? p : bound; }
// dot<n> (geometry.h:122-127): summed left to right from 0
static inline double dot3_from_zero(const double* a, double x, double y, double z) { double sum = 0; sum += a[0] * x; sum += a[1] * y; sum += a[2] * z; return sum; }

int trgl_mesh_bounds(trgl_ctx* c, const double* vertices, int stride, uint64_t n, int mem_kind, double out_min[3], double out_max[3]) {
    auto bad = [&](const char* msg) { if (c) c->err = msg; else g_create_error = msg; return TRGL_E_INVALID; };
    if (!out_min || !out_max) return bad("trgl_mesh_bounds: null output");
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return bad("trgl_mesh_bounds: bad mem_kind");
    if (stride < 3) return bad("trgl_mesh_bounds: vertex stride must be >= 3 doubles (the position)");
    if (n && !vertices) return bad("trgl_mesh_bounds: vertices is null");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return bad("trgl_mesh_bounds: TRGL_MEM_DEVICE needs a context");
    if (n == 0) {                                                               // model.cpp:16-19
        for (int a = 0; a < 3; ++a) out_min[a] = out_max[a] = 0.0;
        return TRGL_OK;
    }
    if (mem_kind == TRGL_MEM_HOST) {
        double lo[3] = { 1e9, 1e9, 1e9 }, hi[3] = { -1e9, -1e9, -1e9 };         // :21-22
        for (uint64_t i = 0; i < n; ++i) {
            const double* p = vertices + i * (uint64_t)stride;
            for (int a = 0; a < 3; ++a) lo[a] = keep_min(lo[a], p[a]);          // :25-27
            for (int a = 0; a < 3; ++a) hi[a] = keep_max(hi[a], p[a]);          // :29-31
        }
        for (int a = 0; a < 3; ++a) {
            const double margin = (hi[a] - lo[a]) * 0.01;                       // :35
            out_min[a] = lo[a] - margin; out_max[a] = hi[a] + margin;           // :36
        }
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (!c->bounds_scratch.p && (r = c->bounds_scratch.alloc(c, 1 + MESH_BOUNDS_MAX_BLOCKS))) return r;
    launch_mesh_bounds(c->stream, vertices, stride, n, c->bounds_scratch.p);
    HIPCHK(c, hipGetLastError());
    double res[6];
    HIPCHK(c, hipMemcpyAsync(res, c->bounds_scratch.p->v, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int a = 0; a < 3; ++a) { out_min[a] = res[a]; out_max[a] = res[3 + a]; }
    return TRGL_OK;
}

// ---- Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388) ----------------------
// norm (geometry.h:130-133) of three consecutive doubles
static inline double norm3_from_zero(const double* v) { return std::sqrt(dot3_from_zero(v, v[0], v[1], v[2])); }
// normalized (geometry.h:136-140): a zero vector comes back unchanged
static inline void normalize3(double* v) {
    const double length = norm3_from_zero(v);
    if (length == 0) return;
    for (int a = 0; a < 3; ++a) v[a] = v[a] / length;
}

static void host_mesh_normals(double* vertices, uint64_t stride, uint64_t n, const uint32_t* indices, uint64_t nfaces) {
    for (uint64_t i = 0; i < n; ++i) { double* nrm = vertices + i * stride + 3; nrm[0] = nrm[1] = nrm[2] = 0.0; }     // :283-285
    for (uint64_t f = 0; f < nfaces; ++f) {                                                                          // :288-305
        const double* v0 = vertices + indices[3 * f] * stride; const double* v1 = vertices + indices[3 * f + 1] * stride;
        const double* v2 = vertices + indices[3 * f + 2] * stride;
        double e1[3], e2[3];
        for (int a = 0; a < 3; ++a) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
        const double fn[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        for (int k = 0; k < 3; ++k) {
            double* nrm = vertices + indices[3 * f + k] * stride + 3;
            for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] + fn[a];
        }
    }
    for (uint64_t i = 0; i < n; ++i) {                                                                               // :308-315
        double* nrm = vertices + i * stride + 3;
        const double length = norm3_from_zero(nrm);
        if (length > 0.001) { for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] / length; }
        else { nrm[0] = 0; nrm[1] = 0; nrm[2] = 1; }
    }
}

static void host_mesh_tangents(double* vertices, uint64_t stride, uint64_t n, const uint32_t* indices, uint64_t nfaces) {
    for (uint64_t i = 0; i < n; ++i) { double* t = vertices + i * stride + 8; for (int a = 0; a < 6; ++a) t[a] = 0.0; }   // :332-335
    for (uint64_t f = 0; f < nfaces; ++f) {                                                                          // :338-368
        const double* v0 = vertices + indices[3 * f] * stride; const double* v1 = vertices + indices[3 * f + 1] * stride;
        const double* v2 = vertices + indices[3 * f + 2] * stride;
        double dp1[3], dp2[3];
        for (int a = 0; a < 3; ++a) { dp1[a] = v1[a] - v0[a]; dp2[a] = v2[a] - v0[a]; }
        const double duv1x = v1[6] - v0[6], duv1y = v1[7] - v0[7], duv2x = v2[6] - v0[6], duv2y = v2[7] - v0[7];
        const double r = duv1x * duv2y - duv2x * duv1y;                                                              // :353
        if (std::fabs(r) < 1e-8) continue;
        const double invr = 1.0 / r;
        double tangent[3], bitangent[3];
        for (int a = 0; a < 3; ++a) {
            tangent[a] = (dp1[a] * duv2y - dp2[a] * duv1y) * invr;                                                   // :358
            bitangent[a] = (dp2[a] * duv1x - dp1[a] * duv2x) * invr;                                                 // :359
        }
        for (int k = 0; k < 3; ++k) { double* t = vertices + indices[3 * f + k] * stride + 8; for (int a = 0; a < 3; ++a) t[a] = t[a] + tangent[a]; }
        for (int k = 0; k < 3; ++k) { double* b = vertices + indices[3 * f + k] * stride + 11; for (int a = 0; a < 3; ++a) b[a] = b[a] + bitangent[a]; }
    }
    for (uint64_t i = 0; i < n; ++i) {                                                                               // :371-387
        double* rec = vertices + i * stride;
        double* t = rec + 8; double* b = rec + 11;
        if (norm3_from_zero(t) > 0.001 && norm3_from_zero(rec + 3) > 0.001) {
            double nn[3] = { rec[3], rec[4], rec[5] };
            normalize3(nn);                                                                                          // :374
            normalize3(t);                                                                                           // :375
            const double d = dot3_from_zero(nn, t[0], t[1], t[2]);
            for (int a = 0; a < 3; ++a) t[a] = t[a] - nn[a] * d;                                                     // :378
            normalize3(t);
            b[0] = rec[4] * t[2] - rec[5] * t[1]; b[1] = rec[5] * t[0] - rec[3] * t[2]; b[2] = rec[3] * t[1] - rec[4] * t[0];   // :381
        } else {
            t[0] = 1; t[1] = 0; t[2] = 0; b[0] = 0; b[1] = 1; b[2] = 0;                                              // :384-385
        }
    }
}

static int mesh_attr(trgl_ctx* c, bool tangents, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces,
                     int mem_kind, int* generated) {
    const char* who = tangents ? "trgl_mesh_tangents" : "trgl_mesh_normals";
    auto bad = [&](const char* msg) { const std::string m = std::string(who) + ": " + msg; if (c) c->err = m; else g_create_error = m; return TRGL_E_INVALID; };
    const int field = tangents ? 8 : 3, min_stride = tangents ? 14 : 6;
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return bad("bad mem_kind");
    if (stride < min_stride) return bad(tangents ? "vertex stride must be >= 14 doubles (pos3, normal3, uv2, tangent3, bitangent3)"
                                                 : "vertex stride must be >= 6 doubles (pos3, normal3)");
    if (nfaces > 0xffffffffull / 3) return bad("3 * n_faces must fit in 32 bits");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return bad("TRGL_MEM_DEVICE needs a context");
    if (generated) *generated = 0;
    if (n == 0) return TRGL_OK;
    if (!vertices) return bad("vertices is null");
    if (nfaces && !indices) return bad("indices is null");
    if (mem_kind == TRGL_MEM_HOST) {
        for (uint64_t k = 0; k < 3 * nfaces; ++k)
            if (indices[k] >= n) return bad("index out of range");
        bool need = false;                                                      // :270-276 / :319-325
        for (uint64_t i = 0; i < n && !need; ++i) need = norm3_from_zero(vertices + i * (uint64_t)stride + field) < 0.001;
        if (!need) return TRGL_OK;
        if (tangents) host_mesh_tangents(vertices, (uint64_t)stride, n, indices, nfaces);
        else host_mesh_normals(vertices, (uint64_t)stride, n, indices, nfaces);
        if (generated) *generated = 1;
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    size_t bytes = 0;
    HIPCHK(c, mesh_attr_scratch_bytes(n, (uint32_t)nfaces, &bytes));
    if ((r = c->mesh_scratch.grow(c, bytes))) return r;
    const uint32_t* flag = nullptr;
    HIPCHK(c, launch_mesh_attr(c->stream, tangents, vertices, stride, n, indices, (uint32_t)nfaces, c->mesh_scratch.p, c->mesh_scratch.cap, &flag));
    if (generated) {
        uint32_t word = 0;
        HIPCHK(c, hipMemcpyAsync(&word, flag, sizeof(word), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *generated = word ? 1 : 0;
    }
    return TRGL_OK;
}

int trgl_mesh_normals(trgl_ctx* c, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces, int mem_kind, int* generated) {
    return mesh_attr(c, false, vertices, stride, n, indices, nfaces, mem_kind, generated);
}
int trgl_mesh_tangents(trgl_ctx* c, double* vertices, int stride, uint64_t n, const uint32_t* indices, uint64_t nfaces, int mem_kind, int* generated) {
    return mesh_attr(c, true, vertices, stride, n, indices, nfaces, mem_kind, generated);
}

int trgl_aabb_transform(const double bmin[3], const double bmax[3], const double m[16], double out_min[3], double out_max[3]) {
    if (!bmin || !bmax || !m || !out_min || !out_max) return TRGL_E_INVALID;
    double lo[3] = { 1e9, 1e9, 1e9 }, hi[3] = { -1e9, -1e9, -1e9 };             // geometry.h:309-310
    for (int i = 0; i < 8; ++i) {                                               // :300-307: corner i takes max.x for bit 0, max.y for bit 1, max.z for bit 2
        const double x = (i & 1) ? bmax[0] : bmin[0], y = (i & 2) ? bmax[1] : bmin[1], z = (i & 4) ? bmax[2] : bmin[2];
        double t[4];
        for (int row = 0; row < 4; ++row) {                                     // :314, mat * vec4(corner, 1.0): one dot<4> per row
            double sum = 0;
            sum += m[4 * row] * x; sum += m[4 * row + 1] * y; sum += m[4 * row + 2] * z; sum += m[4 * row + 3] * 1.0;
            t[row] = sum;
        }
        for (int a = 0; a < 3; ++a) {
            const double pos = t[a] / t[3];                                     // :315, no guard
            lo[a] = keep_min(lo[a], pos);                                       // :317-319
            hi[a] = keep_max(hi[a], pos);                                       // :321-323
        }
    }
    for (int a = 0; a < 3; ++a) { out_min[a] = lo[a]; out_max[a] = hi[a]; }
    return TRGL_OK;
}

int trgl_frustum_from_matrix(const double m[16], double planes[24]) {
    if (!m || !planes) return TRGL_E_INVALID;
    for (int pair = 0; pair < 3; ++pair)                                        // our_gl.cpp:217-250: LEFT/RIGHT with k = 0, BOTTOM/TOP 1, NEAR/FAR 2
        for (int side = 0; side < 2; ++side) {
            double* pl = planes + 4 * (2 * pair + side);
            for (int row = 0; row < 4; ++row)                                   // rows 0..2 give the normal, row 3 gives d
                pl[row] = side == 0 ? m[4 * row + 3] + m[4 * row + pair] : m[4 * row + 3] - m[4 * row + pair];
        }
    for (int i = 0; i < 6; ++i) {                                               // :253-259
        double* pl = planes + 4 * i;
        const double length = std::sqrt(dot3_from_zero(pl, pl[0], pl[1], pl[2]));
        if (length > 0.0) { pl[0] = pl[0] / length; pl[1] = pl[1] / length; pl[2] = pl[2] / length; pl[3] /= length; }
    }
    return TRGL_OK;
}

int trgl_frustum_intersects(const double planes[24], const double bmin[3], const double bmax[3]) {
    if (!planes || !bmin || !bmax) return TRGL_E_INVALID;
    for (int i = 0; i < 6; ++i) {                                               // our_gl.cpp:265-278
        const double* pl = planes + 4 * i;
        double positive[3] = { bmin[0], bmin[1], bmin[2] };                     // :269
        for (int a = 0; a < 3; ++a) if (pl[a] >= 0) positive[a] = bmax[a];      // :270-272
        if (dot3_from_zero(pl, positive[0], positive[1], positive[2]) + pl[3] < 0) return 0;   // :275, Plane::distance
    }
    return 1;
}

static int zsnap_slot(trgl_ctx* c, int slot, const char* who) {
    if (slot >= 0 && slot < TRGL_MAX_Z_SNAPSHOTS) return TRGL_OK;
    c->err = std::string(who) + ": slot must be 0.." + std::to_string(TRGL_MAX_Z_SNAPSHOTS - 1);
    return TRGL_E_INVALID;
}

int trgl_zbuffer_snapshot(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_snapshot"); if (r) return r;
    if ((r = trgl_flush(c))) return r;                // completes a begun flush, draws what is queued, runs a pending clear
    const size_t npx = (size_t)c->W * c->H;
    if (!c->zsnap[slot].p && c->zsnap[slot].alloc(c, npx)) return fail(c, TRGL_E_NOMEM, "trgl_zbuffer_snapshot: out of device memory");
    HIPCHK(c, hipMemcpyAsync(c->zsnap[slot].p, c->zb.p, npx * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return TRGL_OK;
}

int trgl_zbuffer_restore(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_restore"); if (r) return r;
    if (!c->zsnap[slot].p) return fail(c, TRGL_E_STATE, "trgl_zbuffer_restore: the slot holds no snapshot");
    if ((r = trgl_flush(c))) return r;                // what is queued was submitted against the depths as they are now
    HIPCHK(c, hipMemcpyAsync(c->zb.p, c->zsnap[slot].p, (size_t)c->W * c->H * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return TRGL_OK;
}

int trgl_zbuffer_snapshot_free(trgl_ctx* c, int slot) {
    CHKCTX(c);
    int r = zsnap_slot(c, slot, "trgl_zbuffer_snapshot_free"); if (r) return r;
    if ((r = end_pending_raster(c))) return r;
    return c->zsnap[slot].release(c);
}

// ---- TGAImage::gaussian_blur and TGAImage::scale (tgaimage.cpp:246-324) ------------------------------------------------------------
static int image_fail(trgl_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; else g_create_error = msg; return code; }

int trgl_gaussian_kernel(int radius, float* weights) {
    if (radius <= 0 || !weights) return image_fail(nullptr, TRGL_E_INVALID, "trgl_gaussian_kernel: need radius >= 1 and room for 2 * radius + 1 weights");
    if (radius > TRGL_MAX_BLUR_RADIUS) return image_fail(nullptr, TRGL_E_UNSUPPORTED, "trgl_gaussian_kernel: radius above 46340 (i * i overflows the reference's int)");
    trgl_image::gaussian_weights(radius, weights);
    return TRGL_OK;
}

// The weights of `radius` in c->blur_weights, uploaded on the stream unless the previous blur left the same ones there.
static int upload_blur_weights(trgl_ctx* c, int radius) {
    if (c->blur_radius == radius) return TRGL_OK;
    const size_t n = 2 * (size_t)radius + 1;
    if (!c->ev_blur_w) HIPCHK(c, hipEventCreateWithFlags(&c->ev_blur_w, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->ev_blur_w));            // the previous upload has read the pinned weights (no wait when none was queued)
    c->blur_radius = 0;
    if (n > c->blur_w_pinned_cap) {
        if (c->blur_w_pinned) { HIPCHK(c, hipHostFree(c->blur_w_pinned)); c->blur_w_pinned = nullptr; c->blur_w_pinned_cap = 0; }
        HIPCHK(c, hipHostMalloc((void**)&c->blur_w_pinned, headroom(n) * sizeof(float)));
        c->blur_w_pinned_cap = headroom(n);
    }
    if (int r = c->blur_weights.grow(c, n)) return r;
    trgl_image::gaussian_weights(radius, c->blur_w_pinned);
    HIPCHK(c, hipMemcpyAsync(c->blur_weights.p, c->blur_w_pinned, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_blur_w, c->stream));
    c->blur_radius = radius;
    return TRGL_OK;
}

// both passes of the blur over device memory, queued on the stream; nbytes = w * h * bpp
static int queue_blur(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, int radius, size_t nbytes) {
    int r = upload_blur_weights(c, radius); if (r) return r;
    if ((r = c->blur_tmp.grow(c, nbytes))) return r;
    launch_image_blur(c->stream, pixels, w, h, bpp, radius, c->blur_weights.p, c->blur_tmp.p);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_image_blur(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, int radius, int mem_kind) {
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return image_fail(c, TRGL_E_INVALID, "trgl_image_blur: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4) || w < 0 || h < 0) return image_fail(c, TRGL_E_INVALID, "trgl_image_blur: need w, h >= 0 and bpp in {1, 3, 4}");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return image_fail(c, TRGL_E_INVALID, "trgl_image_blur: TRGL_MEM_DEVICE needs a context");
    if (radius <= 0 || w == 0 || h == 0) return TRGL_OK;                         // tgaimage.cpp:272
    if (!pixels) return image_fail(c, TRGL_E_INVALID, "trgl_image_blur: pixels is null");
    if (radius > TRGL_MAX_BLUR_RADIUS) return image_fail(c, TRGL_E_UNSUPPORTED, "trgl_image_blur: radius above 46340 (i * i overflows the reference's int)");
    if ((int64_t)w * h * bpp > INT_MAX) return image_fail(c, TRGL_E_UNSUPPORTED, "trgl_image_blur: w * h * bpp above INT_MAX (the reference's int byte index overflows)");
    const size_t nbytes = (size_t)w * h * bpp;
    if (mem_kind == TRGL_MEM_HOST) {
        try {
            std::vector<float> weights(2 * (size_t)radius + 1);
            std::vector<uint8_t> tmp(nbytes);
            trgl_image::gaussian_weights(radius, weights.data());
            trgl_image::blur_bytes(pixels, w, h, bpp, radius, weights.data(), tmp.data());
        } catch (const std::bad_alloc&) { return image_fail(c, TRGL_E_NOMEM, "trgl_image_blur: out of memory"); }
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    return queue_blur(c, pixels, w, h, bpp, radius, nbytes);
}

int trgl_image_scale(trgl_ctx* c, const uint8_t* src, int w, int h, int bpp, uint8_t* dst, int w2, int h2, int mem_kind) {
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4)) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: bpp must be 1, 3 or 4");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: TRGL_MEM_DEVICE needs a context");
    if (w2 <= 0 || h2 <= 0 || w <= 0 || h <= 0) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: a size <= 0 or an empty source (the reference returns false)");   // tgaimage.cpp:247
    if (!src || !dst) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: null image");
    if ((int64_t)(w2 - 1) * w > INT_MAX || (int64_t)(h2 - 1) * h > INT_MAX || (int64_t)w2 * h2 * bpp > INT_MAX || (int64_t)w * h * bpp > INT_MAX)
        return image_fail(c, TRGL_E_UNSUPPORTED, "trgl_image_scale: (w2 - 1) * w, (h2 - 1) * h or a byte count above INT_MAX (the reference's int arithmetic overflows)");
    const size_t nsrc = (size_t)w * h * bpp, ndst = (size_t)w2 * h2 * bpp;
    if ((uintptr_t)src < (uintptr_t)dst + ndst && (uintptr_t)dst < (uintptr_t)src + nsrc) return image_fail(c, TRGL_E_INVALID, "trgl_image_scale: src and dst overlap");
    if (mem_kind == TRGL_MEM_HOST) { trgl_image::scale_bytes(src, w, h, bpp, dst, w2, h2); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_image_scale(c->stream, src, w, h, bpp, dst, w2, h2);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_framebuffer_blur(trgl_ctx* c, int radius) {
    CHKCTX(c);
    if (c->strip_y0 != 0 || c->strip_y1 != c->H || c->il_world > 1)
        return fail(c, TRGL_E_STATE, "trgl_framebuffer_blur: the context owns a strip or interleaved bands; the vertical pass would read rows of another rank");
    if (radius <= 0) return TRGL_OK;                                             // tgaimage.cpp:272
    if (radius > TRGL_MAX_BLUR_RADIUS) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_blur: radius above 46340 (i * i overflows the reference's int)");
    if ((int64_t)c->W * c->H * c->bpp > INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_blur: W * H * bpp above INT_MAX (the reference's int byte index overflows)");
    int r = trgl_flush(c); if (r) return r;          // completes a begun flush, draws what is queued, runs a pending clear
    return queue_blur(c, c->fb.p, c->W, c->H, c->bpp, radius, (size_t)c->W * c->H * c->bpp);
}

// ---- the shadow post-pass (include/trgl.h; host loops in shim/trgl_image.h, kernels in kernels_shadow.hip) ----------------------------
static int check_shadow_params(trgl_ctx* c, const char* who, const trgl_shadow_params* p) {
    const std::string w(who);
    if (!p) return image_fail(c, TRGL_E_INVALID, w + ": params is null");
    if (p->pcf_radius < 0 || p->pcf_radius > TRGL_MAX_PCF_RADIUS || p->reserved != 0)
        return image_fail(c, TRGL_E_INVALID, w + ": need pcf_radius in 0.." + std::to_string(TRGL_MAX_PCF_RADIUS) + " and reserved == 0");
    if (!(p->darkness >= 0.0 && p->darkness <= 1.0) || !std::isfinite(p->bias))
        return image_fail(c, TRGL_E_INVALID, w + ": need darkness in [0, 1] and a finite bias");
    return TRGL_OK;
}

static ShadowArgs shadow_args(const trgl_shadow_params* p, const double* depth, int w, int h, const double* map, int map_w, int map_h, uint8_t* mask) {
    ShadowArgs a;
    std::memcpy(a.M, p->screen_to_light, sizeof(a.M));
    a.bias = p->bias; a.darkness = p->darkness;
    a.depth = depth; a.map = map; a.mask = mask;
    a.w = w; a.h = h; a.map_w = map_w; a.map_h = map_h; a.radius = p->pcf_radius;
    return a;
}

int trgl_shadow_matrix(const double light_mv[16], const double light_proj[16], const double light_vp[16],
                       const double cam_mv[16], const double cam_proj[16], const double cam_vp[16], double out[16]) {
    if (!light_mv || !light_proj || !light_vp || !cam_mv || !cam_proj || !cam_vp || !out)
        return image_fail(nullptr, TRGL_E_INVALID, "trgl_shadow_matrix: null matrix");
    auto mul = [](const double* a, const double* b, double* r) {                     // geometry.h:196-205
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double sum = 0;
                for (int k = 0; k < 4; ++k) sum += a[4 * i + k] * b[4 * k + j];
                r[4 * i + j] = sum;
            }
    };
    double t[16], L[16], Cm[16], inv[16];
    mul(light_vp, light_proj, t); mul(t, light_mv, L);                               // Viewport * Perspective * ModelView, left to right
    mul(cam_vp, cam_proj, t); mul(t, cam_mv, Cm);
    // Gauss-Jordan with partial pivoting on [Cm | I]
    for (int i = 0; i < 16; ++i) inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(Cm[4 * r + col]) > std::fabs(Cm[4 * piv + col])) piv = r;
        const double pv = Cm[4 * piv + col];
        if (pv == 0.0 || !std::isfinite(pv)) return image_fail(nullptr, TRGL_E_INVALID, "trgl_shadow_matrix: the camera's matrix is singular (a pivot is 0 or not finite)");
        if (piv != col)
            for (int k = 0; k < 4; ++k) { std::swap(Cm[4 * piv + k], Cm[4 * col + k]); std::swap(inv[4 * piv + k], inv[4 * col + k]); }
        for (int k = 0; k < 4; ++k) { Cm[4 * col + k] /= pv; inv[4 * col + k] /= pv; }
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = Cm[4 * r + col];
            for (int k = 0; k < 4; ++k) { Cm[4 * r + k] -= f * Cm[4 * col + k]; inv[4 * r + k] -= f * inv[4 * col + k]; }
        }
    }
    mul(L, inv, t);
    std::memcpy(out, t, sizeof(t));
    return TRGL_OK;
}

int trgl_shadow_mask_image(trgl_ctx* c, const trgl_shadow_params* params, const double* depth, int w, int h,
                           const double* map, int map_w, int map_h, uint8_t* mask, int mem_kind) {
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return image_fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: bad mem_kind");
    if (int r = check_shadow_params(c, "trgl_shadow_mask_image", params)) return r;
    if (w < 0 || h < 0 || map_w < 0 || map_h < 0) return image_fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: a negative dimension");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return image_fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: TRGL_MEM_DEVICE needs a context");
    if (w == 0 || h == 0) return TRGL_OK;
    if (map_w == 0 || map_h == 0) return image_fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: an empty depth map");
    if (!depth || !map || !mask) return image_fail(c, TRGL_E_INVALID, "trgl_shadow_mask_image: null array");
    if ((int64_t)w * h > INT_MAX || (int64_t)map_w * map_h > INT_MAX) return image_fail(c, TRGL_E_UNSUPPORTED, "trgl_shadow_mask_image: w * h or map_w * map_h above INT_MAX");
    if (mem_kind == TRGL_MEM_HOST) {
        trgl_image::shadow_mask_bytes(depth, w, h, params->screen_to_light, map, map_w, map_h, params->bias, params->darkness, params->pcf_radius, mask);
        return TRGL_OK;
    }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_shadow_mask(c->stream, shadow_args(params, depth, w, h, map, map_w, map_h, mask));
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_shadow_mask(trgl_ctx* c, const trgl_shadow_params* params, int slot, uint8_t* mask, int mask_mem_kind) {
    CHKCTX(c);
    if (mask_mem_kind != TRGL_MEM_HOST && mask_mem_kind != TRGL_MEM_DEVICE) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask: bad mask_mem_kind");
    int r = check_shadow_params(c, "trgl_shadow_mask", params); if (r) return r;
    if ((r = zsnap_slot(c, slot, "trgl_shadow_mask"))) return r;
    if (!mask) return fail(c, TRGL_E_INVALID, "trgl_shadow_mask: mask is null");
    if (c->strip_y0 != 0 || c->strip_y1 != c->H || c->il_world > 1)
        return fail(c, TRGL_E_STATE, "trgl_shadow_mask: the context owns a strip or interleaved bands; its snapshot holds only this rank's rows (gather with with_z and mask on one context)");
    if (!c->zsnap[slot].p) return fail(c, TRGL_E_STATE, "trgl_shadow_mask: the slot holds no snapshot");
    const size_t npx = (size_t)c->W * c->H;
    if (npx > (size_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_shadow_mask: W * H above INT_MAX");
    if ((r = trgl_flush(c))) return r;                // completes a begun flush, draws what is queued, runs a pending clear
    uint8_t* d_mask = mask;
    if (mask_mem_kind == TRGL_MEM_HOST) { if ((r = c->shadow_tmp.grow(c, npx))) return r; d_mask = c->shadow_tmp.p; }
    launch_shadow_mask(c->stream, shadow_args(params, c->zb.p, c->W, c->H, c->zsnap[slot].p, c->W, c->H, d_mask));
    HIPCHK(c, hipGetLastError());
    if (mask_mem_kind == TRGL_MEM_HOST) {
        HIPCHK(c, hipMemcpyAsync(mask, d_mask, npx, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return TRGL_OK;
}

int trgl_image_modulate(trgl_ctx* c, uint8_t* pixels, int w, int h, int bpp, const uint8_t* mask, int mem_kind) {
    if (mem_kind != TRGL_MEM_HOST && mem_kind != TRGL_MEM_DEVICE) return image_fail(c, TRGL_E_INVALID, "trgl_image_modulate: bad mem_kind");
    if (!(bpp == 1 || bpp == 3 || bpp == 4) || w < 0 || h < 0) return image_fail(c, TRGL_E_INVALID, "trgl_image_modulate: need w, h >= 0 and bpp in {1, 3, 4}");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return image_fail(c, TRGL_E_INVALID, "trgl_image_modulate: TRGL_MEM_DEVICE needs a context");
    if (w == 0 || h == 0) return TRGL_OK;
    if (!pixels || !mask) return image_fail(c, TRGL_E_INVALID, "trgl_image_modulate: null image");
    if ((int64_t)w * h * bpp > INT_MAX) return image_fail(c, TRGL_E_UNSUPPORTED, "trgl_image_modulate: w * h * bpp above INT_MAX");
    if (mem_kind == TRGL_MEM_HOST) { trgl_image::modulate_bytes(pixels, (size_t)w * h, bpp, mask); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    launch_modulate(c->stream, pixels, (uint64_t)w * h, bpp, mask);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_framebuffer_modulate(trgl_ctx* c, const uint8_t* mask, int mask_mem_kind) {
    CHKCTX(c);
    if (mask_mem_kind != TRGL_MEM_HOST && mask_mem_kind != TRGL_MEM_DEVICE) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_modulate: bad mask_mem_kind");
    if (!mask) return fail(c, TRGL_E_INVALID, "trgl_framebuffer_modulate: mask is null");
    const size_t npx = (size_t)c->W * c->H;
    if (npx * c->bpp > (size_t)INT_MAX) return fail(c, TRGL_E_UNSUPPORTED, "trgl_framebuffer_modulate: W * H * bpp above INT_MAX");
    int r = trgl_flush(c); if (r) return r;          // completes a begun flush, draws what is queued, runs a pending clear
    if (mask_mem_kind == TRGL_MEM_HOST) {
        if ((r = c->shadow_tmp.grow(c, npx))) return r;
        // in stream order behind an earlier modulate that may still read shadow_tmp; a pinned mask is read when the stream gets here (include/trgl.h)
        HIPCHK(c, hipMemcpyAsync(c->shadow_tmp.p, mask, npx, hipMemcpyHostToDevice, c->stream));
        mask = c->shadow_tmp.p;
    }
    launch_modulate(c->stream, c->fb.p, npx, c->bpp, mask);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

void* trgl_framebuffer_device_ptr(trgl_ctx* c) { return c ? c->fb.p : nullptr; }
void* trgl_zbuffer_device_ptr(trgl_ctx* c) { return c ? c->zb.p : nullptr; }
void* trgl_stream(trgl_ctx* c) { return c ? (void*)c->stream : nullptr; }

int trgl_obj_load(const char* path, double** vertices, uint64_t* n_vertices, uint32_t** indices, uint64_t* n_faces) {
    if (!path || !vertices || !n_vertices || !indices || !n_faces) return TRGL_E_INVALID;
    trgl_obj::Mesh m;
    try {
        if (!trgl_obj::load(path, m)) { g_create_error = m.error; return TRGL_E_INVALID; }
    } catch (const std::bad_alloc&) {
        g_create_error = "trgl_obj_load: out of memory"; return TRGL_E_NOMEM;
    }
    *n_vertices = m.vertices.size() / 14; *n_faces = m.indices.size() / 3;
    *vertices = (double*)std::malloc(m.vertices.size() * sizeof(double) + 8);
    *indices = (uint32_t*)std::malloc(m.indices.size() * sizeof(uint32_t) + 8);
    if (!*vertices || !*indices) { std::free(*vertices); std::free(*indices); return TRGL_E_NOMEM; }
    std::memcpy(*vertices, m.vertices.data(), m.vertices.size() * sizeof(double));
    std::memcpy(*indices, m.indices.data(), m.indices.size() * sizeof(uint32_t));
    return TRGL_OK;
}
void trgl_obj_free(double* vertices, uint32_t* indices) { std::free(vertices); std::free(indices); }

size_t trgl_tga_max_size(int w, int h, int bpp) {
    if (w <= 0 || h <= 0 || bpp <= 0) return 18;
    return size_t(18) + size_t(w) * h * bpp + size_t(w) * h;      // every pixel its own literal packet
}

int trgl_tga_encode(const uint8_t* pixels, int w, int h, int bpp, int vflip, int rle, uint8_t* out, size_t* out_len) {
    if (!pixels || !out || !out_len || w <= 0 || h <= 0 || w > 65535 || h > 65535 || !(bpp == 1 || bpp == 3 || bpp == 4)) return TRGL_E_INVALID;
    try {
        TGAImage img(w, h, bpp);
        std::memcpy(img.buffer(), pixels, size_t(w) * h * bpp);
        std::vector<uint8_t> bytes = img.encode_tga(vflip != 0, rle != 0);
        std::memcpy(out, bytes.data(), bytes.size());
        *out_len = bytes.size();
    } catch (const std::bad_alloc&) {
        return TRGL_E_NOMEM;
    }
    return TRGL_OK;
}

int trgl_tga_info(const uint8_t* file, size_t size, int* width, int* height, int* bpp) {
    if (!file || !width || !height || !bpp || size < 18) return TRGL_E_INVALID;            // tgaimage.cpp:85-90
    const int w = file[12] | (file[13] << 8), h = file[14] | (file[15] << 8), b = file[16] >> 3;
    if (w <= 0 || h <= 0 || (b != 1 && b != 3 && b != 4)) return TRGL_E_INVALID;           // :96-99
    if (!(file[2] == 2 || file[2] == 3 || file[2] == 10 || file[2] == 11)) return TRGL_E_INVALID;   // :113-116
    *width = w; *height = h; *bpp = b;
    return TRGL_OK;
}

int trgl_tga_decode(const uint8_t* file, size_t size, uint8_t* pixels) {
    if (!file || !pixels) return TRGL_E_INVALID;
    try {                                          // a header may claim 65535 x 65535 x 4 bytes: nothing throws across the C ABI
        TGAImage img;
        if (!img.decode_tga(file, size)) return TRGL_E_INVALID;
        std::memcpy(pixels, img.buffer(), size_t(img.width()) * img.height() * img.bytespp());
    } catch (const std::bad_alloc&) {
        return TRGL_E_NOMEM;
    }
    return TRGL_OK;
}

int trgl_selftest_division(trgl_ctx* c, uint64_t samples, uint64_t seed, uint64_t* mismatches) {
    CHKCTX(c);
    if (!mismatches) return fail(c, TRGL_E_INVALID, "null mismatches");
    int r = trgl_flush(c); if (r) return r;
    DevBuf<unsigned long long> d;
    if ((r = d.alloc(c, 1))) return r;
    HIPCHK(c, hipMemsetAsync(d.p, 0, 8, c->stream));
    unsigned long long per_thread = (samples + 1024ull * 256 - 1) / (1024ull * 256);
    launch_selftest_division(c->stream, per_thread, seed, d.p);
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mismatches = h;
    return TRGL_OK;
}

int trgl_selftest_sampler(trgl_ctx* c, int slot, const double* uv, uint64_t n, uint8_t* out) {
    CHKCTX(c);
    if (!uv || !out) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler: null argument");
    if (slot < 0 || slot >= TRGL_MAX_TEXTURES) return fail(c, TRGL_E_INVALID, "trgl_selftest_sampler: bad slot");
    int r = trgl_flush(c); if (r) return r;
    if (!n) return TRGL_OK;
    DevBuf<double> d_uv; DevBuf<uint8_t> d_out;
    if ((r = d_uv.alloc(c, n * 2)) || (r = d_out.alloc(c, n * 5))) return r;
    HIPCHK(c, hipMemcpyAsync(d_uv.p, uv, n * 16, hipMemcpyHostToDevice, c->stream));
    launch_selftest_sampler(c->stream, c->tex_dev.p, slot, d_uv.p, n, d_out.p);
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, n * 5, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRGL_OK;
}

int trgl_set_stream(trgl_ctx* c, void* hip_stream, int use_own) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if ((r = flush_queued(c))) return r;           // a pending clear alone needs no launch: it stays pending
    if ((r = resolve_events(c))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // a NULL hipStream_t is a real stream (the legacy default stream, which is what torch's current stream
    // usually is), so "go back to the context's own stream" is a separate flag
    c->stream = use_own ? c->own_stream : (hipStream_t)hip_stream;
    return TRGL_OK;
}

int trgl_set_profiling(trgl_ctx* c, int on) {
    CHKCTX(c);
    int r = resolve_events(c); if (r) return r;
    c->profiling = on != 0;
    return TRGL_OK;
}
int trgl_get_phase_ms(trgl_ctx* c, double ms[TRGL_NUM_PHASES], uint64_t* flushes) {
    CHKCTX(c);
    int r = resolve_events(c); if (r) return r;
    if (ms) for (int i = 0; i < TRGL_NUM_PHASES; ++i) ms[i] = c->phase_ms[i];
    if (flushes) *flushes = c->flushes_timed;
    return TRGL_OK;
}
int trgl_reset_phase_ms(trgl_ctx* c) {
    CHKCTX(c);
    int r = resolve_events(c); if (r) return r;
    for (int i = 0; i < TRGL_NUM_PHASES; ++i) c->phase_ms[i] = 0;
    c->flushes_timed = 0;
    return TRGL_OK;
}
// diagnostic builds (-DTRGL_DEBUG_COUNTERS): k_raster work counters since the last stats reset
extern "C" int trgl_debug_counters(trgl_ctx* c, unsigned long long out[16]) {
    CHKCTX(c);
    int r = flush_sync(c); if (r) return r;
    HIPCHK(c, hipMemcpy(c->stats_pinned, c->stats_dev.p, sizeof(DevStats), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out[k] = c->stats_pinned->dbg[k];
    return TRGL_OK;
}

// Diagnostic read-back of one flush's intermediate buffers (tests/test_stage_outputs_gpu.py; not part of include/trgl.h).
// Valid between trgl_flush_begin and trgl_flush_end - the one entry point that does NOT complete a begun flush - and after a
// complete flush until the next trgl_draw / trgl_clear; TRGL_E_STATE otherwise.  Synchronises the stream and copies device ->
// host; launches nothing unless the pending flush fell back from the direct path: then k_expand's chain is queued first, as
// trgl_flush_end would (settle_binning).  *needed receives the size in bytes of `what`; with dst == nullptr that is all the call does.
//   what 0 RECS       TriRec[N + 1]   (the record behind the last is written by the raster half)
//        1 CNT        uint32[N]       2 TILEBOX uint2[N]
//        3 VALS       uint32[P]       4 BMASK   uint16[P]      the ping-pong side k_raster is (or was) handed
//        5 TILE_START uint32[tiles]   6 TILE_END uint32[tiles]
//        7 INFO       int64[24]: N, P, pair capacity, wide, literal_tris, large_tris, zq_cull, pending, W, H, tiles_x, tiles_y,
//                     strip_y0, strip_y1, strip_ty0, strip_ty1, il_tiles, il_world, il_rank, side, direct (trgl_flush_begin queued the
//                     direct path), fell_back (its kernels did nothing: the flush did not fit, k_expand's chain bins it), seg_S, seg_G (the
//                     segment and group sizes k_chunk_spine was given: the direct path's, or on k_expand's chain those it only checks;
//                     0, 0 without sizes: forced k_expand, WIDE, the rule gives none), 0...
// While a flush is pending whose pairs exceed the capacity (trgl_flush_end will grow the buffers and bin again), the pair lists
// and tile bounds do not exist yet: TRGL_E_STATE for what 3-6; INFO still reports P and the capacity.
extern "C" int trgl_debug_read(trgl_ctx* c, int what, void* dst, size_t bytes, size_t* needed) {
    CHKCTX(c);
    const bool pending = c->rp.active;
    if (!pending && !c->snap.valid) return fail(c, TRGL_E_STATE, "trgl_debug_read: no flush to read (between trgl_flush_begin and trgl_flush_end, or after a flush until the next draw or clear)");
    if (what < 0 || what > 7) return fail(c, TRGL_E_INVALID, "trgl_debug_read: unknown buffer");
    FrameParams fp; uint64_t N, P, cap, lit, lrg; int cur, direct = 0, fell = 0; uint32_t seg_S = 0, seg_G = 0;
    if (pending) {
        fp = c->rp.fp; N = c->rp.N; cap = c->rp.cap; cur = c->rp.cur; P = lit = lrg = 0;
        if (N) {
            if (int r = settle_binning(c, false)) return r;      // (a flush that fell back from the direct path is binned by k_expand's chain first)
            cap = c->rp.cap; cur = c->rp.cur;
            HIPCHK(c, hipEventSynchronize(c->ev_pairs));
            P = c->stats_pinned->pairs_total; lit = c->stats_pinned->literal_tris; lrg = c->stats_pinned->large_tris;
        }
        fp.zq_cull = (N != 0 && lrg != 0) ? 1 : 0;         // what trgl_flush_end will decide
        direct = (N && c->rp.direct) ? 1 : 0; fell = (direct && *c->seg_flag_pinned != 0 && P <= 0xffffe000ull) ? 1 : 0;
        if (N) { seg_S = c->rp.seg.S; seg_G = c->rp.seg.G; }
    } else {
        direct = c->snap.direct; fell = c->snap.fell_back; seg_S = c->snap.seg_S; seg_G = c->snap.seg_G;
        fp = c->snap.fp; N = c->snap.N; P = c->snap.P; cap = c->snap.cap; cur = c->snap.cur; lit = c->snap.literal_tris; lrg = c->snap.large_tris;
    }
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    if (what >= 3 && what <= 6 && P > cap) return fail(c, TRGL_E_STATE, "trgl_debug_read: the pending flush has more pairs than the pair buffers hold; its lists exist after trgl_flush_end");
    int64_t info[24] = { (int64_t)N, (int64_t)P, (int64_t)cap, ntiles > 65536 ? 1 : 0, (int64_t)lit, (int64_t)lrg, fp.zq_cull, pending ? 1 : 0,
                         fp.W, fp.H, fp.tiles_x, fp.tiles_y, fp.strip_y0, fp.strip_y1, fp.strip_ty0, fp.strip_ty1, fp.il_tiles, fp.il_world, fp.il_rank, cur, direct, fell, seg_S, seg_G };
    const void* src = nullptr; size_t need = 0;
    switch (what) {
    case 0: src = c->recs.p; need = N ? (size_t)(N + 1) * sizeof(TriRec) : 0; break;
    case 1: src = c->cnt.p; need = (size_t)N * sizeof(uint32_t); break;
    case 2: src = c->tilebox.p; need = (size_t)N * sizeof(uint2); break;
    case 3: src = c->vals[cur].p; need = (size_t)P * sizeof(uint32_t); break;
    case 4: src = c->bmask[cur].p; need = (size_t)P * sizeof(uint16_t); break;
    case 5: src = c->tile_start.p; need = ntiles * sizeof(uint32_t); break;
    case 6: src = c->tile_end(); need = ntiles * sizeof(uint32_t); break;
    default: need = sizeof(info); break;
    }
    if (needed) *needed = need;
    if (!dst) return TRGL_OK;
    if (bytes < need) return fail(c, TRGL_E_INVALID, "trgl_debug_read: destination too small");
    if (what == 7) { std::memcpy(dst, info, sizeof(info)); return TRGL_OK; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (need) HIPCHK(c, hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    return TRGL_OK;
}

// Test hook beside trgl_debug_read (not part of include/trgl.h): how the NEXT flushes bin.  mode 0: the automatic choice; 1: always
// k_expand's chain; 2: always the direct path, with segments of S slots (a multiple of 4 in 4..4096) and groups of G (1..16) setup
// blocks - a flush that does not fit them falls back; -1: change nothing.  *last_direct / *last_fell_back (may be null): what the last
// complete flush did.
extern "C" int trgl_debug_binning(trgl_ctx* c, int mode, uint32_t S, uint32_t G, int* last_direct, int* last_fell_back) {
    CHKCTX(c);
    if (mode < -1 || mode > 2) return fail(c, TRGL_E_INVALID, "trgl_debug_binning: mode is -1 (report only), 0 (automatic), 1 (k_expand) or 2 (direct)");
    if (mode == 2 && !seg_layout_ok(SegLayout{ nullptr, nullptr, nullptr, nullptr, 0, S, G }))
        return fail(c, TRGL_E_INVALID, "trgl_debug_binning: S is a multiple of 4 in 4..4096, G in 1..16");
    if (mode >= 0) { c->bin_mode = mode; c->bin_S = mode == 2 ? S : 0; c->bin_G = mode == 2 ? G : 0; c->seg_hold = false; }
    if (last_direct) *last_direct = c->last_direct;
    if (last_fell_back) *last_fell_back = c->last_fell_back;
    return TRGL_OK;
}

}  // extern "C"

// ---- RCCL, loaded on demand (the library has no link-time dependency on it) --------------------------------------------
namespace {
struct Rccl {
    struct Id { char b[128]; };          // ncclUniqueId, passed by value (rccl.h)
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r;
    if (!r.lib) {
        r.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!r.lib) r.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (r.lib) {
            r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
            r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
            r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
            r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
            r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.lib, "ncclGroupStart"));
            r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.lib, "ncclGroupEnd"));
            r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
            r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.GroupStart && r.GroupEnd;
        }
    }
    return r;
}
std::string rccl_err(const char* what, int code) {
    Rccl& r = rccl();
    return std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(code) : "RCCL error") + " (" + std::to_string(code) + ")";
}
constexpr int NCCL_UINT8 = 1;       // ncclUint8 (rccl.h, ncclDataType_t)
}  // namespace

extern "C" {

int trgl_rccl_unique_id(uint8_t id[TRGL_RCCL_ID_BYTES]) {
    if (!id) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) { g_create_error = "librccl.so.1 could not be loaded"; return TRGL_E_UNSUPPORTED; }
    const int rc = r.GetUniqueId(id);
    if (rc) { g_create_error = rccl_err("ncclGetUniqueId", rc); return TRGL_E_HIP; }
    return TRGL_OK;
}
int trgl_rccl_comm_create(const uint8_t id[TRGL_RCCL_ID_BYTES], int rank, int world, int device, void** comm) {
    if (!id || !comm || world < 1 || rank < 0 || rank >= world) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) { g_create_error = "librccl.so.1 could not be loaded"; return TRGL_E_UNSUPPORTED; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return TRGL_E_HIP; }
    Rccl::Id uid; std::memcpy(uid.b, id, 128);
    const int rc = r.CommInitRank(comm, world, uid, rank);
    if (rc) { g_create_error = rccl_err("ncclCommInitRank", rc); return TRGL_E_HIP; }
    return TRGL_OK;
}
int trgl_rccl_comm_destroy(void* comm) {
    if (!comm) return TRGL_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return TRGL_E_UNSUPPORTED;
    return r.CommDestroy(comm) ? TRGL_E_HIP : TRGL_OK;
}

int trgl_gather(trgl_ctx* c, void* comm, int rank, int world, int with_z) {
    CHKCTX(c);
    if (!comm || world < 1 || rank < 0 || rank >= world) return fail(c, TRGL_E_INVALID, "trgl_gather: bad communicator / rank / world");
    Rccl& r = rccl();
    if (!r.ok) return fail(c, TRGL_E_UNSUPPORTED, "trgl_gather: librccl.so.1 could not be loaded");
    int fr = trgl_flush(c); if (fr) return fr;               // the rows this context owns are complete behind this point of the stream
    const size_t row_fb = (size_t)c->W * c->bpp, row_z = (size_t)c->W * sizeof(double);
    int rc = 0;
    if (c->il_tiles == 0) {
        // one strip per rank: equal, contiguous chunks of the row-major buffers
        if (c->H % world) return fail(c, TRGL_E_INVALID, "trgl_gather: the height is not divisible by the number of ranks (equal strips are required)");
        const int rows = c->H / world;
        if (c->strip_y0 != rank * rows || c->strip_y1 != (rank + 1) * rows)
            return fail(c, TRGL_E_STATE, "trgl_gather: this context's strip is not rows [rank * H / world, (rank + 1) * H / world)");
        if ((rc = r.GroupStart())) { c->err = rccl_err("ncclGroupStart", rc); return TRGL_E_HIP; }
        rc = r.AllGather(c->fb.p + (size_t)c->strip_y0 * row_fb, c->fb.p, (size_t)rows * row_fb, NCCL_UINT8, comm, c->stream);
        if (!rc && with_z) rc = r.AllGather(reinterpret_cast<uint8_t*>(c->zb.p) + (size_t)c->strip_y0 * row_z, c->zb.p, (size_t)rows * row_z, NCCL_UINT8, comm, c->stream);
        const int rc2 = r.GroupEnd();
        if (!rc) rc = rc2;
    } else {
        // interleaved bands: inside each period of world * band_rows rows the bands lie in rank order
        if (c->il_world != world || c->il_rank != rank) return fail(c, TRGL_E_STATE, "trgl_gather: rank / world differ from trgl_set_interleave");
        const int band = c->il_tiles * TRGL_TILE, period = band * world;
        if (c->H % period) return fail(c, TRGL_E_INVALID, "trgl_gather: the height is not a multiple of world * band_rows");
        if ((rc = r.GroupStart())) { c->err = rccl_err("ncclGroupStart", rc); return TRGL_E_HIP; }
        for (int p0 = 0; p0 < c->H && !rc; p0 += period) {
            const int y0 = p0 + rank * band;
            rc = r.AllGather(c->fb.p + (size_t)y0 * row_fb, c->fb.p + (size_t)p0 * row_fb, (size_t)band * row_fb, NCCL_UINT8, comm, c->stream);
            if (!rc && with_z) rc = r.AllGather(reinterpret_cast<uint8_t*>(c->zb.p) + (size_t)y0 * row_z, reinterpret_cast<uint8_t*>(c->zb.p) + (size_t)p0 * row_z,
                                                (size_t)band * row_z, NCCL_UINT8, comm, c->stream);
        }
        const int rc2 = r.GroupEnd();
        if (!rc) rc = rc2;
    }
    if (rc) { c->err = rccl_err("ncclAllGather", rc); return TRGL_E_HIP; }
    return TRGL_OK;
}

int trgl_get_last_flush_info(trgl_ctx* c, uint64_t* triangles, uint64_t* pairs, uint64_t* tiles) {
    if (!c) return TRGL_E_INVALID;
    if (triangles) *triangles = c->last_tris;
    if (pairs) *pairs = c->last_pairs;
    if (tiles) *tiles = (uint64_t)c->tiles_x * c->tiles_y;
    return TRGL_OK;
}

}  // extern "C"
