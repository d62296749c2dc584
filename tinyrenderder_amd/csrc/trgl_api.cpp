// trgl_api.cpp — host side of the C ABI in include/trgl.h: context, HBM buffers, the flush pipeline.
//
// A flush runs, on the context's own HIP stream:
//   setup (per draw) -> scan(counts) -> expand -> stable radix passes by tile id -> bounds -> raster
// and is the batched equivalent of the reference's per-face loop of rasterize() calls
// (main.cpp:660-666): submission order is preserved per tile, so results are identical.
// Passes, shader registration, the stages in front of a draw, host-only functions and RCCL: trgl_passes.cpp, trgl_shader.cpp,
// trgl_stage_*.cpp, trgl_host.cpp, trgl_rccl.cpp (trgl_ctx.h).
#include <algorithm>
#include <cstring>

#include "trgl_ctx.h"
#include "user_shaders.h"

// the growth rule of the pair buffers: headroom() as a multiple of 4 entries (k_radix_hist reads 16 bytes at a time, k_raster 4 entries), at most 0xffffe000 (grids are sized by
// cap + 4095 in 32 bits; a flush of 2^32 - 16 pairs and more is refused)
static size_t pair_capacity(size_t need) {
    const size_t ncap = (headroom(need) + 3) & ~size_t(3);
    return ncap > 0xffffe000ull ? 0xffffe000ull : ncap;
}

int trgl::fail(trgl_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; else set_global_error(msg); return code; }

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
int trgl::end_pending_raster(trgl_ctx* c) { return c->rp.active ? trgl_flush_end(c) : TRGL_OK; }
// ... and submit the queued draws, which were made under the old state
static int flush_queued(trgl_ctx* c) { return c->draws.empty() ? TRGL_OK : trgl_flush(c); }
// everything queued, done
int trgl::flush_sync(trgl_ctx* c) {
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
int trgl::stage_alloc(trgl_ctx* c, size_t bytes, void** dev) {
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
int trgl::stage_copy(trgl_ctx* c, const void* src, size_t bytes, void** dev) {
    int r = stage_alloc(c, bytes, dev); if (r) return r;
    HIPCHK(c, hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice));   // "copied before trgl_draw returns"
    return TRGL_OK;
}

// a registered user kind that may discard (its draws are rasterized by its own kernel, in flushes of their own)
static bool discarding_kind(const trgl_ctx* c, int kind) {
    const UserKind* uk = user_kind(c, kind);
    return uk && (uk->flags & TRGL_SHADER_MAY_DISCARD);
}

int trgl::kind_vary_count(const trgl_ctx* c, int kind) {
    const UserKind* uk = user_kind(c, kind);
    return uk ? uk->K : (kind >= 0 && kind < TRGL_NUM_SHADERS) ? vary_count(kind) : -1;
}

int trgl::check_kind_uniforms(trgl_ctx* c, const char* who, int kind, const trgl_uniforms* u) {
    if ((kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE) && !u) return fail(c, TRGL_E_INVALID, std::string(who) + ": PHONG/EYE need uniforms");
    if (kind == TRGL_SHADER_CHECKER && (!u || u->reserved < 1)) return fail(c, TRGL_E_INVALID, std::string(who) + ": CHECKER needs uniforms with reserved = cells >= 1");
    return TRGL_OK;
}

extern "C" {

const char* trgl_last_error(const trgl_ctx* ctx) { return ctx ? ctx->err.c_str() : global_error(); }

int trgl_create(int device, int width, int height, int bpp, trgl_ctx** out) {
    if (!out || width <= 0 || height <= 0 || width > 65535 || height > 65535 || !(bpp == 1 || bpp == 3 || bpp == 4))
        return fail(nullptr, TRGL_E_INVALID, "trgl_create: bad arguments (width/height in 1..65535, bpp in {1,3,4})");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, TRGL_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    trgl_ctx* c = new trgl_ctx();
    c->device = device; c->W = width; c->H = height; c->bpp = bpp;
    c->tiles_x = (width + TRGL_TILE - 1) / TRGL_TILE;
    c->tiles_y = (height + TRGL_TILE - 1) / TRGL_TILE;
    c->strip_y0 = 0; c->strip_y1 = height;
    std::memset(c->tex_host, 0, sizeof(c->tex_host));
    if (int r = init_ctx(c)) { fail(nullptr, r, c->err); trgl_destroy(c); return r; }
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
    c->tex_cap[slot] = 0;
    if (texels && w > 0 && h > 0) {
        if (!(bpp == 1 || bpp == 3 || bpp == 4)) return fail(c, TRGL_E_INVALID, "trgl_upload_texture: bpp must be 1, 3 or 4");
        uint8_t* d = nullptr; size_t bytes = (size_t)w * h * bpp;
        HIPCHK(c, hipMalloc((void**)&d, bytes + 8));         // +8: the samplers read each texel as one 4-byte load
        HIPCHK(c, hipMemset(d + bytes, 0, 8));
        HIPCHK(c, hipMemcpy(d, texels, bytes, hipMemcpyHostToDevice));
        c->tex_host[slot] = DevTexture{ d, w, h, bpp, 0 };      // one level until trgl_texture_mipmaps
        c->tex_cap[slot] = bytes + 8;
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

int trgl_draw(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* clip, const double* vary,
              const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const int K = kind_vary_count(c, kind);
    if (K < 0) return fail(c, TRGL_E_INVALID, "trgl_draw: unknown shader kind");
    if (n == 0) return TRGL_OK;
    c->snap.valid = false;
    if (!clip) return fail(c, TRGL_E_INVALID, "trgl_draw: clip is null");
    if (K && !vary) return fail(c, TRGL_E_INVALID, "trgl_draw: this shader kind needs varyings");
    if ((r = check_kind_uniforms(c, "trgl_draw", kind, u))) return r;
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_draw: bad mem_kind");
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
        const uint32_t grid = launch_radix_pass(s, rp, wide, ps == passes - 1, pairs_dev, cap, c->hist.p, c->scan_tmp.p, ps == 0 ? seg : nullptr,
                                                (seg && ps > 0) ? seg->flag : nullptr, c->radix_max_blocks);
        if (ps == 0) c->radix_used[0] = grid;
        if (ps == passes - 1) c->radix_used[1] = grid;
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
    if ((r = c->item_stats.grow(c, ((size_t)max_items + 64) * TRGL_ITEM_STATS_WORDS))) return r;
    // k_setup counted the triangles that are not well scaled (it came over with the pair count): without any, the kernel without the literal path
    const bool all_well_scaled = N == 0 || c->stats_pinned->literal_tris == 0;
    fp.zq_cull = (N != 0 && c->stats_pinned->large_tris != 0) ? 1 : 0;      // (k_setup counted them; the count came over with the pair count)
    UserShade user[TRGL_MAX_USER_SHADERS];
    int n_user = 0;
    for (int i = 0; i < (int)c->user.size(); ++i)
        if (c->rp.user_kinds >> i & 1u) user[n_user++] = UserShade{ c->user[i].fn, TRGL_SHADER_USER_FIRST + i };
    // a flush of a kind that may discard: its own raster kernel in place of k_raster
    const hipFunction_t user_raster = discarding_kind(c, flush_kind) ? user_kind(c, flush_kind)->fn : nullptr;
    launch_raster(s, fp, flush_kind, all_well_scaled, recs_arg, c->recs_w.p, vals_arg, bmask_arg, c->tile_start.p, c->tile_end(), c->draws_dev.p, c->tex_dev.p,
                  c->stats_dev.p, max_items, c->items.p, c->n_items.p, c->item_stats.p, c->rp.builtin_shade, user, n_user, user_raster,
                  c->profiling ? c->ev[4] : nullptr, c->profiling ? c->ev[5] : nullptr);
    if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[3], s)); c->events_pending = true; }
    HIPCHK(c, hipGetLastError());

    c->triangles_total += N;
    if (N) { c->rule_pairs = P; c->rule_nblk = c->rp.nblk; }       // (a flush that only clears has no pairs per block: the rule keeps its input)
    // the record of this flush (a flush without triangles has direct, fell_back, seg.S and seg.G at 0 from trgl_flush_begin)
    c->snap = Snapshot{ true, c->rp, P, N ? c->stats_pinned->literal_tris : 0, N ? c->stats_pinned->large_tris : 0 };
    c->snap.rp.fp = fp; c->snap.rp.cap = (uint32_t)c->keys[0].cap;
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

void* trgl_framebuffer_device_ptr(trgl_ctx* c) { return c ? c->fb.p : nullptr; }
void* trgl_zbuffer_device_ptr(trgl_ctx* c) { return c ? c->zb.p : nullptr; }
void* trgl_stream(trgl_ctx* c) { return c ? (void*)c->stream : nullptr; }

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
    Snapshot f = c->snap;
    if (pending) {                                         // the record trgl_flush_end would take, as far as it is known
        if (int r = settle_binning(c, false)) return r;    // (a flush that fell back from the direct path is binned by k_expand's chain first)
        f = Snapshot{ true, c->rp, 0, 0, 0 };
        if (f.rp.N) {
            HIPCHK(c, hipEventSynchronize(c->ev_pairs));
            f.P = c->stats_pinned->pairs_total; f.literal_tris = c->stats_pinned->literal_tris; f.large_tris = c->stats_pinned->large_tris;
            f.rp.fell_back = f.rp.direct && *c->seg_flag_pinned != 0 && f.P <= 0xffffe000ull;      // (also where the binning is not settled)
        }
        f.rp.fp.zq_cull = f.large_tris != 0 ? 1 : 0;       // what trgl_flush_end will decide
    }
    const FrameParams& fp = f.rp.fp; const uint64_t N = f.rp.N, P = f.P, cap = f.rp.cap; const int cur = f.rp.cur;
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    if (what >= 3 && what <= 6 && P > cap) return fail(c, TRGL_E_STATE, "trgl_debug_read: the pending flush has more pairs than the pair buffers hold; its lists exist after trgl_flush_end");
    int64_t info[24] = { (int64_t)N, (int64_t)P, (int64_t)cap, ntiles > 65536 ? 1 : 0, (int64_t)f.literal_tris, (int64_t)f.large_tris, fp.zq_cull, pending ? 1 : 0,
                         fp.W, fp.H, fp.tiles_x, fp.tiles_y, fp.strip_y0, fp.strip_y1, fp.strip_ty0, fp.strip_ty1, fp.il_tiles, fp.il_world, fp.il_rank, cur, f.rp.direct, f.rp.fell_back, f.rp.seg.S, f.rp.seg.G };
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
    if (last_direct) *last_direct = c->snap.rp.direct;
    if (last_fell_back) *last_fell_back = c->snap.rp.fell_back;
    return TRGL_OK;
}

// Test hook beside trgl_debug_binning (not part of include/trgl.h): the radix scatters of the NEXT flushes run at most max_blocks blocks
// (0: as many as the device holds at once, the default); every block walks its chunks with a stride of the grid, so a small grid makes
// every block loop.  *used_first / *used_last (may be null): the grids of the first and the last pass of the last binning queued.
extern "C" int trgl_debug_radix_blocks(trgl_ctx* c, uint32_t max_blocks, uint32_t* used_first, uint32_t* used_last) {
    CHKCTX(c);
    c->radix_max_blocks = max_blocks;
    if (used_first) *used_first = c->radix_used[0];
    if (used_last) *used_last = c->radix_used[1];
    return TRGL_OK;
}

int trgl_get_last_flush_info(trgl_ctx* c, uint64_t* triangles, uint64_t* pairs, uint64_t* tiles) {
    if (!c) return TRGL_E_INVALID;
    if (triangles) *triangles = c->snap.rp.N;
    if (pairs) *pairs = c->snap.P;
    if (tiles) *tiles = (uint64_t)c->tiles_x * c->tiles_y;
    return TRGL_OK;
}

}  // extern "C"
