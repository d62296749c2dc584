// trgl_stage_rows.cpp — the stages over triangle rows and over points: the depth-ordered triangle draw (trgl_triangle_depths,
// trgl_order_stage, trgl_draw_ordered) and point sprites and wide lines (trgl_sprite_stage, trgl_draw_sprites, trgl_line_stage,
// trgl_draw_lines).  The draws go through trgl_draw (trgl_api.cpp), which owns the queue and its ordering rules.
#include <cstring>

#include "trgl_stage.h"

// ---- depth-ordered triangle draws (include/trgl.h: trgl_triangle_depths, trgl_order_stage, trgl_draw_ordered) ----
// what the three calls check of n and group alike
static int check_groups(trgl_ctx* c, const std::string& w, uint64_t n, uint32_t group) {
    if (group == 0) return fail(c, TRGL_E_INVALID, w + "group is 0");
    if (n % group) return fail(c, TRGL_E_INVALID, w + "n is not a multiple of group");
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    return TRGL_OK;
}

// ... and of the list: n_order * group rows fit, and with host_list every entry names a group
static int check_order_list(trgl_ctx* c, const std::string& w, const uint32_t* order, uint64_t n_order, uint32_t group, uint64_t G, bool host_list) {
    if (n_order > 0x7fffffffull / group) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in the ordered list");
    if (host_list && !all_below(order, n_order, G)) return fail(c, TRGL_E_INVALID, w + "an entry of the order list is not a group");
    return TRGL_OK;
}

// The gather over device arrays, queued on the context's stream: one launch per array (vary null: K = 0; colors null: none)
static int queue_order_stage(trgl_ctx* c, int K, const double* clip, const double* vary, const uint32_t* colors, uint64_t G, const uint32_t* order,
                             uint64_t n_order, uint32_t g, const Rows& out) {
    launch_gather_rows(c->stream, clip, out.clip, 12 * sizeof(double), order, (uint32_t)n_order, (uint32_t)G, g);
    if (K) launch_gather_rows(c->stream, vary, out.vary, (uint32_t)K * sizeof(double), order, (uint32_t)n_order, (uint32_t)G, g);
    if (colors) launch_gather_rows(c->stream, colors, out.colors, sizeof(uint32_t), order, (uint32_t)n_order, (uint32_t)G, g);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// ---- point sprites and wide lines (include/trgl.h: trgl_sprite_stage, trgl_draw_sprites, trgl_line_stage, trgl_draw_lines) ----
// The inputs of either stage: n primitives over n_points rows of `stride` doubles (sprites: n_points == n, no indices)
struct QuadInputs { const double* points; int stride; uint64_t n_points; const uint32_t* indices; const uint32_t* colors; uint64_t n; int mem_kind; };

// what the scalars of a sprite call must satisfy; *K = 6 + n_attr
static int check_sprite_params(trgl_ctx* c, const std::string& w, const trgl_sprite_params* P, int stride, int mem_kind, uint64_t n, int* K) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (P->mode != TRGL_SPRITE_VIEW && P->mode != TRGL_SPRITE_SCREEN) return fail(c, TRGL_E_INVALID, w + "bad mode");
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (stride < 3) return fail(c, TRGL_E_INVALID, w + "point stride must be >= 3 doubles");
    if (P->size_offset >= stride) return fail(c, TRGL_E_INVALID, w + "size_offset is outside the point's row");
    if (P->n_attr < 0 || (P->n_attr && (P->attr_offset < 0 || (int64_t)P->attr_offset + P->n_attr > stride)))
        return fail(c, TRGL_E_INVALID, w + "the attribute range is outside the point's row");
    if (6 + (int64_t)P->n_attr > TRGL_MAX_USER_VARY) return fail(c, TRGL_E_INVALID, w + "6 + n_attr is above TRGL_MAX_USER_VARY");
    if (n > 0x3fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    *K = 6 + P->n_attr;
    return TRGL_OK;
}

static int check_line_params(trgl_ctx* c, const std::string& w, const trgl_line_params* P, const QuadInputs& in) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (int r = check_mem(c, w, in.mem_kind)) return r;
    if (in.stride < 3) return fail(c, TRGL_E_INVALID, w + "point stride must be >= 3 doubles");
    if (!(P->w_min > 0.0) || !(P->w_min - P->w_min == 0.0)) return fail(c, TRGL_E_INVALID, w + "w_min must be positive and finite");
    if (in.n > 0x3fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    if (!in.indices && 2 * in.n > in.n_points) return fail(c, TRGL_E_INVALID, w + "without indices 2 * n_segments points are needed");
    return TRGL_OK;
}

// ... and its arrays (n > 0): present, aligned, outputs apart from inputs; with host memory every index of a line list in range.
// K: the varyings per row when out.vary is given.
static int check_quad_arrays(trgl_ctx* c, const std::string& w, const QuadInputs& in, int K, const Rows& out) {
    if (!in.points || !out.clip || (in.colors && !out.colors)) return fail(c, TRGL_E_INVALID, w + "null array");
    const uint32_t* colors_out = in.colors ? out.colors : nullptr;
    if (!aligned({ { in.points, 8 }, { out.clip, 8 }, { out.vary, 8 }, { in.colors, 4 }, { in.indices, 4 }, { colors_out, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for colours and indices)");
    struct Range { const void* p; uint64_t bytes; };
    const Range ins[3] = { { in.points, in.n_points * (uint64_t)in.stride * 8 }, { in.colors, in.n * 4 }, { in.indices, in.n * 8 } };
    const Range outs[3] = { { out.clip, in.n * 192 }, { out.vary, in.n * 16 * (uint64_t)K }, { colors_out, in.n * 8 } };
    for (const Range& i : ins)
        for (const Range& o : outs)
            if (arrays_overlap(i.p, i.bytes, o.p, o.bytes)) return fail(c, TRGL_E_INVALID, w + "an output overlaps an input");
    for (int x = 0; x < 3; ++x)
        for (int y = x + 1; y < 3; ++y)
            if (arrays_overlap(outs[x].p, outs[x].bytes, outs[y].p, outs[y].bytes)) return fail(c, TRGL_E_INVALID, w + "two outputs overlap");
    if (in.mem_kind == TRGL_MEM_HOST && in.indices && !all_below(in.indices, 2 * in.n, in.n_points))
        return fail(c, TRGL_E_INVALID, w + "index out of range");
    return TRGL_OK;
}

// What trgl_sprite_stage (lines null) and trgl_line_stage share once their scalars are checked
static int quad_stage_call(trgl_ctx* c, const std::string& w, const trgl_sprite_params* sprites, const trgl_line_params* lines, const QuadInputs& in,
                           int K, const Rows& out) {
    if (in.n == 0) return TRGL_OK;
    if (sprites && sprites->n_attr && !out.vary) return fail(c, TRGL_E_INVALID, w + "vary_out is null and n_attr is not 0");
    int r = check_quad_arrays(c, w, in, K, out); if (r) return r;
    if (in.mem_kind == TRGL_MEM_HOST) {
        if (sprites) host_sprite_stage(*sprites, in.points, in.stride, in.colors, in.n, out.clip, out.vary, out.colors);
        else host_line_stage(*lines, in.points, in.stride, in.indices, in.colors, in.n, out.clip, out.vary, out.colors);
        return TRGL_OK;
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    if (sprites) {
        SpriteArgs a; std::memset(&a, 0, sizeof(a));
        a.P = *sprites; a.points = in.points; a.colors = in.colors;
        a.clip_out = out.clip; a.vary_out = out.vary; a.colors_out = in.colors ? out.colors : nullptr;
        a.n = in.n; a.stride = in.stride;
        launch_sprite_stage(c->stream, a);
    } else {
        LineArgs a; std::memset(&a, 0, sizeof(a));
        a.P = *lines; a.points = in.points; a.indices = in.indices; a.colors = in.colors;
        a.clip_out = out.clip; a.vary_out = out.vary; a.colors_out = in.colors ? out.colors : nullptr;
        a.n_points = in.n_points; a.n = in.n; a.stride = in.stride;
        launch_line_stage(c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// ... and trgl_draw_sprites / trgl_draw_lines: the scalars are checked, K is the stage's
static int quad_draw_call(trgl_ctx* c, const std::string& w, int kind, const trgl_uniforms* u, const trgl_sprite_params* sprites,
                          const trgl_line_params* lines, const QuadInputs& in, int K) {
    // (what trgl_draw would refuse is refused before anything is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (kind_K != K && !(kind_K == 0 && K == 6)) return fail(c, TRGL_E_INVALID, w + "the shader kind's number of varyings does not fit the stage's");
    int r;
    if ((r = check_kind_uniforms(c, w, kind, u))) return r;
    if (in.n == 0) return TRGL_OK;
    const uint64_t rows = 2 * in.n;
    if (in.mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        const HostRows host(rows, kind_K, in.colors != nullptr); const Rows& o = host.o;
        if (int e = quad_stage_call(c, w, sprites, lines, in, K, o)) return e;
        return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, rows, TRGL_MEM_HOST);
    });
    if (!in.points) return fail(c, TRGL_E_INVALID, w + "null array");
    StageHold hold(c);
    CallMem mem(c, true); Rows o;
    if ((r = alloc_rows(mem, rows, kind_K, in.colors != nullptr, &o)) || (r = quad_stage_call(c, w, sprites, lines, in, K, o))) return r;
    return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, rows, TRGL_MEM_DEVICE);
}

extern "C" {

int trgl_sprite_stage(trgl_ctx* c, const trgl_sprite_params* P, const double* points, int stride, const uint32_t* colors, uint64_t n, int mem_kind,
                      double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_sprite_stage: ";
    int K = 0;
    if (int r = check_sprite_params(c, w, P, stride, mem_kind, n, &K)) return r;
    const QuadInputs in{ points, stride, n, nullptr, colors, n, mem_kind };
    return quad_stage_call(c, w, P, nullptr, in, K, Rows{ clip_out, vary_out, colors_out });
}

int trgl_draw_sprites(trgl_ctx* c, int kind, const trgl_uniforms* u, const trgl_sprite_params* P, const double* points, int stride,
                      const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_sprites: ";
    int K = 0;
    if ((r = check_sprite_params(c, w, P, stride, mem_kind, n, &K))) return r;
    const QuadInputs in{ points, stride, n, nullptr, colors, n, mem_kind };
    return quad_draw_call(c, w, kind, u, P, nullptr, in, K);
}

int trgl_line_stage(trgl_ctx* c, const trgl_line_params* P, const double* points, int stride, uint64_t n_points, const uint32_t* indices,
                    const uint32_t* colors, uint64_t n_segments, int mem_kind, double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_line_stage: ";
    const QuadInputs in{ points, stride, n_points, indices, colors, n_segments, mem_kind };
    if (int r = check_line_params(c, w, P, in)) return r;
    return quad_stage_call(c, w, nullptr, P, in, 6, Rows{ clip_out, vary_out, colors_out });
}

int trgl_draw_lines(trgl_ctx* c, int kind, const trgl_uniforms* u, const trgl_line_params* P, const double* points, int stride, uint64_t n_points,
                    const uint32_t* indices, const uint32_t* colors, uint64_t n_segments, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_lines: ";
    const QuadInputs in{ points, stride, n_points, indices, colors, n_segments, mem_kind };
    if ((r = check_line_params(c, w, P, in))) return r;
    return quad_draw_call(c, w, kind, u, nullptr, P, in, 6);
}

int trgl_triangle_depths(trgl_ctx* c, const double* clip, uint64_t n, uint32_t group, int mode, int mem_kind, double* depths_out) {
    const std::string w = "trgl_triangle_depths: ";
    if (mode != TRGL_TRI_DEPTH_CENTROID && mode != TRGL_TRI_DEPTH_NEAREST && mode != TRGL_TRI_DEPTH_FARTHEST) return fail(c, TRGL_E_INVALID, w + "bad mode");
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if ((r = check_groups(c, w, n, group))) return r;
    if (n == 0) return TRGL_OK;
    if (!clip || !depths_out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (mem_kind == TRGL_MEM_HOST) { host_triangle_depths(clip, n / group, group, mode, depths_out); return TRGL_OK; }
    CHKCTX(c);
    if (!aligned({ { clip, 8 }, { depths_out, 8 } })) return fail(c, TRGL_E_INVALID, w + "device arrays must be 8-byte aligned");
    launch_triangle_depths(c->stream, clip, (uint32_t)(n / group), group, mode, depths_out);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_order_stage(trgl_ctx* c, int K, const double* clip, const double* vary, const uint32_t* colors, uint64_t n,
                     const uint32_t* order, uint64_t n_order, uint32_t group, int mem_kind,
                     double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_order_stage: ";
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (K < 0 || K > TRGL_MAX_USER_VARY) return fail(c, TRGL_E_INVALID, w + "K outside 0..TRGL_MAX_USER_VARY");
    if ((r = check_groups(c, w, n, group))) return r;
    if (!order && n_order) return fail(c, TRGL_E_INVALID, w + "order is null");
    if ((r = check_order_list(c, w, order, n_order, group, n / group, false))) return r;
    if (n_order == 0) return TRGL_OK;
    if (!clip_out || (K && !vary_out) || (colors && !colors_out)) return fail(c, TRGL_E_INVALID, w + "null output");
    if (n && (!clip || (K && !vary))) return fail(c, TRGL_E_INVALID, w + "null array");
    if (mem_kind == TRGL_MEM_HOST) {
        if ((r = check_order_list(c, w, order, n_order, group, n / group, true))) return r;
        host_order_stage(K, clip, vary, colors, order, n_order, group, clip_out, vary_out, colors_out);
        return TRGL_OK;
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    if (!aligned({ { clip, 8 }, { K ? vary : nullptr, 8 }, { colors, 4 }, { order, 4 }, { clip_out, 8 }, { K ? vary_out : nullptr, 8 },
                   { colors ? colors_out : nullptr, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for doubles, 4 for colours and the list)");
    return queue_order_stage(c, K, clip, K ? vary : nullptr, colors, n / group, order, n_order, group, Rows{ clip_out, vary_out, colors_out });
}

int trgl_draw_ordered(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* clip, const double* vary, const uint32_t* colors, uint64_t n,
                      int mem_kind, const uint32_t* order, uint64_t n_order, uint32_t group, int order_mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_ordered: ";
    if ((r = check_mem(c, w, order_mem_kind, "order_mem_kind"))) return r;
    if ((order == nullptr) != (n_order == 0)) return fail(c, TRGL_E_INVALID, w + "order must be null exactly when n_order is 0");
    if (!order) return trgl_draw(c, kind, u, clip, vary, colors, n, mem_kind);
    // (what trgl_draw would refuse is refused before anything is queued)
    const int K = kind_vary_count(c, kind);
    if (K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if ((r = check_mem(c, w, mem_kind)) || (r = check_groups(c, w, n, group))) return r;
    if (n && !clip) return fail(c, TRGL_E_INVALID, w + "clip is null");
    if (n && K && !vary) return fail(c, TRGL_E_INVALID, w + "this shader kind needs varyings");
    if ((r = check_kind_uniforms(c, w, kind, u))) return r;
    const uint64_t G = n / group, rows = n_order * group;
    const bool host_rows = mem_kind == TRGL_MEM_HOST, host_list = order_mem_kind == TRGL_MEM_HOST;
    if ((r = check_order_list(c, w, order, n_order, group, G, host_list))) return r;
    if (!K) vary = nullptr;
    if (host_rows && host_list) return no_bad_alloc(c, w, [&] {
        const HostRows host(rows, K, colors != nullptr); const Rows& o = host.o;
        host_order_stage(K, clip, vary, colors, order, n_order, group, o.clip, o.vary, o.colors);
        return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, rows, TRGL_MEM_HOST);
    });
    if ((!host_rows && !aligned({ { clip, 8 }, { vary, 8 }, { colors, 4 } })) || (!host_list && !aligned({ { order, 4 } })))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for doubles, 4 for colours and the list)");
    StageHold hold(c);
    CallMem mem(c, true); Rows o;
    if (host_rows && n) {
        if ((r = mem.copy(clip, n * 12, &clip)) || (K && (r = mem.copy(vary, n * (size_t)K, &vary))) || (colors && (r = mem.copy(colors, n, &colors)))) return r;
    }
    if (host_list && (r = mem.copy(order, n_order, &order))) return r;
    if ((r = alloc_rows(mem, rows, K, colors != nullptr, &o))) return r;
    if ((r = queue_order_stage(c, K, clip, vary, colors, G, order, n_order, group, o))) return r;
    return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, rows, TRGL_MEM_DEVICE);
}

}  // extern "C"
