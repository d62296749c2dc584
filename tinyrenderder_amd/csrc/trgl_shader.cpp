// trgl_shader.cpp — run-time shader registration (fragment kinds and vertex shaders, compiled by user_shaders.cpp) and the entry points
// that run a stage in front of a draw: the vertex stage over an indexed mesh (trgl_draw_indexed, trgl_draw_indexed_vs, trgl_vertex_stage)
// the clip stage (trgl_clip_stage, trgl_draw_clipped, trgl_draw_indexed_vs_clipped) and the instanced stages (trgl_draw_instanced,
// trgl_instance_stage, their ordered forms, and the depths and order those take: trgl_instance_depths, trgl_depth_order) the ordered triangle draw (trgl_triangle_depths, trgl_order_stage, trgl_draw_ordered) the sprite and line stages (trgl_sprite_stage, trgl_draw_sprites, trgl_line_stage, trgl_draw_lines) and skeletal animation (trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned).  The draws they make go through trgl_draw (trgl_api.cpp), which owns the queue and its ordering rules.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "trgl_ctx.h"
#include "user_shaders.h"
#include "skin_core.h"

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
    const std::string w = std::string(who) + ": ";
    if (!((builtin_ok && vs == -1) || (vs >= 0 && vs < (int)c->vertex.size()))) return fail(c, TRGL_E_INVALID, w + "unknown vertex shader");
    *K = vs < 0 ? TRGL_VARY_PHONG : c->vertex[vs].K;
    if (!projection || !vertices || !indices) return fail(c, TRGL_E_INVALID, w + "null argument");
    if (vs < 0 && !u) return fail(c, TRGL_E_INVALID, w + "the built-in vertex stage needs uniforms (model_view)");
    if (stride < (vs < 0 ? 8 : 1)) return fail(c, TRGL_E_INVALID, w + (vs < 0 ? "vertex stride must be >= 8 doubles (pos3, normal3, uv2)" : "vertex stride must be >= 1"));
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (n_faces > 0xffffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "too many faces in one call");
    if (mem_kind == TRGL_MEM_HOST)
        for (uint64_t k = 0; k < 3 * n_faces; ++k)
            if (indices[k] >= n_vertices) return fail(c, TRGL_E_INVALID, w + "index out of range");
    return TRGL_OK;
}

// A plane and an attribute list as the clipped draws take them; null plane: no clipping
struct ClipSpec { const double* plane; const trgl_clip_attr* attrs; int n_attrs; };

// the table of `spec` for a draw of `kind` with K varyings; n_attrs = -1: the kind's built-in layout
static int clip_spec_table(trgl_ctx* c, const char* who, const ClipSpec& spec, int kind, int K, ClipTable* tab) {
    const std::string w = std::string(who) + ": ";
    if (!spec.plane) return fail(c, TRGL_E_INVALID, w + "plane is null");
    trgl_clip_attr builtin[TRGL_MAX_CLIP_ATTRS];
    const trgl_clip_attr* attrs = spec.attrs; int n_attrs = spec.n_attrs;
    if (n_attrs == -1) {
        attrs = builtin; n_attrs = 0;
        if (kind >= 0 && kind < TRGL_NUM_SHADERS) (void)trgl_clip_layout(kind, builtin, &n_attrs);
        else if (K > 0) return fail(c, TRGL_E_INVALID, w + "a user kind with varyings has no built-in clip layout: pass its attributes");
    }
    if (!clip_table(attrs, n_attrs, K, tab)) return fail(c, TRGL_E_INVALID, w + "invalid clip attribute list");
    return TRGL_OK;
}

// The clip stage over device arrays, queued on the context's stream; *n_out is complete when the stream has been waited for.
static int queue_clip_stage(trgl_ctx* c, const double plane[4], const ClipTable& tab, int K, const double* clip, const double* vary,
                            const uint32_t* colors, uint64_t n, double* clip_out, double* vary_out, uint32_t* colors_out, unsigned long long* n_out) {
    int r;
    if ((r = c->clip_scratch.grow(c, 2 + clip_scratch_words(n)))) return r;
    ClipArgs a; std::memset(&a, 0, sizeof(a));
    std::memcpy(a.plane, plane, sizeof(a.plane));
    a.clip = clip; a.vary = K ? vary : nullptr; a.colors = colors;
    a.clip_out = clip_out; a.vary_out = K ? vary_out : nullptr; a.colors_out = colors ? colors_out : nullptr;
    a.n = n; a.K = K; a.tab = tab;
    unsigned long long* total = reinterpret_cast<unsigned long long*>(c->clip_scratch.p);
    launch_clip_stage(c->stream, a, c->clip_scratch.p + 2, total);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(n_out, total, sizeof(*n_out), hipMemcpyDeviceToHost, c->stream));
    return TRGL_OK;
}

// trgl_draw of device arrays, through the clip stage when `spec` has a plane (checked: tab is spec's table).  The arrays are read when the
// stage runs; its outputs are staged, under the caller's StageHold.
static int draw_device_clipped(trgl_ctx* c, int kind, int K, const trgl_uniforms* u, const ClipSpec* spec, const ClipTable& tab,
                               const double* clip, const double* vary, const uint32_t* colors, uint64_t n) {
    if (!spec) return trgl_draw(c, kind, u, clip, vary, colors, n, TRGL_MEM_DEVICE);
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "clip stage: 2^31 or more triangles in one call");
    int r; void* p = nullptr;
    double* oclip = nullptr; double* ovary = nullptr; uint32_t* ocol = nullptr;
    if ((r = stage_alloc(c, 2 * n * 12 * sizeof(double), &p))) return r;
    oclip = (double*)p;
    if (K) { if ((r = stage_alloc(c, 2 * n * (size_t)K * sizeof(double), &p))) return r; ovary = (double*)p; }
    if (colors) { if ((r = stage_alloc(c, 2 * n * sizeof(uint32_t), &p))) return r; ocol = (uint32_t*)p; }
    unsigned long long n_out = 0;
    if ((r = queue_clip_stage(c, spec->plane, tab, K, clip, vary, colors, n, oclip, ovary, ocol, &n_out))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of a clipped draw: the queue needs the count on the host
    if (n_out == 0) {
        // nothing is queued; with no draw waiting for a flush either, nobody refers to the staged arrays (the stream has just been waited for)
        if (c->draws.empty() && c->stage_hold == 1) for (auto& ch : c->stage) ch.used = 0;
        return TRGL_OK;
    }
    return trgl_draw(c, kind, u, oclip, ovary, ocol, n_out, TRGL_MEM_DEVICE);
}

// What the indexed draws share once their arguments are checked (n_faces > 0): stage a host mesh, run the vertex stage of `vs` (K
// varyings) into staged clip / vary arrays and hand those to trgl_draw - through the clip stage when `spec` is given.
static int draw_indexed_checked(trgl_ctx* c, int vs, int K, int kind, const trgl_uniforms* u, const double projection[16], const double* vertices,
                                int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, const uint32_t* colors, int mem_kind,
                                const ClipSpec* spec = nullptr) {
    int r;
    ClipTable tab;
    if (spec && (r = clip_spec_table(c, "trgl_draw_indexed_vs_clipped", *spec, kind, K, &tab))) return r;
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
    return draw_device_clipped(c, kind, K, u, spec, tab, clip, vary, dcol, n_faces);
}

// the checks of trgl_draw_indexed; *go: there is something to draw
static int check_draw_indexed(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* projection, const double* vertices, int stride,
                              uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, bool* go) {
    *go = false;
    const UserKind* uk = user_kind(c, kind);
    if (kind != TRGL_SHADER_PHONG && kind != TRGL_SHADER_EYE && !(uk && uk->K == TRGL_VARY_PHONG))     // (a user kind's varyings: the PHONG layout)
        return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: kind must be PHONG, EYE or a user kind registered with 24 varyings");
    if (!u || !projection || !vertices || !indices) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: null argument");
    if (stride < 8) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: vertex stride must be >= 8 doubles (pos3, normal3, uv2)");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: bad mem_kind");
    if (n_faces == 0) return TRGL_OK;
    if (n_faces > 0xffffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, "trgl_draw_indexed: too many faces in one call");
    if (mem_kind == TRGL_MEM_HOST)
        for (uint64_t k = 0; k < 3 * n_faces; ++k)
            if (indices[k] >= n_vertices) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed: index out of range");
    *go = true;
    return TRGL_OK;
}

// the checks of trgl_draw_indexed_vs; K of the stage comes back in *K
static int check_draw_indexed_vs(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double* projection, const double* vertices, int stride,
                                 uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, int* K, bool* go) {
    *go = false;
    int r;
    if ((r = check_vertex_call(c, "trgl_draw_indexed_vs", vs, false, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, K))) return r;
    // (what trgl_draw would refuse is refused before the vertex stage is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: unknown shader kind");
    if (kind_K != *K) return fail(c, TRGL_E_INVALID, "trgl_draw_indexed_vs: the shader kind and the vertex shader differ in their number of varyings");
    if ((r = check_kind_uniforms(c, "trgl_draw_indexed_vs", kind, u))) return r;
    *go = n_faces != 0;
    return TRGL_OK;
}

// ---- instanced draws (include/trgl.h: trgl_draw_instanced) ----
struct InstanceCall {
    int vs; const trgl_uniforms* u; const double* projection;
    const double* vertices; int stride; uint64_t n_vertices; const uint32_t* indices; uint64_t n_faces; const uint32_t* face_colors; int mesh_mem;
    const double* instances; int inst_stride; uint64_t n_inst; const uint32_t* inst_colors; const uint8_t* visible; int inst_mem;
    const uint32_t* order = nullptr; uint64_t n_order = 0; int order_mem = TRGL_MEM_HOST;      // the ordered calls; order null: ascending i
};

// what trgl_draw_instanced and trgl_instance_stage check alike; K of the stage comes back in *K; *go: there is something to run
static int check_instance_call(trgl_ctx* c, const char* who, const InstanceCall& a, int* K, bool* go) {
    *go = false;
    const std::string w = std::string(who) + ": ";
    int r;
    // (with no instances nothing is read: the indices are then not looked at either)
    if ((r = check_vertex_call(c, who, a.vs, true, a.u, a.projection, a.vertices, a.stride, a.n_vertices, a.indices, a.n_inst ? a.n_faces : 0, a.mesh_mem, K))) return r;
    if (!valid_mem_kind(a.inst_mem)) return fail(c, TRGL_E_INVALID, w + "bad instance_mem_kind");
    if (a.inst_stride < (a.vs < 0 ? 16 : 0)) return fail(c, TRGL_E_INVALID, w + (a.vs < 0 ? "instance stride must be >= 16 doubles (a row-major 4x4 matrix)" : "instance stride must be >= 0"));
    if (a.n_inst && (a.instances == nullptr) != (a.inst_stride == 0)) return fail(c, TRGL_E_INVALID, w + "instances must be null exactly when instance_stride is 0");
    if (a.inst_colors && a.face_colors) return fail(c, TRGL_E_INVALID, w + "face_colors and instance_colors are both given");
    if (a.n_inst > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more instances in one call");
    if (a.inst_mem == TRGL_MEM_DEVICE && (((uintptr_t)a.instances & 7) || ((uintptr_t)a.inst_colors & 3)))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for instances, 4 for colours)");
    *go = a.n_inst != 0 && a.n_faces != 0;
    return TRGL_OK;
}

// what the ordered calls check of their list on top of that (a list with no entries is no list: the call is the unordered one)
static int check_instance_order(trgl_ctx* c, const char* who, const InstanceCall& a, bool go) {
    const std::string w = std::string(who) + ": ";
    if (!valid_mem_kind(a.order_mem)) return fail(c, TRGL_E_INVALID, w + "bad order_mem_kind");
    if ((a.order == nullptr) != (a.n_order == 0)) return fail(c, TRGL_E_INVALID, w + "order must be null exactly when n_order is 0");
    if (a.n_order > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more entries in the order list");
    if (a.order_mem == TRGL_MEM_DEVICE && ((uintptr_t)a.order & 3)) return fail(c, TRGL_E_INVALID, w + "a device order list must be 4-byte aligned");
    if (go && a.order_mem == TRGL_MEM_HOST)
        for (uint64_t p = 0; p < a.n_order; ++p)
            if (a.order[p] >= a.n_inst) return fail(c, TRGL_E_INVALID, w + "an entry of the order list is not an instance");
    return TRGL_OK;
}

// The stages of an instanced call, checked (n_inst, n_faces > 0).  draw: the rows go to staged arrays and to trgl_draw(kind), under a
// StageHold of this call's; else to clip_out / vary_out / colors_out (in a.inst_mem memory) and *n_out receives their number.
static int run_instanced(trgl_ctx* c, const char* who, const InstanceCall& a, int K, bool draw, int kind,
                         double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out) {
    const std::string w = std::string(who) + ": ";
    int r;
    // Memory of this call's: the per-flush arena for a draw; for the stage alone buffers that go with the call (nothing is left staged
    // for a flush that may never come)
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> own;
    auto dev_alloc = [&](size_t bytes, void** p) -> int {
        if (draw) return stage_alloc(c, bytes, p);
        own.emplace_back(new DevBuf<uint8_t>());
        if (int e = own.back()->alloc(c, bytes ? bytes : 1)) return e;
        *p = own.back()->p;
        return TRGL_OK;
    };
    auto dev_copy = [&](const void* src, size_t bytes, void** p) -> int {
        if (draw) return stage_copy(c, src, bytes, p);
        if (int e = dev_alloc(bytes, p)) return e;
        HIPCHK(c, hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
        return TRGL_OK;
    };
    void* p = nullptr;
    const bool builtin = a.vs < 0;
    const bool has_colors = a.inst_colors || a.face_colors;

    // a. which instances are drawn: list (null: all of them, in order) and n_vis
    const uint32_t* list = nullptr;
    uint64_t n_vis = a.n_inst;
    bool mv_done = false, have_host_list = false;
    std::vector<uint32_t> host_list;
    if (a.order && a.order_mem == TRGL_MEM_HOST && (!a.visible || a.inst_mem == TRGL_MEM_HOST)) {
        try {                                                     // (its entries are checked: all below n_inst)
            for (uint64_t q = 0; q < a.n_order; ++q) if (!a.visible || (a.visible[a.order[q]] & 1u)) host_list.push_back(a.order[q]);
        } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, w + "out of memory"); }
        n_vis = host_list.size(); have_host_list = true;
    } else if (a.order) {
        // the compaction over the positions: a device list (its entries may be anything), or device bytes behind a host list
        const uint32_t* dorder = a.order; const uint8_t* dvis = a.visible;
        if (a.order_mem == TRGL_MEM_HOST) { if ((r = dev_copy(a.order, a.n_order * sizeof(uint32_t), &p))) return r; dorder = (const uint32_t*)p; }
        if (a.visible && a.inst_mem == TRGL_MEM_HOST) { if ((r = dev_copy(a.visible, a.n_inst, &p))) return r; dvis = (const uint8_t*)p; }
        const bool mv_here = builtin && a.inst_mem == TRGL_MEM_DEVICE;      // (host matrices are not on the device yet: k_inst_mv, below)
        if ((r = c->inst_scratch.grow(c, inst_scratch_words(a.n_order))) || (r = c->inst_list.grow(c, a.n_order)) ||
            (mv_here && (r = c->inst_mv.grow(c, 16 * a.n_order)))) return r;
        launch_inst_compact_ordered(c->stream, dorder, (uint32_t)a.n_order, dvis, (uint32_t)a.n_inst, c->inst_scratch.p, c->inst_list.p,
                                    mv_here ? a.u->model_view : nullptr, a.instances, a.inst_stride, mv_here ? c->inst_mv.p : nullptr);
        HIPCHK(c, hipGetLastError());
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, c->inst_scratch.p, sizeof(count), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of an ordered call, as below
        n_vis = count; list = c->inst_list.p; mv_done = mv_here;
    } else if (a.visible && a.inst_mem == TRGL_MEM_HOST) {
        try {
            for (uint64_t i = 0; i < a.n_inst; ++i) if (a.visible[i] & 1u) host_list.push_back((uint32_t)i);
        } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, w + "out of memory"); }
        n_vis = host_list.size(); have_host_list = true;
    } else if (a.visible) {
        if ((r = c->inst_scratch.grow(c, inst_scratch_words(a.n_inst))) || (r = c->inst_list.grow(c, a.n_inst)) ||
            (builtin && (r = c->inst_mv.grow(c, 16 * a.n_inst)))) return r;
        launch_inst_compact(c->stream, a.visible, (uint32_t)a.n_inst, c->inst_scratch.p, c->inst_list.p, builtin ? a.u->model_view : nullptr,
                            a.instances, a.inst_stride, builtin ? c->inst_mv.p : nullptr);
        HIPCHK(c, hipGetLastError());
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, c->inst_scratch.p, sizeof(count), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of an instanced call: the queue needs the count on the host
        n_vis = count; list = c->inst_list.p; mv_done = true;
    }
    if (n_out) *n_out = 0;
    if (n_vis == 0) return TRGL_OK;
    if (n_vis * a.n_faces > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    const uint64_t total = n_vis * a.n_faces;

    // host arrays on their way
    const double* dv = a.vertices; const uint32_t* di = a.indices; const uint32_t* dfc = a.face_colors;
    if (a.mesh_mem == TRGL_MEM_HOST) {
        if ((r = dev_copy(a.vertices, a.n_vertices * (size_t)a.stride * sizeof(double), &p))) return r;
        dv = (const double*)p;
        if ((r = dev_copy(a.indices, 3 * a.n_faces * sizeof(uint32_t), &p))) return r;
        di = (const uint32_t*)p;
        if (a.face_colors) { if ((r = dev_copy(a.face_colors, a.n_faces * sizeof(uint32_t), &p))) return r; dfc = (const uint32_t*)p; }
    }
    const double* dinst = a.instances; const uint32_t* dic = a.inst_colors;
    if (have_host_list) { if ((r = dev_copy(host_list.data(), n_vis * sizeof(uint32_t), &p))) return r; list = (const uint32_t*)p; }
    if (a.inst_mem == TRGL_MEM_HOST) {
        if (a.instances) { if ((r = dev_copy(a.instances, a.n_inst * (size_t)a.inst_stride * sizeof(double), &p))) return r; dinst = (const double*)p; }
        if (a.inst_colors) { if ((r = dev_copy(a.inst_colors, a.n_inst * sizeof(uint32_t), &p))) return r; dic = (const uint32_t*)p; }
    }
    if (builtin && !mv_done) {
        if ((r = c->inst_mv.grow(c, 16 * n_vis))) return r;
        launch_inst_mv(c->stream, list, (uint32_t)n_vis, a.u->model_view, dinst, a.inst_stride, c->inst_mv.p);
        HIPCHK(c, hipGetLastError());
    }

    // b. the rows
    const bool host_out = !draw && a.inst_mem == TRGL_MEM_HOST;
    double* clip = clip_out; double* vary = K ? vary_out : nullptr; uint32_t* col = has_colors ? colors_out : nullptr;
    if (draw || host_out) {
        if ((r = dev_alloc(total * 12 * sizeof(double), &p))) return r;
        clip = (double*)p;
        if (K) { if ((r = dev_alloc(total * (size_t)K * sizeof(double), &p))) return r; vary = (double*)p; }
        if (has_colors) { if ((r = dev_alloc(total * sizeof(uint32_t), &p))) return r; col = (uint32_t*)p; }
    }
    InstanceParams ip; std::memset(&ip, 0, sizeof(ip));
    ip.list = list; ip.instances = dinst; ip.mv = builtin ? c->inst_mv.p : nullptr; ip.inst_colors = dic; ip.face_colors = dfc;
    ip.colors = col; ip.total = (uint32_t)total; ip.inst_stride = a.inst_stride;
    if (builtin) {
        launch_instance_vertex_stage(c->stream, ip, a.projection, dv, a.stride, di, (uint32_t)a.n_faces, clip, vary);
        HIPCHK(c, hipGetLastError());
    } else {
        VertexUserInstancedParams q; std::memset(&q, 0, sizeof(q));
        if (a.u) q.v.u = *a.u; else q.v.u.tex_diffuse = q.v.u.tex_normal = q.v.u.tex_specular = -1;
        std::memcpy(q.v.proj, a.projection, sizeof(q.v.proj));
        q.v.vertices = dv; q.v.indices = di; q.v.clip = clip; q.v.vary = vary; q.v.nfaces = (uint32_t)a.n_faces; q.v.stride = a.stride;
        q.i = ip;
        void* args[] = { &q };
        const uint64_t blocks = (total + TRGL_VERTEX_USER_FACES - 1) / TRGL_VERTEX_USER_FACES;
        HIPCHK(c, hipModuleLaunchKernel(c->vertex[a.vs].fn_inst, (unsigned)blocks, 1, 1, TRGL_VERTEX_USER_FACES * 3, 1, 1, 0, c->stream, args, nullptr));
    }

    // c. the draw, or the rows back to their caller
    if (draw) return trgl_draw(c, kind, a.u, clip, vary, col, total, TRGL_MEM_DEVICE);
    if (host_out) {
        HIPCHK(c, hipMemcpyAsync(clip_out, clip, total * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (K) HIPCHK(c, hipMemcpyAsync(vary_out, vary, total * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (has_colors) HIPCHK(c, hipMemcpyAsync(colors_out, col, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (!own.empty()) HIPCHK(c, hipStreamSynchronize(c->stream));       // (they are freed on return)
    *n_out = total;
    return TRGL_OK;
}

// trgl_draw_instanced (a.order null) and trgl_draw_instanced_ordered
static int draw_instanced_call(trgl_ctx* c, const char* who, int kind, const InstanceCall& a) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = std::string(who) + ": ";
    int K = 0; bool go;
    if ((r = check_instance_call(c, who, a, &K, &go)) || (r = check_instance_order(c, who, a, go))) return r;
    // (what trgl_draw would refuse is refused before anything is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (kind_K != K) return fail(c, TRGL_E_INVALID, w + "the shader kind and the vertex stage differ in their number of varyings");
    if ((r = check_kind_uniforms(c, who, kind, a.u)) || !go) return r;
    StageHold hold(c);
    return run_instanced(c, who, a, K, true, kind, nullptr, nullptr, nullptr, nullptr);
}

// trgl_instance_stage (a.order null) and trgl_instance_stage_ordered
static int instance_stage_call(trgl_ctx* c, const char* who, const InstanceCall& a, double* clip_out, double* vary_out, uint32_t* colors_out,
                               uint64_t* n_out) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = std::string(who) + ": ";
    int K = 0; bool go;
    if ((r = check_instance_call(c, who, a, &K, &go)) || (r = check_instance_order(c, who, a, go))) return r;
    if (!n_out) return fail(c, TRGL_E_INVALID, w + "n_out is null");
    *n_out = 0;
    if (!go) return TRGL_OK;
    const bool has_colors = a.inst_colors || a.face_colors;
    if (!clip_out || (K && !vary_out) || (has_colors && !colors_out)) return fail(c, TRGL_E_INVALID, w + "null output");
    if (a.inst_mem == TRGL_MEM_DEVICE && (((uintptr_t)clip_out | (K ? (uintptr_t)vary_out : 0) | (has_colors ? (uintptr_t)colors_out : 0)) & 15))
        return fail(c, TRGL_E_INVALID, w + "device outputs must be 16-byte aligned");
    return run_instanced(c, who, a, K, false, 0, clip_out, vary_out, colors_out, n_out);
}

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
    if (host_list)
        for (uint64_t p = 0; p < n_order; ++p)
            if (order[p] >= G) return fail(c, TRGL_E_INVALID, w + "an entry of the order list is not a group");
    return TRGL_OK;
}

static bool order_rows_aligned(const double* clip, const double* vary, const uint32_t* colors) {
    return !((((uintptr_t)clip | (uintptr_t)vary) & 7) || ((uintptr_t)colors & 3));
}

// The gather over device arrays, queued on the context's stream: one launch per array (vary null: K = 0; colors null: none)
static int queue_order_stage(trgl_ctx* c, int K, const double* clip, const double* vary, const uint32_t* colors, uint64_t G, const uint32_t* order,
                             uint64_t n_order, uint32_t g, double* clip_out, double* vary_out, uint32_t* colors_out) {
    launch_gather_rows(c->stream, clip, clip_out, 12 * sizeof(double), order, (uint32_t)n_order, (uint32_t)G, g);
    if (K) launch_gather_rows(c->stream, vary, vary_out, (uint32_t)K * sizeof(double), order, (uint32_t)n_order, (uint32_t)G, g);
    if (colors) launch_gather_rows(c->stream, colors, colors_out, sizeof(uint32_t), order, (uint32_t)n_order, (uint32_t)G, g);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// ---- point sprites and wide lines (include/trgl.h: trgl_sprite_stage, trgl_draw_sprites, trgl_line_stage, trgl_draw_lines) ----
// The inputs of either stage: n primitives over n_points rows of `stride` doubles (sprites: n_points == n, no indices)
struct QuadInputs { const double* points; int stride; uint64_t n_points; const uint32_t* indices; const uint32_t* colors; uint64_t n; int mem_kind; };

static bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// what the scalars of a sprite call must satisfy; *K = 6 + n_attr
static int check_sprite_params(trgl_ctx* c, const std::string& w, const trgl_sprite_params* P, int stride, int mem_kind, uint64_t n, int* K) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (P->mode != TRGL_SPRITE_VIEW && P->mode != TRGL_SPRITE_SCREEN) return fail(c, TRGL_E_INVALID, w + "bad mode");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
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
    if (!valid_mem_kind(in.mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (in.mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    if (in.stride < 3) return fail(c, TRGL_E_INVALID, w + "point stride must be >= 3 doubles");
    if (!(P->w_min > 0.0) || !(P->w_min - P->w_min == 0.0)) return fail(c, TRGL_E_INVALID, w + "w_min must be positive and finite");
    if (in.n > 0x3fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    if (!in.indices && 2 * in.n > in.n_points) return fail(c, TRGL_E_INVALID, w + "without indices 2 * n_segments points are needed");
    return TRGL_OK;
}

// ... and its arrays (n > 0): present, aligned, outputs apart from inputs; with host memory every index of a line list in range.
// K: the varyings per row when vary_out is given.
static int check_quad_arrays(trgl_ctx* c, const std::string& w, const QuadInputs& in, int K, const double* clip_out, const double* vary_out,
                             const uint32_t* colors_out) {
    if (!in.points || !clip_out || (in.colors && !colors_out)) return fail(c, TRGL_E_INVALID, w + "null array");
    if ((((uintptr_t)in.points | (uintptr_t)clip_out | (uintptr_t)vary_out) & 7) ||
        (((uintptr_t)in.colors | (uintptr_t)in.indices | (in.colors ? (uintptr_t)colors_out : 0)) & 3))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for colours and indices)");
    const struct { const void* p; uint64_t bytes; } ins[3] = { { in.points, in.n_points * (uint64_t)in.stride * 8 }, { in.colors, in.n * 4 },
                                                              { in.indices, in.n * 8 } },
                                                    outs[3] = { { clip_out, in.n * 192 }, { vary_out, in.n * 16 * (uint64_t)K },
                                                                { in.colors ? colors_out : nullptr, in.n * 8 } };
    for (const auto& i : ins)
        for (const auto& o : outs)
            if (ranges_overlap(i.p, i.bytes, o.p, o.bytes)) return fail(c, TRGL_E_INVALID, w + "an output overlaps an input");
    for (int x = 0; x < 3; ++x)
        for (int y = x + 1; y < 3; ++y)
            if (ranges_overlap(outs[x].p, outs[x].bytes, outs[y].p, outs[y].bytes)) return fail(c, TRGL_E_INVALID, w + "two outputs overlap");
    if (in.mem_kind == TRGL_MEM_HOST && in.indices)
        for (uint64_t k = 0; k < 2 * in.n; ++k)
            if (in.indices[k] >= in.n_points) return fail(c, TRGL_E_INVALID, w + "index out of range");
    return TRGL_OK;
}

static int queue_sprite_stage(trgl_ctx* c, const trgl_sprite_params& P, const QuadInputs& in, double* clip_out, double* vary_out, uint32_t* colors_out) {
    SpriteArgs a; std::memset(&a, 0, sizeof(a));
    a.P = P; a.points = in.points; a.colors = in.colors; a.clip_out = clip_out; a.vary_out = vary_out; a.colors_out = in.colors ? colors_out : nullptr;
    a.n = in.n; a.stride = in.stride;
    launch_sprite_stage(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

static int queue_line_stage(trgl_ctx* c, const trgl_line_params& P, const QuadInputs& in, double* clip_out, double* vary_out, uint32_t* colors_out) {
    LineArgs a; std::memset(&a, 0, sizeof(a));
    a.P = P; a.points = in.points; a.indices = in.indices; a.colors = in.colors;
    a.clip_out = clip_out; a.vary_out = vary_out; a.colors_out = in.colors ? colors_out : nullptr;
    a.n_points = in.n_points; a.n = in.n; a.stride = in.stride;
    launch_line_stage(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

// What trgl_sprite_stage (lines null) and trgl_line_stage share once their scalars are checked
static int quad_stage_call(trgl_ctx* c, const std::string& w, const trgl_sprite_params* sprites, const trgl_line_params* lines, const QuadInputs& in,
                           int K, double* clip_out, double* vary_out, uint32_t* colors_out) {
    if (in.n == 0) return TRGL_OK;
    if (sprites && sprites->n_attr && !vary_out) return fail(c, TRGL_E_INVALID, w + "vary_out is null and n_attr is not 0");
    int r;
    if ((r = check_quad_arrays(c, w, in, K, clip_out, vary_out, colors_out))) return r;
    if (in.mem_kind == TRGL_MEM_HOST) {
        if (sprites) host_sprite_stage(*sprites, in.points, in.stride, in.colors, in.n, clip_out, vary_out, colors_out);
        else host_line_stage(*lines, in.points, in.stride, in.indices, in.colors, in.n, clip_out, vary_out, colors_out);
        return TRGL_OK;
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    return sprites ? queue_sprite_stage(c, *sprites, in, clip_out, vary_out, colors_out) : queue_line_stage(c, *lines, in, clip_out, vary_out, colors_out);
}

// ... and trgl_draw_sprites / trgl_draw_lines: the scalars are checked, K is the stage's
static int quad_draw_call(trgl_ctx* c, const std::string& w, const char* who, int kind, const trgl_uniforms* u, const trgl_sprite_params* sprites,
                          const trgl_line_params* lines, const QuadInputs& in, int K) {
    // (what trgl_draw would refuse is refused before anything is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (kind_K != K && !(kind_K == 0 && K == 6)) return fail(c, TRGL_E_INVALID, w + "the shader kind's number of varyings does not fit the stage's");
    int r;
    if ((r = check_kind_uniforms(c, who, kind, u))) return r;
    if (in.n == 0) return TRGL_OK;
    const uint64_t rows = 2 * in.n;
    if (in.mem_kind == TRGL_MEM_HOST) {
        try {
            std::vector<double> oclip(rows * 12), ovary(rows * (size_t)kind_K);
            std::vector<uint32_t> ocol(in.colors ? rows : 0);
            if ((r = quad_stage_call(c, w, sprites, lines, in, K, oclip.data(), kind_K ? ovary.data() : nullptr, in.colors ? ocol.data() : nullptr))) return r;
            return trgl_draw(c, kind, u, oclip.data(), kind_K ? ovary.data() : nullptr, in.colors ? ocol.data() : nullptr, rows, TRGL_MEM_HOST);
        } catch (const std::bad_alloc&) {
            return fail(c, TRGL_E_NOMEM, w + "out of memory");
        }
    }
    if (!in.points) return fail(c, TRGL_E_INVALID, w + "null array");
    StageHold hold(c);
    void* p = nullptr;
    double* oclip = nullptr; double* ovary = nullptr; uint32_t* ocol = nullptr;
    if ((r = stage_alloc(c, rows * 12 * sizeof(double), &p))) return r;
    oclip = (double*)p;
    if (kind_K) { if ((r = stage_alloc(c, rows * (size_t)kind_K * sizeof(double), &p))) return r; ovary = (double*)p; }
    if (in.colors) { if ((r = stage_alloc(c, rows * sizeof(uint32_t), &p))) return r; ocol = (uint32_t*)p; }
    if ((r = quad_stage_call(c, w, sprites, lines, in, K, oclip, ovary, ocol))) return r;
    return trgl_draw(c, kind, u, oclip, ovary, ocol, rows, TRGL_MEM_DEVICE);
}

// ---- skeletal animation (include/trgl.h: trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned) ----
static bool mul_fits(uint64_t a, uint64_t b, uint64_t limit) { return a == 0 || b <= limit / a; }

// what the scalars of a skinning call must satisfy
static int check_skin_params(trgl_ctx* c, const std::string& w, const trgl_skin_params* P, int mem_kind, uint64_t n) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    if (P->vertex_stride < 3) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 3 doubles");
    if (P->n_influences < 1 || P->n_influences > 8) return fail(c, TRGL_E_INVALID, w + "n_influences must be 1 .. 8");
    if (P->n_joints < 1 || P->n_joints > 65536) return fail(c, TRGL_E_INVALID, w + "n_joints must be 1 .. 65536");
    if (P->n_poses < 1) return fail(c, TRGL_E_INVALID, w + "n_poses must be >= 1");
    if (P->palette_stride < 16ull * P->n_joints && !(P->palette_stride == 0 && P->n_poses == 1))
        return fail(c, TRGL_E_INVALID, w + "palette_stride must be >= 16 * n_joints (or 0 with one pose)");
    if (P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (P->flags & ~(TRGL_SKIN_NORMAL | TRGL_SKIN_TANGENT | TRGL_SKIN_BITANGENT)) return fail(c, TRGL_E_INVALID, w + "unknown flag");
    if (((P->flags & TRGL_SKIN_NORMAL) && P->vertex_stride < 6) || ((P->flags & TRGL_SKIN_TANGENT) && P->vertex_stride < 11) ||
        ((P->flags & TRGL_SKIN_BITANGENT) && P->vertex_stride < 14))
        return fail(c, TRGL_E_INVALID, w + "a flagged direction lies outside the vertex record");
    // (every byte count of the call fits 64 bits)
    if (!mul_fits(n, (uint64_t)P->vertex_stride, 1ull << 60) || !mul_fits(n * (uint64_t)P->vertex_stride, P->n_poses, 1ull << 60) ||
        !mul_fits(P->n_poses, P->palette_stride, 1ull << 60))
        return fail(c, TRGL_E_UNSUPPORTED, w + "the arrays are too large");
    return TRGL_OK;
}

// ... and its arrays (n > 0): present, aligned, the output apart from the inputs; with host memory every joint number in range
static int check_skin_arrays(trgl_ctx* c, const std::string& w, const trgl_skin_params& P, const double* vertices, uint64_t n, const uint16_t* joints,
                             const double* weights, const double* palette, int mem_kind, const double* out) {
    if (!vertices || !joints || !weights || !palette || !out) return fail(c, TRGL_E_INVALID, w + "null array");
    if ((((uintptr_t)vertices | (uintptr_t)weights | (uintptr_t)palette | (uintptr_t)out) & 7) || ((uintptr_t)joints & 1))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 2 for joints)");
    const uint64_t ni = (uint64_t)P.n_influences, rec = n * (uint64_t)P.vertex_stride * 8;
    const struct { const void* p; uint64_t bytes; } ins[4] = { { vertices, rec }, { joints, n * ni * 2 }, { weights, n * ni * 8 },
                                                              { palette, ((P.n_poses - 1) * P.palette_stride + 16ull * P.n_joints) * 8 } };
    for (const auto& i : ins)
        if (ranges_overlap(i.p, i.bytes, out, rec * P.n_poses)) return fail(c, TRGL_E_INVALID, w + "the output overlaps an input");
    if (mem_kind == TRGL_MEM_HOST)
        for (uint64_t k = 0; k < n * ni; ++k)
            if (joints[k] >= P.n_joints) return fail(c, TRGL_E_INVALID, w + "joint number out of range");
    return TRGL_OK;
}

// the skin kernel over device arrays (checked), queued on the context's stream
static int queue_skin_stage(trgl_ctx* c, const std::string& w, const trgl_skin_params& P, const double* vertices, uint64_t n, const uint16_t* joints,
                            const double* weights, const double* palette, double* out) {
    if (P.vertex_stride > SKIN_MAX_DEVICE_STRIDE) return fail(c, TRGL_E_UNSUPPORTED, w + "vertex_stride above 5120 doubles with device memory");
    SkinArgs a; std::memset(&a, 0, sizeof(a));
    a.vertices = vertices; a.joints = joints; a.weights = weights; a.palette = palette; a.out = out;
    a.n = n; a.n_poses = P.n_poses; a.palette_stride = P.palette_stride;
    a.stride = (uint32_t)P.vertex_stride; a.n_joints = P.n_joints; a.flags = P.flags;
    a.vb = (uint32_t)std::min<int>(SKIN_BLOCK, SKIN_TILE_DOUBLES / P.vertex_stride);
    a.n_vblocks = (n + a.vb - 1) / a.vb;
    if (!mul_fits(a.n_vblocks, (P.n_poses + SKIN_POSE_GROUP - 1) / SKIN_POSE_GROUP, 0x7fffffffull))
        return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more blocks in one call");
    launch_skin_stage(c->stream, a, P.n_influences);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

extern "C" {

int trgl_sprite_stage(trgl_ctx* c, const trgl_sprite_params* P, const double* points, int stride, const uint32_t* colors, uint64_t n, int mem_kind,
                      double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_sprite_stage: ";
    int K = 0;
    if (int r = check_sprite_params(c, w, P, stride, mem_kind, n, &K)) return r;
    const QuadInputs in{ points, stride, n, nullptr, colors, n, mem_kind };
    return quad_stage_call(c, w, P, nullptr, in, K, clip_out, vary_out, colors_out);
}

int trgl_draw_sprites(trgl_ctx* c, int kind, const trgl_uniforms* u, const trgl_sprite_params* P, const double* points, int stride,
                      const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_sprites: ";
    int K = 0;
    if ((r = check_sprite_params(c, w, P, stride, mem_kind, n, &K))) return r;
    const QuadInputs in{ points, stride, n, nullptr, colors, n, mem_kind };
    return quad_draw_call(c, w, "trgl_draw_sprites", kind, u, P, nullptr, in, K);
}

int trgl_line_stage(trgl_ctx* c, const trgl_line_params* P, const double* points, int stride, uint64_t n_points, const uint32_t* indices,
                    const uint32_t* colors, uint64_t n_segments, int mem_kind, double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_line_stage: ";
    const QuadInputs in{ points, stride, n_points, indices, colors, n_segments, mem_kind };
    if (int r = check_line_params(c, w, P, in)) return r;
    return quad_stage_call(c, w, nullptr, P, in, 6, clip_out, vary_out, colors_out);
}

int trgl_draw_lines(trgl_ctx* c, int kind, const trgl_uniforms* u, const trgl_line_params* P, const double* points, int stride, uint64_t n_points,
                    const uint32_t* indices, const uint32_t* colors, uint64_t n_segments, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_lines: ";
    const QuadInputs in{ points, stride, n_points, indices, colors, n_segments, mem_kind };
    if ((r = check_line_params(c, w, P, in))) return r;
    return quad_draw_call(c, w, "trgl_draw_lines", kind, u, nullptr, P, in, 6);
}

int trgl_skin_stage(trgl_ctx* c, const trgl_skin_params* P, const double* vertices, uint64_t n, const uint16_t* joints, const double* weights,
                    const double* palette, int mem_kind, double* out) {
    const std::string w = "trgl_skin_stage: ";
    int r;
    if ((r = check_skin_params(c, w, P, mem_kind, n))) return r;
    if (n == 0) return TRGL_OK;
    if ((r = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, out))) return r;
    if (mem_kind == TRGL_MEM_HOST) { host_skin_stage(*P, vertices, n, joints, weights, palette, out); return TRGL_OK; }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    return queue_skin_stage(c, w, *P, vertices, n, joints, weights, palette, out);
}

int trgl_pose_palette(trgl_ctx* c, const int32_t* parents, const double* inverse_bind, uint32_t n_joints, const double* local, uint64_t local_stride,
                      uint64_t n_poses, int mem_kind, double* palette, uint64_t palette_stride) {
    const std::string w = "trgl_pose_palette: ";
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    if (n_joints < 1) return fail(c, TRGL_E_INVALID, w + "n_joints must be >= 1");
    for (const uint64_t stride : { local_stride, palette_stride })
        if (stride < 16ull * n_joints && !(stride == 0 && n_poses <= 1)) return fail(c, TRGL_E_INVALID, w + "a stride must be >= 16 * n_joints (or 0 with one pose)");
    if (!mul_fits(n_poses, local_stride, 1ull << 60) || !mul_fits(n_poses, palette_stride, 1ull << 60)) return fail(c, TRGL_E_UNSUPPORTED, w + "the arrays are too large");
    if (n_poses == 0) return TRGL_OK;
    if (!parents || !local || !palette) return fail(c, TRGL_E_INVALID, w + "null array");
    if ((((uintptr_t)inverse_bind | (uintptr_t)local | (uintptr_t)palette) & 7) || ((uintptr_t)parents & 3))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for parents)");
    const uint64_t mats = 16ull * n_joints * 8, out_bytes = (n_poses - 1) * palette_stride * 8 + mats;
    if (ranges_overlap(parents, 4ull * n_joints, palette, out_bytes) || ranges_overlap(inverse_bind, mats, palette, out_bytes) ||
        ranges_overlap(local, (n_poses - 1) * local_stride * 8 + mats, palette, out_bytes))
        return fail(c, TRGL_E_INVALID, w + "the output overlaps an input");
    if (mem_kind == TRGL_MEM_HOST) {
        for (uint32_t j = 0; j < n_joints; ++j)
            if (parents[j] != -1 && !pose_parent_below(parents[j], j)) return fail(c, TRGL_E_INVALID, w + "a parent must be -1 or a joint below its child");
        try {
            host_pose_palette(parents, inverse_bind, n_joints, local, local_stride, n_poses, palette, palette_stride);
        } catch (const std::bad_alloc&) {
            return fail(c, TRGL_E_NOMEM, w + "out of memory");
        }
        return TRGL_OK;
    }
    CHKCTX(c);
    if (int r = end_pending_raster(c)) return r;
    if ((n_poses + POSE_GROUP - 1) / POSE_GROUP > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more blocks in one call");
    PoseArgs a; std::memset(&a, 0, sizeof(a));
    a.parents = parents; a.inverse_bind = inverse_bind; a.local = local; a.palette = palette;
    a.local_stride = local_stride; a.n_poses = n_poses; a.palette_stride = palette_stride; a.n_joints = n_joints;
    launch_pose_palette(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_draw_skinned(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16], const trgl_skin_params* P,
                      const double* vertices, uint64_t n, const uint16_t* joints, const double* weights, const double* palette,
                      const uint32_t* indices, uint64_t n_faces, const uint32_t* colors, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_skinned: ";
    if ((r = check_skin_params(c, w, P, mem_kind, n))) return r;
    if (P->n_poses != 1) return fail(c, TRGL_E_INVALID, w + "n_poses must be 1");
    if (vs == -1 && colors) return fail(c, TRGL_E_INVALID, w + "colors: only with a vertex shader");
    const int stride = P->vertex_stride;
    int K = TRGL_VARY_PHONG; bool go;
    // (what the draw would refuse is refused before the skin stage is queued; `vertices` stands in for the skinned array)
    if (vs == -1) r = check_draw_indexed(c, kind, u, projection, vertices, stride, n, indices, n_faces, mem_kind, &go);
    else r = check_draw_indexed_vs(c, vs, kind, u, projection, vertices, stride, n, indices, n_faces, mem_kind, &K, &go);
    if (r || !go) return r;
    if (n == 0) return fail(c, TRGL_E_INVALID, w + "faces without vertices");
    if (mem_kind == TRGL_MEM_HOST) {
        try {
            std::vector<double> skinned((size_t)n * (size_t)stride);
            if ((r = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, skinned.data()))) return r;
            host_skin_stage(*P, vertices, n, joints, weights, palette, skinned.data());
            return vs == -1 ? trgl_draw_indexed(c, kind, u, projection, skinned.data(), stride, n, indices, n_faces, TRGL_MEM_HOST)
                            : trgl_draw_indexed_vs(c, vs, kind, u, projection, skinned.data(), stride, n, indices, n_faces, colors, TRGL_MEM_HOST);
        } catch (const std::bad_alloc&) {
            return fail(c, TRGL_E_NOMEM, w + "out of memory");
        }
    }
    StageHold hold(c);
    void* p = nullptr;
    if ((r = stage_alloc(c, (size_t)n * (size_t)stride * sizeof(double), &p))) return r;
    double* skinned = (double*)p;
    if ((r = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, skinned))) return r;
    if ((r = queue_skin_stage(c, w, *P, vertices, n, joints, weights, palette, skinned))) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, skinned, stride, n, indices, n_faces, colors, TRGL_MEM_DEVICE);
}

int trgl_triangle_depths(trgl_ctx* c, const double* clip, uint64_t n, uint32_t group, int mode, int mem_kind, double* depths_out) {
    const std::string w = "trgl_triangle_depths: ";
    if (mode != TRGL_TRI_DEPTH_CENTROID && mode != TRGL_TRI_DEPTH_NEAREST && mode != TRGL_TRI_DEPTH_FARTHEST) return fail(c, TRGL_E_INVALID, w + "bad mode");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    if (int r = check_groups(c, w, n, group)) return r;
    if (n == 0) return TRGL_OK;
    if (!clip || !depths_out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (mem_kind == TRGL_MEM_HOST) { host_triangle_depths(clip, n / group, group, mode, depths_out); return TRGL_OK; }
    CHKCTX(c);
    if (((uintptr_t)clip | (uintptr_t)depths_out) & 7) return fail(c, TRGL_E_INVALID, w + "device arrays must be 8-byte aligned");
    launch_triangle_depths(c->stream, clip, (uint32_t)(n / group), group, mode, depths_out);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_order_stage(trgl_ctx* c, int K, const double* clip, const double* vary, const uint32_t* colors, uint64_t n,
                     const uint32_t* order, uint64_t n_order, uint32_t group, int mem_kind,
                     double* clip_out, double* vary_out, uint32_t* colors_out) {
    const std::string w = "trgl_order_stage: ";
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    if (K < 0 || K > TRGL_MAX_USER_VARY) return fail(c, TRGL_E_INVALID, w + "K outside 0..TRGL_MAX_USER_VARY");
    int r;
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
    if (!order_rows_aligned(clip, K ? vary : nullptr, colors) || !order_rows_aligned(clip_out, K ? vary_out : nullptr, colors ? colors_out : nullptr) ||
        ((uintptr_t)order & 3))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for doubles, 4 for colours and the list)");
    return queue_order_stage(c, K, clip, K ? vary : nullptr, colors, n / group, order, n_order, group, clip_out, vary_out, colors_out);
}

int trgl_draw_ordered(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* clip, const double* vary, const uint32_t* colors, uint64_t n,
                      int mem_kind, const uint32_t* order, uint64_t n_order, uint32_t group, int order_mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_ordered: ";
    if (!valid_mem_kind(order_mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad order_mem_kind");
    if ((order == nullptr) != (n_order == 0)) return fail(c, TRGL_E_INVALID, w + "order must be null exactly when n_order is 0");
    if (!order) return trgl_draw(c, kind, u, clip, vary, colors, n, mem_kind);
    // (what trgl_draw would refuse is refused before anything is queued)
    const int K = kind_vary_count(c, kind);
    if (K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad mem_kind");
    if ((r = check_groups(c, w, n, group))) return r;
    if (n && !clip) return fail(c, TRGL_E_INVALID, w + "clip is null");
    if (n && K && !vary) return fail(c, TRGL_E_INVALID, w + "this shader kind needs varyings");
    if ((r = check_kind_uniforms(c, "trgl_draw_ordered", kind, u))) return r;
    const uint64_t G = n / group, rows = n_order * group;
    const bool host_rows = mem_kind == TRGL_MEM_HOST, host_list = order_mem_kind == TRGL_MEM_HOST;
    if ((r = check_order_list(c, w, order, n_order, group, G, host_list))) return r;
    if (!K) vary = nullptr;
    if (host_rows && host_list) {
        try {
            std::vector<double> oclip(rows * 12), ovary(rows * (size_t)K);
            std::vector<uint32_t> ocol(colors ? rows : 0);
            host_order_stage(K, clip, vary, colors, order, n_order, group, oclip.data(), ovary.data(), ocol.data());
            return trgl_draw(c, kind, u, oclip.data(), K ? ovary.data() : nullptr, colors ? ocol.data() : nullptr, rows, TRGL_MEM_HOST);
        } catch (const std::bad_alloc&) {
            return fail(c, TRGL_E_NOMEM, w + "out of memory");
        }
    }
    if ((!host_rows && !order_rows_aligned(clip, vary, colors)) || (!host_list && ((uintptr_t)order & 3)))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for doubles, 4 for colours and the list)");
    StageHold hold(c);
    void* p = nullptr;
    if (host_rows && n) {
        if ((r = stage_copy(c, clip, n * 12 * sizeof(double), &p))) return r;
        clip = (const double*)p;
        if (K) { if ((r = stage_copy(c, vary, n * (size_t)K * sizeof(double), &p))) return r; vary = (const double*)p; }
        if (colors) { if ((r = stage_copy(c, colors, n * sizeof(uint32_t), &p))) return r; colors = (const uint32_t*)p; }
    }
    if (host_list) { if ((r = stage_copy(c, order, n_order * sizeof(uint32_t), &p))) return r; order = (const uint32_t*)p; }
    double* oclip = nullptr; double* ovary = nullptr; uint32_t* ocol = nullptr;
    if ((r = stage_alloc(c, rows * 12 * sizeof(double), &p))) return r;
    oclip = (double*)p;
    if (K) { if ((r = stage_alloc(c, rows * (size_t)K * sizeof(double), &p))) return r; ovary = (double*)p; }
    if (colors) { if ((r = stage_alloc(c, rows * sizeof(uint32_t), &p))) return r; ocol = (uint32_t*)p; }
    if ((r = queue_order_stage(c, K, clip, vary, colors, G, order, n_order, group, oclip, ovary, ocol))) return r;
    return trgl_draw(c, kind, u, oclip, ovary, ocol, rows, TRGL_MEM_DEVICE);
}

int trgl_draw_instanced(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16],
                        const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                        const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind };
    return draw_instanced_call(c, "trgl_draw_instanced", kind, a);
}

int trgl_draw_instanced_ordered(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16],
                                const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                                const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                                const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                                const uint32_t* order, uint64_t n_order, int order_mem_kind) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind, order, n_order, order_mem_kind };
    return draw_instanced_call(c, "trgl_draw_instanced_ordered", kind, a);
}

int trgl_instance_stage(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16],
                        const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                        const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                        double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind };
    return instance_stage_call(c, "trgl_instance_stage", a, clip_out, vary_out, colors_out, n_out);
}

int trgl_instance_stage_ordered(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16],
                                const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                                const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                                const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                                const uint32_t* order, uint64_t n_order, int order_mem_kind,
                                double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind, order, n_order, order_mem_kind };
    return instance_stage_call(c, "trgl_instance_stage_ordered", a, clip_out, vary_out, colors_out, n_out);
}

int trgl_instance_depths(trgl_ctx* c, const double model_view[16], const double point[3], const double* instances, int instance_stride,
                         uint64_t n_instances, int mem_kind, double* depths_out) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: TRGL_MEM_DEVICE needs a context");
    if (!model_view || !point) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: null model_view or point");
    if (instance_stride < 16) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: instance stride must be >= 16 doubles (a row-major 4x4 matrix)");
    if (n_instances > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_instance_depths: 2^31 or more instances in one call");
    if (n_instances == 0) return TRGL_OK;
    if (!instances || !depths_out) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: null array");
    if (mem_kind == TRGL_MEM_HOST) { host_instance_depths(model_view, point, instances, instance_stride, n_instances, depths_out); return TRGL_OK; }
    CHKCTX(c);
    if (((uintptr_t)instances | (uintptr_t)depths_out) & 7) return fail(c, TRGL_E_INVALID, "trgl_instance_depths: device arrays must be 8-byte aligned");
    launch_instance_depths(c->stream, model_view, point, instances, instance_stride, (uint32_t)n_instances, depths_out);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_depth_order(trgl_ctx* c, const double* depths, uint64_t n, int direction, int mem_kind, uint32_t* order_out) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_depth_order: bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_depth_order: TRGL_MEM_DEVICE needs a context");
    if (direction != TRGL_ORDER_BACK_TO_FRONT && direction != TRGL_ORDER_FRONT_TO_BACK) return fail(c, TRGL_E_INVALID, "trgl_depth_order: bad direction");
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_depth_order: 2^31 or more depths in one call");
    if (n == 0) return TRGL_OK;
    if (!depths || !order_out) return fail(c, TRGL_E_INVALID, "trgl_depth_order: null array");
    const bool front_to_back = direction == TRGL_ORDER_FRONT_TO_BACK;
    if (mem_kind == TRGL_MEM_HOST) {
        if (!host_depth_order(depths, n, front_to_back, order_out)) return fail(c, TRGL_E_NOMEM, "trgl_depth_order: out of memory");
        return TRGL_OK;
    }
    CHKCTX(c);
    if (((uintptr_t)depths & 7) || ((uintptr_t)order_out & 3))
        return fail(c, TRGL_E_INVALID, "trgl_depth_order: device arrays need natural alignment (8 bytes for depths, 4 for the order)");
    size_t bytes = 0;
    HIPCHK(c, depth_order_scratch_bytes((uint32_t)n, &bytes));
    if (int r = c->order_scratch.grow(c, bytes)) return r;
    HIPCHK(c, launch_depth_order(c->stream, depths, (uint32_t)n, front_to_back, c->order_scratch.p, c->order_scratch.cap, order_out));
    return TRGL_OK;
}

int trgl_register_shader_ex(trgl_ctx* c, const char* source, int n_varyings, uint32_t flags, int* kind) {
    CHKCTX(c);
    if (!kind) return fail(c, TRGL_E_INVALID, "trgl_register_shader: kind is null");
    if (c->user.size() >= TRGL_MAX_USER_SHADERS) return fail(c, TRGL_E_INVALID, "trgl_register_shader: TRGL_MAX_USER_SHADERS already registered");
    std::string log;
    const std::vector<char>* code = nullptr;
    if (int r = user_shader_code(source, n_varyings, flags, &log, &code)) return fail(c, r, "trgl_register_shader: " + log);
    const bool may_discard = (flags & TRGL_SHADER_MAY_DISCARD) != 0;
    UserKind u{ nullptr, nullptr, n_varyings, flags };
    HIPCHK(c, hipModuleLoadData(&u.mod, code->data()));
    const hipError_t e = hipModuleGetFunction(&u.fn, u.mod, may_discard ? USER_RASTER_KERNEL : USER_SHADE_KERNEL);
    if (e != hipSuccess) {
        (void)hipModuleUnload(u.mod);
        return fail(c, TRGL_E_HIP, std::string("hipModuleGetFunction: ") + hipGetErrorString(e));
    }
    c->user.push_back(u);
    *kind = TRGL_SHADER_USER_FIRST + (int)c->user.size() - 1;
    return TRGL_OK;
}

int trgl_register_shader(trgl_ctx* c, const char* source, int n_varyings, int* kind) {
    return trgl_register_shader_ex(c, source, n_varyings, 0u, kind);
}

int trgl_register_vertex_shader(trgl_ctx* c, const char* source, int n_varyings, int* vs) {
    CHKCTX(c);
    if (!vs) return fail(c, TRGL_E_INVALID, "trgl_register_vertex_shader: vs is null");
    if (c->vertex.size() >= TRGL_MAX_USER_VERTEX_SHADERS) return fail(c, TRGL_E_INVALID, "trgl_register_vertex_shader: TRGL_MAX_USER_VERTEX_SHADERS already registered");
    std::string log;
    const std::vector<char>* code = nullptr;
    if (int r = user_vertex_shader_code(source, n_varyings, &log, &code)) return fail(c, r, "trgl_register_vertex_shader: " + log);
    UserVertex v{ nullptr, nullptr, n_varyings, nullptr };
    HIPCHK(c, hipModuleLoadData(&v.mod, code->data()));
    hipError_t e = hipModuleGetFunction(&v.fn, v.mod, USER_VERTEX_KERNEL);
    if (e == hipSuccess) e = hipModuleGetFunction(&v.fn_inst, v.mod, USER_VERTEX_INSTANCED_KERNEL);
    if (e != hipSuccess) {
        (void)hipModuleUnload(v.mod);
        return fail(c, TRGL_E_HIP, std::string("hipModuleGetFunction: ") + hipGetErrorString(e));
    }
    c->vertex.push_back(v);
    *vs = (int)c->vertex.size() - 1;
    return TRGL_OK;
}

int trgl_draw_indexed(trgl_ctx* c, int kind, const trgl_uniforms* u, const double projection[16], const double* vertices,
                      int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    bool go;
    if ((r = check_draw_indexed(c, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &go)) || !go) return r;
    return draw_indexed_checked(c, -1, TRGL_VARY_PHONG, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, nullptr, mem_kind);
}

int trgl_draw_indexed_vs(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16], const double* vertices,
                         int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, const uint32_t* colors, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = 0; bool go;
    if ((r = check_draw_indexed_vs(c, vs, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &K, &go)) || !go) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, colors, mem_kind);
}

int trgl_draw_indexed_vs_clipped(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16], const double plane[4],
                                 const trgl_clip_attr* attrs, int n_attrs, const double* vertices, int stride, uint64_t n_vertices,
                                 const uint32_t* indices, uint64_t n_faces, const uint32_t* colors, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = TRGL_VARY_PHONG; bool go;
    if (vs == -1) r = check_draw_indexed(c, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &go);
    else r = check_draw_indexed_vs(c, vs, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &K, &go);
    if (r) return r;
    const ClipSpec spec{ plane, attrs, n_attrs };
    ClipTable tab;
    if ((r = clip_spec_table(c, "trgl_draw_indexed_vs_clipped", spec, kind, K, &tab)) || !go) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, colors, mem_kind, &spec);
}

int trgl_draw_clipped(trgl_ctx* c, int kind, const trgl_uniforms* u, const double plane[4], const trgl_clip_attr* attrs, int n_attrs,
                      const double* clip, const double* vary, const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const int K = kind_vary_count(c, kind);
    if (K < 0) return fail(c, TRGL_E_INVALID, "trgl_draw_clipped: unknown shader kind");
    const ClipSpec spec{ plane, attrs, n_attrs };
    ClipTable tab;
    if ((r = clip_spec_table(c, "trgl_draw_clipped", spec, kind, K, &tab))) return r;
    if (n == 0) return TRGL_OK;
    if (!clip) return fail(c, TRGL_E_INVALID, "trgl_draw_clipped: clip is null");
    if (K && !vary) return fail(c, TRGL_E_INVALID, "trgl_draw_clipped: this shader kind needs varyings");
    if ((r = check_kind_uniforms(c, "trgl_draw_clipped", kind, u))) return r;
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_draw_clipped: bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE) {
        StageHold hold(c);
        return draw_device_clipped(c, kind, K, u, &spec, tab, clip, vary, colors, n);
    }
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_draw_clipped: 2^31 or more triangles in one call");
    try {
        std::vector<double> oclip(2 * n * 12), ovary(2 * n * (size_t)K);
        std::vector<uint32_t> ocol(colors ? 2 * n : 0);
        const uint64_t n_out = host_clip_stage(plane, tab, K, clip, vary, colors, n, oclip.data(), ovary.data(), ocol.data());
        return trgl_draw(c, kind, u, oclip.data(), K ? ovary.data() : nullptr, colors ? ocol.data() : nullptr, n_out, TRGL_MEM_HOST);
    } catch (const std::bad_alloc&) {
        return fail(c, TRGL_E_NOMEM, "trgl_draw_clipped: out of memory");
    }
}

int trgl_clip_stage(trgl_ctx* c, const double plane[4], const trgl_clip_attr* attrs, int n_attrs, int K, const double* clip, const double* vary,
                    const uint32_t* colors, uint64_t n, double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out, int mem_kind) {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, "trgl_clip_stage: bad mem_kind");
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, "trgl_clip_stage: TRGL_MEM_DEVICE needs a context");
    if (!plane || !n_out) return fail(c, TRGL_E_INVALID, "trgl_clip_stage: null plane or n_out");
    ClipTable tab;
    if (!clip_table(attrs, n_attrs, K, &tab)) return fail(c, TRGL_E_INVALID, "trgl_clip_stage: invalid clip attribute list (or K outside 0..TRGL_MAX_USER_VARY)");
    *n_out = 0;
    if (n == 0) return TRGL_OK;
    if (!clip || !clip_out || (K && (!vary || !vary_out)) || (colors && !colors_out)) return fail(c, TRGL_E_INVALID, "trgl_clip_stage: null array");
    if (mem_kind == TRGL_MEM_HOST) { *n_out = host_clip_stage(plane, tab, K, clip, vary, colors, n, clip_out, vary_out, colors_out); return TRGL_OK; }
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "trgl_clip_stage: 2^31 or more triangles in one call");
    if (((uintptr_t)clip | (uintptr_t)clip_out | (K ? (uintptr_t)vary | (uintptr_t)vary_out : 0)) & 7 || (colors && (((uintptr_t)colors | (uintptr_t)colors_out) & 3)))
        return fail(c, TRGL_E_INVALID, "trgl_clip_stage: device arrays need natural alignment (8 bytes for doubles, 4 for colours)");
    unsigned long long total = 0;
    if ((r = queue_clip_stage(c, plane, tab, K, clip, vary, colors, n, clip_out, vary_out, colors_out, &total))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = total;
    return TRGL_OK;
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

}  // extern "C"
