// trgl_stage_instance.cpp — the instanced stages of include/trgl.h: trgl_draw_instanced and trgl_instance_stage, their ordered forms,
// and the depths and the order those take (trgl_instance_depths, trgl_depth_order).
// The draws go through trgl_draw (trgl_api.cpp), which owns the queue and its ordering rules.
#include <cstring>

#include "trgl_stage.h"

struct InstanceCall {
    int vs; const trgl_uniforms* u; const double* projection;
    const double* vertices; int stride; uint64_t n_vertices; const uint32_t* indices; uint64_t n_faces; const uint32_t* face_colors; int mesh_mem;
    const double* instances; int inst_stride; uint64_t n_inst; const uint32_t* inst_colors; const uint8_t* visible; int inst_mem;
    const uint32_t* order = nullptr; uint64_t n_order = 0; int order_mem = TRGL_MEM_HOST;      // the ordered calls; order null: ascending i
};

// What the four calls check alike, the list of the ordered ones included (a list with no entries is no list: the call is the unordered
// one); K of the stage comes back in *K; *go: there is something to run
static int check_instance_call(trgl_ctx* c, const std::string& w, const InstanceCall& a, int* K, bool* go) {
    *go = false;
    int r;
    // (with no instances nothing is read: the indices are then not looked at either)
    if ((r = check_vertex_call(c, w, a.vs, true, a.u, a.projection, a.vertices, a.stride, a.n_vertices, a.indices, a.n_inst ? a.n_faces : 0, a.mesh_mem, K))) return r;
    if ((r = check_mem(c, w, a.inst_mem, "instance_mem_kind"))) return r;
    if (a.inst_stride < (a.vs < 0 ? 16 : 0))
        return fail(c, TRGL_E_INVALID, w + (a.vs < 0 ? "instance stride must be >= 16 doubles (a row-major 4x4 matrix)" : "instance stride must be >= 0"));
    if (a.n_inst && (a.instances == nullptr) != (a.inst_stride == 0)) return fail(c, TRGL_E_INVALID, w + "instances must be null exactly when instance_stride is 0");
    if (a.inst_colors && a.face_colors) return fail(c, TRGL_E_INVALID, w + "face_colors and instance_colors are both given");
    if (a.n_inst > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more instances in one call");
    if (a.inst_mem == TRGL_MEM_DEVICE && !aligned({ { a.instances, 8 }, { a.inst_colors, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for instances, 4 for colours)");
    *go = a.n_inst != 0 && a.n_faces != 0;
    if ((r = check_mem(c, w, a.order_mem, "order_mem_kind"))) return r;
    if ((a.order == nullptr) != (a.n_order == 0)) return fail(c, TRGL_E_INVALID, w + "order must be null exactly when n_order is 0");
    if (a.n_order > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more entries in the order list");
    if (a.order_mem == TRGL_MEM_DEVICE && !aligned({ { a.order, 4 } })) return fail(c, TRGL_E_INVALID, w + "a device order list must be 4-byte aligned");
    if (*go && a.order_mem == TRGL_MEM_HOST && !all_below(a.order, a.n_order, a.n_inst))
        return fail(c, TRGL_E_INVALID, w + "an entry of the order list is not an instance");
    return TRGL_OK;
}

// The stages of an instanced call, checked (n_inst, n_faces > 0).  draw: the rows go to staged arrays and to trgl_draw(kind), under a
// StageHold of the caller's; else to `out` (in a.inst_mem memory) and *n_out receives their number.
static int run_instanced(trgl_ctx* c, const std::string& w, const InstanceCall& a, int K, bool draw, int kind, const Rows& out, uint64_t* n_out) {
    int r;
    CallMem mem(c, draw);       // the per-flush arena for a draw; for the stage alone buffers that go with the call
    const bool builtin = a.vs < 0, has_colors = a.inst_colors || a.face_colors;

    // a. which instances are drawn: list (null: all of them, in order) and n_vis
    const uint32_t* list = nullptr;
    uint64_t n_vis = a.n_inst;
    bool mv_done = false, have_host_list = false, on_device = false;
    std::vector<uint32_t> host_list;
    if (a.order && a.order_mem == TRGL_MEM_HOST && (!a.visible || a.inst_mem == TRGL_MEM_HOST)) {
        try {                                                     // (its entries are checked: all below n_inst)
            for (uint64_t q = 0; q < a.n_order; ++q) if (!a.visible || (a.visible[a.order[q]] & 1u)) host_list.push_back(a.order[q]);
        } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, w + "out of memory"); }
        n_vis = host_list.size(); have_host_list = true;
    } else if (a.order) {
        // the compaction over the positions: a device list (its entries may be anything), or device bytes behind a host list
        const uint32_t* dorder = a.order; const uint8_t* dvis = a.visible;
        if (a.order_mem == TRGL_MEM_HOST && (r = mem.copy(a.order, a.n_order, &dorder))) return r;
        if (a.visible && a.inst_mem == TRGL_MEM_HOST && (r = mem.copy(a.visible, a.n_inst, &dvis))) return r;
        const bool mv_here = builtin && a.inst_mem == TRGL_MEM_DEVICE;      // (host matrices are not on the device yet: k_inst_mv, below)
        if ((r = c->inst_scratch.grow(c, inst_scratch_words(a.n_order))) || (r = c->inst_list.grow(c, a.n_order)) ||
            (mv_here && (r = c->inst_mv.grow(c, 16 * a.n_order)))) return r;
        launch_inst_compact_ordered(c->stream, dorder, (uint32_t)a.n_order, dvis, (uint32_t)a.n_inst, c->inst_scratch.p, c->inst_list.p,
                                    mv_here ? a.u->model_view : nullptr, a.instances, a.inst_stride, mv_here ? c->inst_mv.p : nullptr);
        on_device = true; mv_done = mv_here;
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
        on_device = true; mv_done = true;
    }
    if (on_device) {      // either compaction leaves its count in front of the scratch words and the list in inst_list
        HIPCHK(c, hipGetLastError());
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, c->inst_scratch.p, sizeof(count), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of an instanced call: the queue needs the count on the host
        n_vis = count; list = c->inst_list.p;
    }
    if (n_out) *n_out = 0;
    if (n_vis == 0) return TRGL_OK;
    if (n_vis * a.n_faces > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    const uint64_t total = n_vis * a.n_faces;

    // host arrays on their way
    const double* dv = a.vertices; const uint32_t* di = a.indices; const uint32_t* dfc = a.face_colors;
    if (a.mesh_mem == TRGL_MEM_HOST) {
        if ((r = mem.copy(a.vertices, a.n_vertices * (size_t)a.stride, &dv)) || (r = mem.copy(a.indices, 3 * a.n_faces, &di)) ||
            (a.face_colors && (r = mem.copy(a.face_colors, a.n_faces, &dfc)))) return r;
    }
    const double* dinst = a.instances; const uint32_t* dic = a.inst_colors;
    if (have_host_list && (r = mem.copy(host_list.data(), n_vis, &list))) return r;
    if (a.inst_mem == TRGL_MEM_HOST) {
        if ((a.instances && (r = mem.copy(a.instances, a.n_inst * (size_t)a.inst_stride, &dinst))) ||
            (a.inst_colors && (r = mem.copy(a.inst_colors, a.n_inst, &dic)))) return r;
    }
    if (builtin && !mv_done) {
        if ((r = c->inst_mv.grow(c, 16 * n_vis))) return r;
        launch_inst_mv(c->stream, list, (uint32_t)n_vis, a.u->model_view, dinst, a.inst_stride, c->inst_mv.p);
        HIPCHK(c, hipGetLastError());
    }

    // b. the rows
    const bool host_out = !draw && a.inst_mem == TRGL_MEM_HOST;
    Rows o{ out.clip, K ? out.vary : nullptr, has_colors ? out.colors : nullptr };
    if ((draw || host_out) && (r = alloc_rows(mem, total, K, has_colors, &o))) return r;
    InstanceParams ip; std::memset(&ip, 0, sizeof(ip));
    ip.list = list; ip.instances = dinst; ip.mv = builtin ? c->inst_mv.p : nullptr; ip.inst_colors = dic; ip.face_colors = dfc;
    ip.colors = o.colors; ip.total = (uint32_t)total; ip.inst_stride = a.inst_stride;
    if (builtin) {
        launch_instance_vertex_stage(c->stream, ip, a.projection, dv, a.stride, di, (uint32_t)a.n_faces, o.clip, o.vary);
        HIPCHK(c, hipGetLastError());
    } else {
        VertexUserInstancedParams q; std::memset(&q, 0, sizeof(q));
        if (a.u) q.v.u = *a.u; else q.v.u.tex_diffuse = q.v.u.tex_normal = q.v.u.tex_specular = -1;
        std::memcpy(q.v.proj, a.projection, sizeof(q.v.proj));
        q.v.vertices = dv; q.v.indices = di; q.v.clip = o.clip; q.v.vary = o.vary; q.v.nfaces = (uint32_t)a.n_faces; q.v.stride = a.stride;
        q.i = ip;
        void* args[] = { &q };
        const uint64_t blocks = (total + TRGL_VERTEX_USER_FACES - 1) / TRGL_VERTEX_USER_FACES;
        HIPCHK(c, hipModuleLaunchKernel(c->vertex[a.vs].fn_inst, (unsigned)blocks, 1, 1, TRGL_VERTEX_USER_FACES * 3, 1, 1, 0, c->stream, args, nullptr));
    }

    // c. the draw, or the rows back to their caller
    if (draw) return trgl_draw(c, kind, a.u, o.clip, o.vary, o.colors, total, TRGL_MEM_DEVICE);
    if (host_out) {
        HIPCHK(c, hipMemcpyAsync(out.clip, o.clip, total * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (K) HIPCHK(c, hipMemcpyAsync(out.vary, o.vary, total * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (has_colors) HIPCHK(c, hipMemcpyAsync(out.colors, o.colors, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if ((r = mem.done())) return r;       // (its buffers are freed on return)
    *n_out = total;
    return TRGL_OK;
}

// trgl_draw_instanced (a.order null) and trgl_draw_instanced_ordered
static int draw_instanced_call(trgl_ctx* c, const std::string& w, int kind, const InstanceCall& a) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = 0; bool go;
    if ((r = check_instance_call(c, w, a, &K, &go))) return r;
    // (what trgl_draw would refuse is refused before anything is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (kind_K != K) return fail(c, TRGL_E_INVALID, w + "the shader kind and the vertex stage differ in their number of varyings");
    if ((r = check_kind_uniforms(c, w, kind, a.u)) || !go) return r;
    StageHold hold(c);
    return run_instanced(c, w, a, K, true, kind, Rows{}, nullptr);
}

// trgl_instance_stage (a.order null) and trgl_instance_stage_ordered
static int instance_stage_call(trgl_ctx* c, const std::string& w, const InstanceCall& a, const Rows& out, uint64_t* n_out) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    int K = 0; bool go;
    if ((r = check_instance_call(c, w, a, &K, &go))) return r;
    if (!n_out) return fail(c, TRGL_E_INVALID, w + "n_out is null");
    *n_out = 0;
    if (!go) return TRGL_OK;
    const bool has_colors = a.inst_colors || a.face_colors;
    if (!out.clip || (K && !out.vary) || (has_colors && !out.colors)) return fail(c, TRGL_E_INVALID, w + "null output");
    if (a.inst_mem == TRGL_MEM_DEVICE && !aligned({ { out.clip, 16 }, { K ? out.vary : nullptr, 16 }, { has_colors ? out.colors : nullptr, 16 } }))
        return fail(c, TRGL_E_INVALID, w + "device outputs must be 16-byte aligned");
    return run_instanced(c, w, a, K, false, 0, out, n_out);
}

extern "C" {

int trgl_draw_instanced(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16],
                        const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                        const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind };
    return draw_instanced_call(c, "trgl_draw_instanced: ", kind, a);
}

int trgl_draw_instanced_ordered(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16],
                                const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                                const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                                const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                                const uint32_t* order, uint64_t n_order, int order_mem_kind) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind, order, n_order, order_mem_kind };
    return draw_instanced_call(c, "trgl_draw_instanced_ordered: ", kind, a);
}

int trgl_instance_stage(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16],
                        const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                        const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                        const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                        double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind };
    return instance_stage_call(c, "trgl_instance_stage: ", a, Rows{ clip_out, vary_out, colors_out }, n_out);
}

int trgl_instance_stage_ordered(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16],
                                const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                                const uint32_t* face_colors, int mesh_mem_kind, const double* instances, int instance_stride, uint64_t n_instances,
                                const uint32_t* instance_colors, const uint8_t* visible, int instance_mem_kind,
                                const uint32_t* order, uint64_t n_order, int order_mem_kind,
                                double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out) {
    const InstanceCall a{ vs, u, projection, vertices, stride, n_vertices, indices, n_faces, face_colors, mesh_mem_kind,
                          instances, instance_stride, n_instances, instance_colors, visible, instance_mem_kind, order, n_order, order_mem_kind };
    return instance_stage_call(c, "trgl_instance_stage_ordered: ", a, Rows{ clip_out, vary_out, colors_out }, n_out);
}

int trgl_instance_depths(trgl_ctx* c, const double model_view[16], const double point[3], const double* instances, int instance_stride,
                         uint64_t n_instances, int mem_kind, double* depths_out) {
    const std::string w = "trgl_instance_depths: ";
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (!model_view || !point) return fail(c, TRGL_E_INVALID, w + "null model_view or point");
    if (instance_stride < 16) return fail(c, TRGL_E_INVALID, w + "instance stride must be >= 16 doubles (a row-major 4x4 matrix)");
    if (n_instances > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more instances in one call");
    if (n_instances == 0) return TRGL_OK;
    if (!instances || !depths_out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (mem_kind == TRGL_MEM_HOST) { host_instance_depths(model_view, point, instances, instance_stride, n_instances, depths_out); return TRGL_OK; }
    CHKCTX(c);
    if (!aligned({ { instances, 8 }, { depths_out, 8 } })) return fail(c, TRGL_E_INVALID, w + "device arrays must be 8-byte aligned");
    launch_instance_depths(c->stream, model_view, point, instances, instance_stride, (uint32_t)n_instances, depths_out);
    HIPCHK(c, hipGetLastError());
    return TRGL_OK;
}

int trgl_depth_order(trgl_ctx* c, const double* depths, uint64_t n, int direction, int mem_kind, uint32_t* order_out) {
    const std::string w = "trgl_depth_order: ";
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (direction != TRGL_ORDER_BACK_TO_FRONT && direction != TRGL_ORDER_FRONT_TO_BACK) return fail(c, TRGL_E_INVALID, w + "bad direction");
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more depths in one call");
    if (n == 0) return TRGL_OK;
    if (!depths || !order_out) return fail(c, TRGL_E_INVALID, w + "null array");
    const bool front_to_back = direction == TRGL_ORDER_FRONT_TO_BACK;
    if (mem_kind == TRGL_MEM_HOST) return host_depth_order(depths, n, front_to_back, order_out) ? TRGL_OK : fail(c, TRGL_E_NOMEM, w + "out of memory");
    CHKCTX(c);
    if (!aligned({ { depths, 8 }, { order_out, 4 } })) return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for depths, 4 for the order)");
    size_t bytes = 0;
    HIPCHK(c, depth_order_scratch_bytes((uint32_t)n, &bytes));
    if (int r = c->order_scratch.grow(c, bytes)) return r;
    HIPCHK(c, launch_depth_order(c->stream, depths, (uint32_t)n, front_to_back, c->order_scratch.p, c->order_scratch.cap, order_out));
    return TRGL_OK;
}

}  // extern "C"
