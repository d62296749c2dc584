// trgl_stage_mesh.cpp — the stages over an indexed mesh and the draws behind them: the vertex stage (trgl_draw_indexed,
// trgl_draw_indexed_vs, trgl_vertex_stage), the clip stage (trgl_clip_stage, trgl_draw_clipped, trgl_draw_indexed_vs_clipped) and
// skeletal animation (trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned), mesh edges (trgl_mesh_edges, trgl_edge_select,
// trgl_draw_outline), mesh subdivision (trgl_subdiv_topology, trgl_subdiv_vertices, trgl_draw_subdivided) mesh welding (trgl_mesh_weld)
// and mesh levels of detail (trgl_mesh_clean, trgl_mesh_simplify).
// The draws they make go through trgl_draw (trgl_api.cpp), which owns the queue and its ordering rules.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "trgl_stage.h"
#include "skin_core.h"
#include "edge_core.h"
#include "subdiv_core.h"
#include "weld_core.h"
#include "lod_core.h"

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

int trgl::check_vertex_call(trgl_ctx* c, const std::string& w, int vs, bool builtin_ok, const trgl_uniforms* u, const double* projection,
                            const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind,
                            int* K) {
    if (!((builtin_ok && vs == -1) || (vs >= 0 && vs < (int)c->vertex.size()))) return fail(c, TRGL_E_INVALID, w + "unknown vertex shader");
    *K = vs < 0 ? TRGL_VARY_PHONG : c->vertex[vs].K;
    if (!projection || !vertices || !indices) return fail(c, TRGL_E_INVALID, w + "null argument");
    if (vs < 0 && !u) return fail(c, TRGL_E_INVALID, w + "the built-in vertex stage needs uniforms (model_view)");
    if (stride < (vs < 0 ? 8 : 1))
        return fail(c, TRGL_E_INVALID, w + (vs < 0 ? "vertex stride must be >= 8 doubles (pos3, normal3, uv2)" : "vertex stride must be >= 1"));
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (n_faces > 0xffffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "too many faces in one call");
    if (mem_kind == TRGL_MEM_HOST && !all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
    return TRGL_OK;
}

// A plane and an attribute list as the clipped draws take them (null plane: no clipping), and the table made of them
struct ClipSpec { const double* plane; const trgl_clip_attr* attrs; int n_attrs; ClipTable tab; };

// spec.tab for a draw of `kind` with K varyings; n_attrs = -1: the kind's built-in layout
static int clip_spec_table(trgl_ctx* c, const std::string& w, ClipSpec& spec, int kind, int K) {
    if (!spec.plane) return fail(c, TRGL_E_INVALID, w + "plane is null");
    trgl_clip_attr builtin[TRGL_MAX_CLIP_ATTRS];
    const trgl_clip_attr* attrs = spec.attrs; int n_attrs = spec.n_attrs;
    if (n_attrs == -1) {
        attrs = builtin; n_attrs = 0;
        if (kind >= 0 && kind < TRGL_NUM_SHADERS) (void)trgl_clip_layout(kind, builtin, &n_attrs);
        else if (K > 0) return fail(c, TRGL_E_INVALID, w + "a user kind with varyings has no built-in clip layout: pass its attributes");
    }
    if (!clip_table(attrs, n_attrs, K, &spec.tab)) return fail(c, TRGL_E_INVALID, w + "invalid clip attribute list");
    return TRGL_OK;
}

// The clip stage over device arrays, queued on the context's stream; *n_out is complete when the stream has been waited for.
static int queue_clip_stage(trgl_ctx* c, const double plane[4], const ClipTable& tab, int K, const double* clip, const double* vary,
                            const uint32_t* colors, uint64_t n, const Rows& out, unsigned long long* n_out) {
    int r;
    if ((r = c->clip_scratch.grow(c, 2 + clip_scratch_words(n)))) return r;
    ClipArgs a; std::memset(&a, 0, sizeof(a));
    std::memcpy(a.plane, plane, sizeof(a.plane));
    a.clip = clip; a.vary = K ? vary : nullptr; a.colors = colors;
    a.clip_out = out.clip; a.vary_out = K ? out.vary : nullptr; a.colors_out = colors ? out.colors : nullptr;
    a.n = n; a.K = K; a.tab = tab;
    unsigned long long* total = reinterpret_cast<unsigned long long*>(c->clip_scratch.p);
    launch_clip_stage(c->stream, a, c->clip_scratch.p + 2, total);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(n_out, total, sizeof(*n_out), hipMemcpyDeviceToHost, c->stream));
    return TRGL_OK;
}

// trgl_draw of device arrays, through the clip stage when `spec` is given (checked: clip_spec_table).  The arrays are read when the
// stage runs; its outputs are staged, under the caller's StageHold.
static int draw_device_clipped(trgl_ctx* c, int kind, int K, const trgl_uniforms* u, const ClipSpec* spec, const double* clip,
                               const double* vary, const uint32_t* colors, uint64_t n) {
    if (!spec) return trgl_draw(c, kind, u, clip, vary, colors, n, TRGL_MEM_DEVICE);
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, "clip stage: 2^31 or more triangles in one call");
    int r; CallMem mem(c, true); Rows o;
    if ((r = alloc_rows(mem, 2 * n, K, colors != nullptr, &o))) return r;
    unsigned long long n_out = 0;
    if ((r = queue_clip_stage(c, spec->plane, spec->tab, K, clip, vary, colors, n, o, &n_out))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of a clipped draw: the queue needs the count on the host
    if (n_out == 0) {
        // nothing is queued; with no draw waiting for a flush either, nobody refers to the staged arrays (the stream has just been waited for)
        if (c->draws.empty() && c->stage_hold == 1) for (auto& ch : c->stage) ch.used = 0;
        return TRGL_OK;
    }
    return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, n_out, TRGL_MEM_DEVICE);
}

// What the indexed draws share once their arguments are checked (n_faces > 0): stage a host mesh, run the vertex stage of `vs` (K
// varyings) into staged clip / vary arrays and hand those to trgl_draw - through the clip stage when `spec` (checked) is given.
static int draw_indexed_checked(trgl_ctx* c, int vs, int K, int kind, const trgl_uniforms* u, const double projection[16],
                                const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                                const uint32_t* colors, int mem_kind, const ClipSpec* spec = nullptr) {
    int r;
    StageHold hold(c);
    CallMem mem(c, true); Rows o;
    if (mem_kind == TRGL_MEM_HOST) {
        if ((r = mem.copy(vertices, n_vertices * (size_t)stride, &vertices)) || (r = mem.copy(indices, 3 * n_faces, &indices)) ||
            (colors && (r = mem.copy(colors, n_faces, &colors)))) return r;
    }
    if ((r = alloc_rows(mem, n_faces, K, false, &o))) return r;
    if ((r = queue_vertex_stage(c, vs, u, projection, vertices, stride, indices, n_faces, o.clip, o.vary))) return r;
    return draw_device_clipped(c, kind, K, u, spec, o.clip, o.vary, colors, n_faces);
}

// the checks of trgl_draw_indexed; *go: there is something to draw
static int check_draw_indexed(trgl_ctx* c, int kind, const trgl_uniforms* u, const double* projection, const double* vertices, int stride,
                              uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, bool* go) {
    *go = false;
    const std::string w = "trgl_draw_indexed: ";
    const UserKind* uk = user_kind(c, kind);
    if (kind != TRGL_SHADER_PHONG && kind != TRGL_SHADER_EYE && !(uk && uk->K == TRGL_VARY_PHONG))     // (a user kind's: the PHONG layout)
        return fail(c, TRGL_E_INVALID, w + "kind must be PHONG, EYE or a user kind registered with 24 varyings");
    if (!u || !projection || !vertices || !indices) return fail(c, TRGL_E_INVALID, w + "null argument");
    if (stride < 8) return fail(c, TRGL_E_INVALID, w + "vertex stride must be >= 8 doubles (pos3, normal3, uv2)");
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (n_faces == 0) return TRGL_OK;
    if (n_faces > 0xffffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "too many faces in one call");
    if (mem_kind == TRGL_MEM_HOST && !all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
    *go = true;
    return TRGL_OK;
}

// the checks of trgl_draw_indexed_vs; K of the stage comes back in *K
static int check_draw_indexed_vs(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double* projection, const double* vertices,
                                 int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, int* K, bool* go) {
    *go = false;
    const std::string w = "trgl_draw_indexed_vs: ";
    int r = check_vertex_call(c, w, vs, false, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, K); if (r) return r;
    // (what trgl_draw would refuse is refused before the vertex stage is queued)
    const int kind_K = kind_vary_count(c, kind);
    if (kind_K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    if (kind_K != *K) return fail(c, TRGL_E_INVALID, w + "the shader kind and the vertex shader differ in their number of varyings");
    if ((r = check_kind_uniforms(c, w, kind, u))) return r;
    *go = n_faces != 0;
    return TRGL_OK;
}

// ---- skeletal animation (include/trgl.h: trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned) ----
// what the scalars of a skinning call must satisfy
static int check_skin_params(trgl_ctx* c, const std::string& w, const trgl_skin_params* P, int mem_kind, uint64_t n) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (int r = check_mem(c, w, mem_kind)) return r;
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
static int check_skin_arrays(trgl_ctx* c, const std::string& w, const trgl_skin_params& P, const double* vertices, uint64_t n,
                             const uint16_t* joints, const double* weights, const double* palette, int mem_kind, const double* out) {
    if (!vertices || !joints || !weights || !palette || !out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { vertices, 8 }, { weights, 8 }, { palette, 8 }, { out, 8 }, { joints, 2 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 2 for joints)");
    const uint64_t ni = (uint64_t)P.n_influences, rec = n * (uint64_t)P.vertex_stride * 8;
    const struct { const void* p; uint64_t bytes; } ins[4] = { { vertices, rec }, { joints, n * ni * 2 }, { weights, n * ni * 8 },
                                                              { palette, ((P.n_poses - 1) * P.palette_stride + 16ull * P.n_joints) * 8 } };
    for (const auto& i : ins)
        if (arrays_overlap(i.p, i.bytes, out, rec * P.n_poses)) return fail(c, TRGL_E_INVALID, w + "the output overlaps an input");
    if (mem_kind == TRGL_MEM_HOST && !all_below(joints, n * ni, P.n_joints)) return fail(c, TRGL_E_INVALID, w + "joint number out of range");
    return TRGL_OK;
}

// the skin kernel over device arrays (checked), queued on the context's stream
static int queue_skin_stage(trgl_ctx* c, const std::string& w, const trgl_skin_params& P, const double* vertices, uint64_t n,
                            const uint16_t* joints, const double* weights, const double* palette, double* out) {
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

// ---- mesh edges (include/trgl.h: trgl_mesh_edges, trgl_edge_select, trgl_draw_outline) ----
// The arrays of a selection call: the mesh, its edge records and the three outputs (each may be null)
struct EdgeArrays { const double* vertices; int stride; uint64_t n_vertices; const uint32_t* indices; uint64_t n_faces; const uint32_t* edges;
                    uint64_t n_edges; uint8_t* codes; uint32_t* segments; uint32_t* colors; };

// what the scalars of a selection call must satisfy
static int check_edge_params(trgl_ctx* c, const std::string& w, const trgl_edge_params* P, const EdgeArrays& a, int mem_kind) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (P->select & ~(TRGL_EDGE_ANY | TRGL_EDGE_BOUNDARY | TRGL_EDGE_SILHOUETTE | TRGL_EDGE_CREASE)) return fail(c, TRGL_E_INVALID, w + "unknown bit in select");
    if (P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (a.stride < 3) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 3 doubles");
    if (a.n_vertices > 0xffffffffull) return fail(c, TRGL_E_INVALID, w + "n_vertices above 2^32 - 1");
    if (a.n_faces > 0x7fffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "3 * n_faces above 2^31 - 1");
    if (a.n_edges > 3 * a.n_faces) return fail(c, TRGL_E_INVALID, w + "n_edges above 3 * n_faces");
    return TRGL_OK;
}

// ... and its arrays (n_edges > 0): present, aligned, outputs apart from inputs and from one another
static int check_edge_arrays(trgl_ctx* c, const std::string& w, const EdgeArrays& a) {
    if (!a.vertices || !a.indices || !a.edges) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { a.vertices, 8 }, { a.indices, 4 }, { a.edges, 4 }, { a.segments, 4 }, { a.colors, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for vertices, 4 for 32-bit words)");
    struct Range { const void* p; uint64_t bytes; };
    const Range ins[3] = { { a.vertices, a.n_vertices * (uint64_t)a.stride * 8 }, { a.indices, a.n_faces * 12 }, { a.edges, a.n_edges * 16 } };
    const Range outs[3] = { { a.codes, a.n_edges }, { a.segments, a.n_edges * 8 }, { a.colors, a.n_edges * 4 } };
    for (const Range& i : ins)
        for (const Range& o : outs)
            if (arrays_overlap(i.p, i.bytes, o.p, o.bytes)) return fail(c, TRGL_E_INVALID, w + "an output overlaps an input");
    for (int x = 0; x < 3; ++x)
        for (int y = x + 1; y < 3; ++y)
            if (arrays_overlap(outs[x].p, outs[x].bytes, outs[y].p, outs[y].bytes)) return fail(c, TRGL_E_INVALID, w + "two outputs overlap");
    return TRGL_OK;
}

// The selection over device arrays (checked, n_edges > 0), queued on the context's stream; with P.compact, *count is complete when the
// stream has been waited for (count null: it is not fetched)
static int queue_edge_select(trgl_ctx* c, const trgl_edge_params& P, const EdgeArrays& a, unsigned long long* count) {
    int r;
    if (P.compact && (r = c->edge_scratch.grow(c, edge_select_scratch_bytes((uint32_t)a.n_edges)))) return r;
    EdgeSelectArgs k; std::memset(&k, 0, sizeof(k));
    k.P = P; k.vertices = a.vertices; k.indices = a.indices; k.edges = a.edges; k.codes = a.codes; k.segments = a.segments; k.colors = a.colors;
    k.n_vertices = a.n_vertices; k.n_faces = (uint32_t)a.n_faces; k.n_edges = (uint32_t)a.n_edges; k.stride = a.stride;
    const unsigned long long* total = nullptr;
    HIPCHK(c, launch_edge_select(c->stream, k, c->edge_scratch.p, &total));
    if (total && count) HIPCHK(c, hipMemcpyAsync(count, total, sizeof(*count), hipMemcpyDeviceToHost, c->stream));
    return TRGL_OK;
}

// ---- mesh subdivision (include/trgl.h: trgl_subdiv_topology, trgl_subdiv_vertices, trgl_draw_subdivided) ----
// what the scalars of a vertex call must satisfy
static int check_subdiv_params(trgl_ctx* c, const std::string& w, const trgl_subdiv_params* P, uint64_t n_vertices, uint64_t n_edges, int mem_kind) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (P->vertex_stride < 1) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 1");
    if (P->mode != TRGL_SUBDIV_LINEAR && P->mode != TRGL_SUBDIV_LOOP) return fail(c, TRGL_E_INVALID, w + "unknown mode");
    if (P->mode == TRGL_SUBDIV_LOOP && (P->smooth < 0 || P->smooth > P->vertex_stride)) return fail(c, TRGL_E_INVALID, w + "smooth must be 0 .. vertex_stride");
    if (P->reserved32 || P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (n_vertices > 0xffffffffull) return fail(c, TRGL_E_INVALID, w + "n_vertices above 2^32 - 1");
    if (n_edges > 0xffffffffull - n_vertices) return fail(c, TRGL_E_INVALID, w + "n_vertices + n_edges above 2^32 - 1");
    return TRGL_OK;
}

// ... and its arrays (n_vertices > 0): present, aligned, the output apart from the inputs
static int check_subdiv_arrays(trgl_ctx* c, const std::string& w, const trgl_subdiv_params& P, const double* vertices, uint64_t n_vertices,
                               const uint32_t* stencils, uint64_t n_edges, const double* out) {
    if (!vertices || !stencils || !out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { vertices, 8 }, { out, 8 }, { stencils, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for stencils)");
    const uint64_t rec = (uint64_t)P.vertex_stride * 8;
    if (arrays_overlap(vertices, n_vertices * rec, out, (n_vertices + n_edges) * rec) ||
        arrays_overlap(stencils, trgl_subdiv_stencil_words(n_vertices, n_edges) * 4, out, (n_vertices + n_edges) * rec))
        return fail(c, TRGL_E_INVALID, w + "the output overlaps an input");
    return TRGL_OK;
}

// the vertex kernel over device arrays (checked, n_vertices > 0), queued on the context's stream
static int queue_subdiv_vertices(trgl_ctx* c, const std::string& w, const trgl_subdiv_params& P, const double* vertices, uint64_t n_vertices,
                                 const uint32_t* stencils, uint64_t n_edges, double* out) {
    if (!mul_fits(n_vertices + n_edges, (uint64_t)P.vertex_stride, 0x7fffffffull * SUBDIV_BLOCK * SUBDIV_ITEMS))
        return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more blocks in one call");
    SubdivVertexArgs a; std::memset(&a, 0, sizeof(a));
    a.vertices = vertices; a.stencils = stencils; a.out = out; a.n_vertices = n_vertices; a.n_edges = n_edges;
    a.stride = (uint32_t)P.vertex_stride; a.smooth = P.mode == TRGL_SUBDIV_LOOP ? (uint32_t)P.smooth : 0u;
    HIPCHK(c, launch_subdiv_vertices(c->stream, a));
    return TRGL_OK;
}

// ---- mesh welding (include/trgl.h: trgl_mesh_weld) ----
// The arrays of a weld: the records, the indices (may be null) and the four outputs (each may be null)
struct WeldArrays { const double* vertices; uint64_t n_vertices; const uint32_t* indices; uint64_t n_faces; uint32_t* remap; uint32_t* firsts;
                    double* vertices_out; uint32_t* indices_out; };

// what the scalars of a weld must satisfy
static int check_weld_params(trgl_ctx* c, const std::string& w, const trgl_weld_params* P, uint64_t n_vertices, uint64_t n_faces, int mem_kind) {
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (P->reserved32 || P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (P->vertex_stride < 1) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 1");
    if (P->key_offset < 0 || P->key_count < 1 || (int64_t)P->key_offset + P->key_count > P->vertex_stride)
        return fail(c, TRGL_E_INVALID, w + "the key must lie inside the record (key_offset >= 0, key_count >= 1)");
    if (!(P->cell >= 0.0) || std::isinf(P->cell)) return fail(c, TRGL_E_INVALID, w + "cell must be 0 or a finite positive width");
    if (n_vertices > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "n_vertices above 2^31 - 1");
    if (n_faces > 0x7fffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "3 * n_faces above 2^31 - 1");
    if (!mul_fits(n_vertices, (uint64_t)P->vertex_stride * 8, 1ull << 60)) return fail(c, TRGL_E_UNSUPPORTED, w + "the vertex array is too large");
    return TRGL_OK;
}

// ... and its arrays (n_vertices > 0): present, aligned, outputs apart from inputs and from one another
static int check_weld_arrays(trgl_ctx* c, const std::string& w, const trgl_weld_params& P, const WeldArrays& a) {
    if (!a.vertices) return fail(c, TRGL_E_INVALID, w + "vertices is null");
    if (a.indices_out && !a.indices) return fail(c, TRGL_E_INVALID, w + "indices_out needs indices");
    if (!aligned({ { a.vertices, 8 }, { a.vertices_out, 8 }, { a.indices, 4 }, { a.remap, 4 }, { a.firsts, 4 }, { a.indices_out, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for 32-bit words)");
    const uint64_t rec = a.n_vertices * (uint64_t)P.vertex_stride * 8;
    return check_apart(c, w, { { a.vertices, rec }, { a.indices, a.n_faces * 12 } },
                       { { a.remap, a.n_vertices * 4 }, { a.firsts, a.n_vertices * 4 }, { a.vertices_out, rec }, { a.indices_out, a.n_faces * 12 } });
}

// ---- mesh levels of detail (include/trgl.h: trgl_mesh_clean, trgl_mesh_simplify) ----
// the counts of a mesh that both calls accept
static int check_lod_counts(trgl_ctx* c, const std::string& w, uint64_t n_vertices, uint64_t n_faces) {
    if (n_vertices > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "n_vertices above 2^31 - 1");
    if (n_faces > 0x7fffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "3 * n_faces above 2^31 - 1");
    return TRGL_OK;
}

extern "C" {

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
    ClipSpec spec{ plane, attrs, n_attrs, {} };
    if ((r = clip_spec_table(c, "trgl_draw_indexed_vs_clipped: ", spec, kind, K)) || !go) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, vertices, stride, n_vertices, indices, n_faces, colors, mem_kind, &spec);
}

int trgl_vertex_stage(trgl_ctx* c, int vs, const trgl_uniforms* u, const double projection[16], const double* vertices, int stride,
                      uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, double* clip_out, double* vary_out, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_vertex_stage: ";
    int K = 0;
    if ((r = check_vertex_call(c, w, vs, true, u, projection, vertices, stride, n_vertices, indices, n_faces, mem_kind, &K))) return r;
    if (!clip_out || (K && !vary_out)) return fail(c, TRGL_E_INVALID, w + "null output");
    if (n_faces == 0) return TRGL_OK;
    if (mem_kind == TRGL_MEM_DEVICE) {
        if (!aligned({ { clip_out, 16 }, { K ? vary_out : nullptr, 16 } })) return fail(c, TRGL_E_INVALID, w + "device outputs must be 16-byte aligned");
        return queue_vertex_stage(c, vs, u, projection, vertices, stride, indices, n_faces, clip_out, K ? vary_out : nullptr);
    }
    // host memory: through buffers of this call's own, filled in stream order
    CallMem mem(c, false);
    double* d_v = nullptr; uint32_t* d_i = nullptr; Rows o;
    if ((r = mem.alloc(n_vertices * (size_t)stride, &d_v)) || (r = mem.alloc(3 * n_faces, &d_i)) || (r = alloc_rows(mem, n_faces, K, false, &o))) return r;
    HIPCHK(c, hipMemcpyAsync(d_v, vertices, n_vertices * (size_t)stride * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_i, indices, 3 * n_faces * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if ((r = queue_vertex_stage(c, vs, u, projection, d_v, stride, d_i, n_faces, o.clip, o.vary))) return r;
    HIPCHK(c, hipMemcpyAsync(clip_out, o.clip, n_faces * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (K) HIPCHK(c, hipMemcpyAsync(vary_out, o.vary, n_faces * (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return mem.done();
}

int trgl_clip_stage(trgl_ctx* c, const double plane[4], const trgl_clip_attr* attrs, int n_attrs, int K, const double* clip, const double* vary,
                    const uint32_t* colors, uint64_t n, double* clip_out, double* vary_out, uint32_t* colors_out, uint64_t* n_out, int mem_kind) {
    const std::string w = "trgl_clip_stage: ";
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (!plane || !n_out) return fail(c, TRGL_E_INVALID, w + "null plane or n_out");
    ClipTable tab;
    if (!clip_table(attrs, n_attrs, K, &tab)) return fail(c, TRGL_E_INVALID, w + "invalid clip attribute list (or K outside 0..TRGL_MAX_USER_VARY)");
    *n_out = 0;
    if (n == 0) return TRGL_OK;
    if (!clip || !clip_out || (K && (!vary || !vary_out)) || (colors && !colors_out)) return fail(c, TRGL_E_INVALID, w + "null array");
    if (mem_kind == TRGL_MEM_HOST) { *n_out = host_clip_stage(plane, tab, K, clip, vary, colors, n, clip_out, vary_out, colors_out); return TRGL_OK; }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    if (!aligned({ { clip, 8 }, { clip_out, 8 }, { K ? vary : nullptr, 8 }, { K ? vary_out : nullptr, 8 }, { colors, 4 }, { colors ? colors_out : nullptr, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "device arrays need natural alignment (8 bytes for doubles, 4 for colours)");
    unsigned long long total = 0;
    if ((r = queue_clip_stage(c, plane, tab, K, clip, vary, colors, n, Rows{ clip_out, vary_out, colors_out }, &total))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = total;
    return TRGL_OK;
}

int trgl_draw_clipped(trgl_ctx* c, int kind, const trgl_uniforms* u, const double plane[4], const trgl_clip_attr* attrs, int n_attrs,
                      const double* clip, const double* vary, const uint32_t* colors, uint64_t n, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_clipped: ";
    const int K = kind_vary_count(c, kind);
    if (K < 0) return fail(c, TRGL_E_INVALID, w + "unknown shader kind");
    ClipSpec spec{ plane, attrs, n_attrs, {} };
    if ((r = clip_spec_table(c, w, spec, kind, K))) return r;
    if (n == 0) return TRGL_OK;
    if (!clip) return fail(c, TRGL_E_INVALID, w + "clip is null");
    if (K && !vary) return fail(c, TRGL_E_INVALID, w + "this shader kind needs varyings");
    if ((r = check_kind_uniforms(c, w, kind, u)) || (r = check_mem(c, w, mem_kind))) return r;
    if (mem_kind == TRGL_MEM_DEVICE) {
        StageHold hold(c);
        return draw_device_clipped(c, kind, K, u, &spec, clip, vary, colors, n);
    }
    if (n > 0x7fffffffull) return fail(c, TRGL_E_UNSUPPORTED, w + "2^31 or more triangles in one call");
    return no_bad_alloc(c, w, [&] {
        const HostRows host(2 * n, K, colors != nullptr); const Rows& o = host.o;
        const uint64_t n_out = host_clip_stage(plane, spec.tab, K, clip, vary, colors, n, o.clip, o.vary, o.colors);
        return trgl_draw(c, kind, u, o.clip, o.vary, o.colors, n_out, TRGL_MEM_HOST);
    });
}

int trgl_skin_stage(trgl_ctx* c, const trgl_skin_params* P, const double* vertices, uint64_t n, const uint16_t* joints, const double* weights,
                    const double* palette, int mem_kind, double* out) {
    const std::string w = "trgl_skin_stage: ";
    int r = check_skin_params(c, w, P, mem_kind, n); if (r) return r;
    if (n == 0) return TRGL_OK;
    if ((r = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, out))) return r;
    if (mem_kind == TRGL_MEM_HOST) { host_skin_stage(*P, vertices, n, joints, weights, palette, out); return TRGL_OK; }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    return queue_skin_stage(c, w, *P, vertices, n, joints, weights, palette, out);
}

int trgl_pose_palette(trgl_ctx* c, const int32_t* parents, const double* inverse_bind, uint32_t n_joints, const double* local,
                      uint64_t local_stride, uint64_t n_poses, int mem_kind, double* palette, uint64_t palette_stride) {
    const std::string w = "trgl_pose_palette: ";
    if (int r = check_mem(c, w, mem_kind)) return r;
    if (n_joints < 1) return fail(c, TRGL_E_INVALID, w + "n_joints must be >= 1");
    for (const uint64_t stride : { local_stride, palette_stride })
        if (stride < 16ull * n_joints && !(stride == 0 && n_poses <= 1)) return fail(c, TRGL_E_INVALID, w + "a stride must be >= 16 * n_joints (or 0 with one pose)");
    if (!mul_fits(n_poses, local_stride, 1ull << 60) || !mul_fits(n_poses, palette_stride, 1ull << 60))
        return fail(c, TRGL_E_UNSUPPORTED, w + "the arrays are too large");
    if (n_poses == 0) return TRGL_OK;
    if (!parents || !local || !palette) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { inverse_bind, 8 }, { local, 8 }, { palette, 8 }, { parents, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for parents)");
    const uint64_t mats = 16ull * n_joints * 8, out_bytes = (n_poses - 1) * palette_stride * 8 + mats;
    if (arrays_overlap(parents, 4ull * n_joints, palette, out_bytes) || arrays_overlap(inverse_bind, mats, palette, out_bytes) ||
        arrays_overlap(local, (n_poses - 1) * local_stride * 8 + mats, palette, out_bytes))
        return fail(c, TRGL_E_INVALID, w + "the output overlaps an input");
    if (mem_kind == TRGL_MEM_HOST) {
        for (uint32_t j = 0; j < n_joints; ++j)
            if (parents[j] != -1 && !pose_parent_below(parents[j], j)) return fail(c, TRGL_E_INVALID, w + "a parent must be -1 or a joint below its child");
        return no_bad_alloc(c, w, [&] {
            host_pose_palette(parents, inverse_bind, n_joints, local, local_stride, n_poses, palette, palette_stride);
            return TRGL_OK;
        });
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
    if (mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        std::vector<double> skinned((size_t)n * (size_t)stride);
        if (int e = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, skinned.data())) return e;
        host_skin_stage(*P, vertices, n, joints, weights, palette, skinned.data());
        return vs == -1 ? trgl_draw_indexed(c, kind, u, projection, skinned.data(), stride, n, indices, n_faces, TRGL_MEM_HOST)
                        : trgl_draw_indexed_vs(c, vs, kind, u, projection, skinned.data(), stride, n, indices, n_faces, colors, TRGL_MEM_HOST);
    });
    StageHold hold(c);
    double* skinned = nullptr;
    if ((r = CallMem(c, true).alloc((size_t)n * (size_t)stride, &skinned))) return r;
    if ((r = check_skin_arrays(c, w, *P, vertices, n, joints, weights, palette, mem_kind, skinned))) return r;
    if ((r = queue_skin_stage(c, w, *P, vertices, n, joints, weights, palette, skinned))) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, skinned, stride, n, indices, n_faces, colors, TRGL_MEM_DEVICE);
}

int trgl_mesh_edges(trgl_ctx* c, const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, int mem_kind, uint32_t* edges_out, uint64_t* n_edges) {
    const std::string w = "trgl_mesh_edges: ";
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (n_vertices > 0xffffffffull) return fail(c, TRGL_E_INVALID, w + "n_vertices above 2^32 - 1");
    if (n_faces > 0x7fffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "3 * n_faces above 2^31 - 1");
    if (n_faces == 0) { if (n_edges) *n_edges = 0; return TRGL_OK; }
    if (!indices || !edges_out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { indices, 4 }, { edges_out, 4 } })) return fail(c, TRGL_E_INVALID, w + "arrays must be 4-byte aligned");
    if (arrays_overlap(indices, n_faces * 12, edges_out, n_faces * 48)) return fail(c, TRGL_E_INVALID, w + "the output overlaps the input");
    if (mem_kind == TRGL_MEM_HOST) {
        if (!all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
        return no_bad_alloc(c, w, [&] {
            const uint64_t e = host_mesh_edges(indices, n_faces, n_vertices, edges_out);
            if (n_edges) *n_edges = e;
            return TRGL_OK;
        });
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    const uint32_t nh = (uint32_t)(3 * n_faces);
    size_t bytes = 0;
    HIPCHK(c, mesh_edges_scratch_bytes(nh, n_vertices, &bytes));
    if ((r = c->edge_scratch.grow(c, bytes))) return r;
    const unsigned long long* total = nullptr;
    HIPCHK(c, launch_mesh_edges(c->stream, indices, nh, n_vertices, c->edge_scratch.p, c->edge_scratch.cap, edges_out, &total));
    if (n_edges) {
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, total, sizeof(count), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait, at load time
        *n_edges = count;
    }
    return TRGL_OK;
}

// Diagnostic, not part of include/trgl.h (profiles/outline_probe.py): the radix sort of the last trgl_mesh_edges call with these counts
// again, over the keys it left in the context's scratch - the floor that call is measured against.  Queued, no wait.
int trgl_debug_edge_sort(trgl_ctx* c, uint64_t n_faces, uint64_t n_vertices) {
    CHKCTX(c);
    if (n_faces == 0 || n_faces > 0x7fffffffull / 3 || n_vertices > 0xffffffffull) return fail(c, TRGL_E_INVALID, "trgl_debug_edge_sort: bad counts");
    size_t bytes = 0;
    HIPCHK(c, mesh_edges_scratch_bytes((uint32_t)(3 * n_faces), n_vertices, &bytes));
    if (c->edge_scratch.cap < bytes) return fail(c, TRGL_E_STATE, "trgl_debug_edge_sort: no trgl_mesh_edges call of this size came before");
    HIPCHK(c, launch_mesh_edges_sort(c->stream, (uint32_t)(3 * n_faces), n_vertices, c->edge_scratch.p, c->edge_scratch.cap));
    return TRGL_OK;
}

int trgl_edge_select(trgl_ctx* c, const trgl_edge_params* P, const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices,
                     uint64_t n_faces, const uint32_t* edges, uint64_t n_edges, int mem_kind, uint8_t* codes_out, uint32_t* segments_out,
                     uint32_t* colors_out, uint64_t* n_selected) {
    const std::string w = "trgl_edge_select: ";
    const EdgeArrays a{ vertices, stride, n_vertices, indices, n_faces, edges, n_edges, codes_out, segments_out, colors_out };
    int r = check_edge_params(c, w, P, a, mem_kind); if (r) return r;
    const bool wants_count = n_selected && (P->compact || mem_kind == TRGL_MEM_HOST);
    if (n_edges == 0) { if (wants_count) *n_selected = 0; return TRGL_OK; }
    if ((r = check_edge_arrays(c, w, a))) return r;
    if (mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        if (!host_edge_select(*P, vertices, stride, n_vertices, indices, n_faces, edges, n_edges, codes_out, segments_out, colors_out, n_selected))
            return fail(c, TRGL_E_INVALID, w + "a record names a face or a vertex out of range");
        return (int)TRGL_OK;
    });
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    unsigned long long count = 0;
    if ((r = queue_edge_select(c, *P, a, wants_count ? &count : nullptr))) return r;
    if (wants_count) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *n_selected = count;
    }
    return TRGL_OK;
}

int trgl_draw_outline(trgl_ctx* c, int kind, const trgl_uniforms* u, const trgl_line_params* LP, const trgl_edge_params* P, const double* vertices,
                      int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, const uint32_t* edges, uint64_t n_edges,
                      int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_outline: ";
    EdgeArrays a{ vertices, stride, n_vertices, indices, n_faces, edges, n_edges, nullptr, nullptr, nullptr };
    if ((r = check_edge_params(c, w, P, a, mem_kind))) return r;
    // (what trgl_draw_lines would refuse of its scalars is refused before anything is queued: a draw of no segments checks them all)
    static const uint32_t no_index = 0;
    if ((r = trgl_draw_lines(c, kind, u, LP, vertices, stride, n_vertices, &no_index, nullptr, 0, mem_kind))) return r;
    if (n_edges == 0) return TRGL_OK;
    if ((r = check_edge_arrays(c, w, a))) return r;
    trgl_edge_params Q = *P; Q.compact = 1;
    if (mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        std::vector<uint32_t> segments(2 * (size_t)n_edges), colors((size_t)n_edges);
        uint64_t n = 0;
        if (!host_edge_select(Q, vertices, stride, n_vertices, indices, n_faces, edges, n_edges, nullptr, segments.data(), colors.data(), &n))
            return fail(c, TRGL_E_INVALID, w + "a record names a face or a vertex out of range");
        return trgl_draw_lines(c, kind, u, LP, vertices, stride, n_vertices, segments.data(), colors.data(), n, TRGL_MEM_HOST);
    });
    StageHold hold(c);
    CallMem mem(c, true);
    if ((r = mem.alloc(2 * (size_t)n_edges, &a.segments)) || (r = mem.alloc((size_t)n_edges, &a.colors))) return r;
    unsigned long long count = 0;
    if ((r = queue_edge_select(c, Q, a, &count))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait of an outline draw: trgl_draw_lines needs the count on the host
    if (count == 0) {
        // nothing is queued; with no draw waiting for a flush either, nobody refers to the staged arrays (the stream has just been waited for)
        if (c->draws.empty() && c->stage_hold == 1) for (auto& ch : c->stage) ch.used = 0;
        return TRGL_OK;
    }
    return trgl_draw_lines(c, kind, u, LP, vertices, stride, n_vertices, a.segments, a.colors, count, TRGL_MEM_DEVICE);
}

uint64_t trgl_subdiv_stencil_words(uint64_t n_vertices, uint64_t n_edges) { return 6 * n_edges + 4 * n_vertices; }

int trgl_subdiv_topology(trgl_ctx* c, const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, const uint32_t* edges, uint64_t n_edges,
                         int mem_kind, uint32_t* indices_out, uint32_t* stencils_out) {
    const std::string w = "trgl_subdiv_topology: ";
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (n_vertices > 0xffffffffull) return fail(c, TRGL_E_INVALID, w + "n_vertices above 2^32 - 1");
    if (n_faces > 0x7fffffffull / 3) return fail(c, TRGL_E_UNSUPPORTED, w + "3 * n_faces above 2^31 - 1");
    if (n_edges > 3 * n_faces) return fail(c, TRGL_E_INVALID, w + "n_edges above 3 * n_faces");
    if (n_edges > 0xffffffffull - n_vertices) return fail(c, TRGL_E_INVALID, w + "n_vertices + n_edges above 2^32 - 1");
    if (n_faces == 0 || n_vertices == 0) return TRGL_OK;
    if (!indices || (n_edges && !edges) || !indices_out || !stencils_out) return fail(c, TRGL_E_INVALID, w + "null array");
    if (!aligned({ { indices, 4 }, { edges, 4 }, { indices_out, 4 }, { stencils_out, 4 } })) return fail(c, TRGL_E_INVALID, w + "arrays must be 4-byte aligned");
    struct Range { const void* p; uint64_t bytes; };
    const Range ins[2] = { { indices, n_faces * 12 }, { edges, n_edges * 16 } };
    const Range outs[2] = { { indices_out, n_faces * 48 }, { stencils_out, trgl_subdiv_stencil_words(n_vertices, n_edges) * 4 } };
    for (const Range& i : ins)
        for (const Range& o : outs)
            if (arrays_overlap(i.p, i.bytes, o.p, o.bytes)) return fail(c, TRGL_E_INVALID, w + "an output overlaps an input");
    if (arrays_overlap(outs[0].p, outs[0].bytes, outs[1].p, outs[1].bytes)) return fail(c, TRGL_E_INVALID, w + "the two outputs overlap");
    if (mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        if (!host_subdiv_topology(indices, n_faces, n_vertices, edges, n_edges, indices_out, stencils_out))
            return fail(c, TRGL_E_INVALID, w + "an index or a record out of range, an inconsistent record, or a pair that no record names");
        return (int)TRGL_OK;
    });
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    size_t bytes = 0;
    HIPCHK(c, subdiv_topology_scratch_bytes(n_edges, n_vertices, &bytes));
    if ((r = c->subdiv_scratch.grow(c, bytes))) return r;
    HIPCHK(c, launch_subdiv_topology(c->stream, indices, n_faces, n_vertices, edges, n_edges, c->subdiv_scratch.p, c->subdiv_scratch.cap,
                                     indices_out, stencils_out));
    return TRGL_OK;
}

// Diagnostic, not part of include/trgl.h (profiles/subdiv_probe.py): the radix sort of the last trgl_subdiv_topology call with these
// counts again, over the entries it left in the context's scratch - the floor that call is measured against.  Queued, no wait.
int trgl_debug_subdiv_sort(trgl_ctx* c, uint64_t n_edges, uint64_t n_vertices) {
    CHKCTX(c);
    if (n_edges == 0 || n_edges > 0x7fffffffull || n_vertices == 0 || n_vertices > 0xffffffffull - n_edges)
        return fail(c, TRGL_E_INVALID, "trgl_debug_subdiv_sort: bad counts");
    size_t bytes = 0;
    HIPCHK(c, subdiv_topology_scratch_bytes(n_edges, n_vertices, &bytes));
    if (c->subdiv_scratch.cap < bytes) return fail(c, TRGL_E_STATE, "trgl_debug_subdiv_sort: no trgl_subdiv_topology call of this size came before");
    HIPCHK(c, launch_subdiv_topology_sort(c->stream, n_edges, n_vertices, c->subdiv_scratch.p, c->subdiv_scratch.cap));
    return TRGL_OK;
}

int trgl_subdiv_vertices(trgl_ctx* c, const trgl_subdiv_params* P, const double* vertices, uint64_t n_vertices, const uint32_t* stencils,
                         uint64_t n_edges, int mem_kind, double* out) {
    const std::string w = "trgl_subdiv_vertices: ";
    int r = check_subdiv_params(c, w, P, n_vertices, n_edges, mem_kind); if (r) return r;
    if (n_vertices == 0) return TRGL_OK;
    if ((r = check_subdiv_arrays(c, w, *P, vertices, n_vertices, stencils, n_edges, out))) return r;
    if (mem_kind == TRGL_MEM_HOST) {
        if (!host_subdiv_vertices(*P, vertices, n_vertices, stencils, n_edges, out)) return fail(c, TRGL_E_INVALID, w + "a stencil word names no vertex");
        return TRGL_OK;
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    return queue_subdiv_vertices(c, w, *P, vertices, n_vertices, stencils, n_edges, out);
}

int trgl_draw_subdivided(trgl_ctx* c, int vs, int kind, const trgl_uniforms* u, const double projection[16], const trgl_subdiv_params* P,
                         const double* vertices, uint64_t n_vertices, const uint32_t* stencils, uint64_t n_edges, const uint32_t* refined_indices,
                         uint64_t n_refined_faces, const uint32_t* colors, int mem_kind) {
    CHKCTX(c);
    int r = end_pending_raster(c); if (r) return r;
    const std::string w = "trgl_draw_subdivided: ";
    if ((r = check_subdiv_params(c, w, P, n_vertices, n_edges, mem_kind))) return r;
    if (vs == -1 && colors) return fail(c, TRGL_E_INVALID, w + "colors: only with a vertex shader");
    const int stride = P->vertex_stride;
    const uint64_t n = n_vertices + n_edges;
    int K = TRGL_VARY_PHONG; bool go;
    // (what the draw would refuse is refused before the vertex kernel is queued; `vertices` stands in for the refined array)
    if (vs == -1) r = check_draw_indexed(c, kind, u, projection, vertices, stride, n, refined_indices, n_refined_faces, mem_kind, &go);
    else r = check_draw_indexed_vs(c, vs, kind, u, projection, vertices, stride, n, refined_indices, n_refined_faces, mem_kind, &K, &go);
    if (r || !go) return r;
    if (n_vertices == 0) return fail(c, TRGL_E_INVALID, w + "faces without vertices");
    if (mem_kind == TRGL_MEM_HOST) return no_bad_alloc(c, w, [&] {
        std::vector<double> refined((size_t)n * (size_t)stride);
        if (int e = check_subdiv_arrays(c, w, *P, vertices, n_vertices, stencils, n_edges, refined.data())) return e;
        if (!host_subdiv_vertices(*P, vertices, n_vertices, stencils, n_edges, refined.data())) return fail(c, TRGL_E_INVALID, w + "a stencil word names no vertex");
        return vs == -1 ? trgl_draw_indexed(c, kind, u, projection, refined.data(), stride, n, refined_indices, n_refined_faces, TRGL_MEM_HOST)
                        : trgl_draw_indexed_vs(c, vs, kind, u, projection, refined.data(), stride, n, refined_indices, n_refined_faces, colors, TRGL_MEM_HOST);
    });
    StageHold hold(c);
    double* refined = nullptr;
    if ((r = CallMem(c, true).alloc((size_t)n * (size_t)stride, &refined))) return r;
    if ((r = check_subdiv_arrays(c, w, *P, vertices, n_vertices, stencils, n_edges, refined))) return r;
    if ((r = queue_subdiv_vertices(c, w, *P, vertices, n_vertices, stencils, n_edges, refined))) return r;
    return draw_indexed_checked(c, vs, K, kind, u, projection, refined, stride, n, refined_indices, n_refined_faces, colors, TRGL_MEM_DEVICE);
}

int trgl_mesh_weld(trgl_ctx* c, const trgl_weld_params* P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                   int mem_kind, uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out, uint64_t* n_unique) {
    const std::string w = "trgl_mesh_weld: ";
    int r = check_weld_params(c, w, P, n_vertices, n_faces, mem_kind); if (r) return r;
    if (n_vertices == 0) {
        if (n_faces) return fail(c, TRGL_E_INVALID, w + "faces without vertices");
        if (n_unique) *n_unique = 0;
        return TRGL_OK;
    }
    const WeldArrays a{ vertices, n_vertices, indices, n_faces, remap_out, firsts_out, vertices_out, indices_out };
    if ((r = check_weld_arrays(c, w, *P, a))) return r;
    if (mem_kind == TRGL_MEM_HOST) {
        if (indices && !all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
        return no_bad_alloc(c, w, [&] {
            const uint64_t u = host_mesh_weld(*P, vertices, n_vertices, indices, n_faces, remap_out, firsts_out, vertices_out, indices_out);
            if (n_unique) *n_unique = u;
            return TRGL_OK;
        });
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    size_t bytes = 0;
    HIPCHK(c, mesh_weld_scratch_bytes((uint32_t)n_vertices, c->weld_hash_bits, &bytes));
    if ((r = c->weld_scratch.grow(c, bytes))) return r;
    WeldArgs k; std::memset(&k, 0, sizeof(k));
    k.P = *P; k.vertices = vertices; k.indices = indices_out ? indices : nullptr;
    k.remap_out = remap_out; k.firsts_out = firsts_out; k.vertices_out = vertices_out; k.indices_out = indices_out;
    k.n = (uint32_t)n_vertices; k.n_idx = indices_out ? (uint32_t)(3 * n_faces) : 0u; k.hash_bits = c->weld_hash_bits;
    const unsigned long long* total = nullptr;
    HIPCHK(c, launch_mesh_weld(c->stream, k, c->weld_scratch.p, c->weld_scratch.cap, &total));
    if (n_unique) {
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, total, sizeof(count), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait, at load time
        *n_unique = count;
    }
    return TRGL_OK;
}

// Test hook, not part of include/trgl.h (tests/test_weld_gpu.py): later device welds of this context keep only the low `bits` bits of
// the hash (0 .. 64; 64 is the default) and sort over that many - small values force the walk through a run of colliding keys, 0 puts
// every vertex in one run.  The outputs do not change with it.
int trgl_debug_weld_hash_bits(trgl_ctx* c, int bits) {
    CHKCTX(c);
    if (bits < 0 || bits > 64) return fail(c, TRGL_E_INVALID, "trgl_debug_weld_hash_bits: bits must be 0 .. 64");
    c->weld_hash_bits = bits;
    return TRGL_OK;
}

// Diagnostic, not part of include/trgl.h (profiles/weld_probe.py): the radix sort of the last trgl_mesh_weld call with this count again,
// over the pairs it left in the context's scratch - the floor that call is measured against.  Queued, no wait.
int trgl_debug_weld_sort(trgl_ctx* c, uint64_t n_vertices) {
    CHKCTX(c);
    if (n_vertices == 0 || n_vertices > 0x7fffffffull || c->weld_hash_bits < 1) return fail(c, TRGL_E_INVALID, "trgl_debug_weld_sort: bad count, or no hash bits to sort");
    size_t bytes = 0;
    HIPCHK(c, mesh_weld_scratch_bytes((uint32_t)n_vertices, c->weld_hash_bits, &bytes));
    if (c->weld_scratch.cap < bytes) return fail(c, TRGL_E_STATE, "trgl_debug_weld_sort: no trgl_mesh_weld call of this size came before");
    HIPCHK(c, launch_mesh_weld_sort(c->stream, (uint32_t)n_vertices, c->weld_hash_bits, c->weld_scratch.p, c->weld_scratch.cap));
    return TRGL_OK;
}

// Test hook, not part of include/trgl.h (tests/test_weld.py): weld_core.h's hash of the key of every vertex of a host array
int trgl_debug_weld_hash(const trgl_weld_params* P, const double* vertices, uint64_t n_vertices, uint64_t* hashes_out) {
    const std::string w = "trgl_debug_weld_hash: ";
    if (int r = check_weld_params(nullptr, w, P, n_vertices, 0, TRGL_MEM_HOST)) return r;
    if (n_vertices && (!vertices || !hashes_out)) return fail(nullptr, TRGL_E_INVALID, w + "null array");
    for (uint64_t v = 0; v < n_vertices; ++v) hashes_out[v] = weld_hash(vertices + v * (uint64_t)P->vertex_stride, P->key_offset, P->key_count, P->cell);
    return TRGL_OK;
}

int trgl_mesh_clean(trgl_ctx* c, const trgl_clean_params* P, const uint32_t* indices, uint64_t n_faces, const double* vertices, uint64_t n_vertices,
                    int mem_kind, uint32_t* indices_out, uint32_t* face_firsts_out, uint32_t* vremap_out, uint32_t* vfirsts_out, double* vertices_out,
                    uint64_t* counts) {
    const std::string w = "trgl_mesh_clean: ";
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (P->reserved32 || P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (P->flags & ~(TRGL_CLEAN_DUPLICATES | TRGL_CLEAN_VERTICES)) return fail(c, TRGL_E_INVALID, w + "unknown flags");
    if (P->fill != TRGL_CLEAN_FILL_NONE && P->fill != TRGL_CLEAN_FILL_ZERO) return fail(c, TRGL_E_INVALID, w + "unknown fill");
    const bool with_vertices = (P->flags & TRGL_CLEAN_VERTICES) != 0;
    if (!with_vertices && (vremap_out || vfirsts_out || vertices_out))
        return fail(c, TRGL_E_INVALID, w + "vremap_out, vfirsts_out and vertices_out need TRGL_CLEAN_VERTICES");
    if (vertices_out && P->vertex_stride < 1) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 1");
    if ((r = check_lod_counts(c, w, n_vertices, n_faces))) return r;
    const uint64_t rec = vertices_out ? (uint64_t)P->vertex_stride * 8 : 0;
    if (!mul_fits(n_vertices, rec, 1ull << 60)) return fail(c, TRGL_E_UNSUPPORTED, w + "the vertex array is too large");
    if (n_vertices == 0) {
        if (n_faces) return fail(c, TRGL_E_INVALID, w + "faces without vertices");
        if (counts) counts[0] = counts[1] = 0;
        return TRGL_OK;
    }
    if (n_faces && !indices) return fail(c, TRGL_E_INVALID, w + "indices is null");
    if (vertices_out && !vertices) return fail(c, TRGL_E_INVALID, w + "vertices_out needs vertices");
    if (!aligned({ { vertices, 8 }, { vertices_out, 8 }, { indices, 4 }, { indices_out, 4 }, { face_firsts_out, 4 }, { vremap_out, 4 }, { vfirsts_out, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for 32-bit words)");
    if ((r = check_apart(c, w, { { indices, n_faces * 12 }, { vertices_out ? vertices : nullptr, n_vertices * rec } },
                             { { indices_out, n_faces * 12 }, { face_firsts_out, n_faces * 4 }, { vremap_out, n_vertices * 4 }, { vfirsts_out, n_vertices * 4 },
                               { vertices_out, n_vertices * rec } }))) return r;
    if (mem_kind == TRGL_MEM_HOST) {
        if (!all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
        return no_bad_alloc(c, w, [&] {
            uint64_t k[2];
            host_mesh_clean(*P, indices, n_faces, vertices, n_vertices, indices_out, face_firsts_out, vremap_out, vfirsts_out, vertices_out, k);
            if (counts) { counts[0] = k[0]; counts[1] = k[1]; }
            return TRGL_OK;
        });
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    if (n_faces == 0 && !with_vertices) {
        if (counts) { counts[0] = 0; counts[1] = n_vertices; }
        return TRGL_OK;
    }
    size_t bytes = 0;
    HIPCHK(c, mesh_clean_scratch_bytes((uint32_t)n_faces, (uint32_t)n_vertices, c->lod_hash_bits, &bytes));
    if ((r = c->lod_scratch.grow(c, bytes))) return r;
    CleanArgs k; std::memset(&k, 0, sizeof(k));
    k.P = *P; k.indices = indices; k.vertices = vertices;
    k.indices_out = indices_out; k.face_firsts_out = face_firsts_out; k.vremap_out = vremap_out; k.vfirsts_out = vfirsts_out; k.vertices_out = vertices_out;
    k.n_faces = (uint32_t)n_faces; k.n_vertices = (uint32_t)n_vertices; k.hash_bits = c->lod_hash_bits;
    const unsigned long long* totals = nullptr;
    HIPCHK(c, launch_mesh_clean(c->stream, k, c->lod_scratch.p, c->lod_scratch.cap, &totals));
    if (counts) {
        unsigned long long got[2] = { 0, 0 };
        HIPCHK(c, hipMemcpyAsync(got, totals, sizeof(got), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait, at load time
        counts[0] = got[0]; counts[1] = with_vertices ? got[1] : n_vertices;
    }
    return TRGL_OK;
}

int trgl_mesh_simplify(trgl_ctx* c, const trgl_simplify_params* P, const double* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces,
                       int mem_kind, uint32_t* remap_out, uint32_t* firsts_out, double* vertices_out, uint32_t* indices_out, uint32_t* face_firsts_out,
                       uint64_t* counts) {
    const std::string w = "trgl_mesh_simplify: ";
    if (!P) return fail(c, TRGL_E_INVALID, w + "params is null");
    int r = check_mem(c, w, mem_kind); if (r) return r;
    if (P->reserved32 || P->reserved) return fail(c, TRGL_E_INVALID, w + "reserved must be 0");
    if (P->fill != TRGL_CLEAN_FILL_NONE && P->fill != TRGL_CLEAN_FILL_ZERO) return fail(c, TRGL_E_INVALID, w + "unknown fill");
    if (P->vertex_stride < 3) return fail(c, TRGL_E_INVALID, w + "vertex_stride must be >= 3");
    if (P->mean_count < 0 || P->mean_count > P->vertex_stride) return fail(c, TRGL_E_INVALID, w + "mean_count must be 0 .. vertex_stride");
    if (!(P->cell >= 0.0) || std::isinf(P->cell)) return fail(c, TRGL_E_INVALID, w + "cell must be 0 or a finite positive width");
    if ((r = check_lod_counts(c, w, n_vertices, n_faces))) return r;
    const uint64_t rec = (uint64_t)P->vertex_stride * 8;
    if (!mul_fits(n_vertices, rec, 1ull << 60)) return fail(c, TRGL_E_UNSUPPORTED, w + "the vertex array is too large");
    if (n_vertices == 0) {
        if (n_faces) return fail(c, TRGL_E_INVALID, w + "faces without vertices");
        if (counts) counts[0] = counts[1] = 0;
        return TRGL_OK;
    }
    if (!vertices) return fail(c, TRGL_E_INVALID, w + "vertices is null");
    if (n_faces && !indices) return fail(c, TRGL_E_INVALID, w + "indices is null");
    if (!aligned({ { vertices, 8 }, { vertices_out, 8 }, { indices, 4 }, { remap_out, 4 }, { firsts_out, 4 }, { indices_out, 4 }, { face_firsts_out, 4 } }))
        return fail(c, TRGL_E_INVALID, w + "arrays need natural alignment (8 bytes for doubles, 4 for 32-bit words)");
    if ((r = check_apart(c, w, { { vertices, n_vertices * rec }, { indices, n_faces * 12 } },
                             { { remap_out, n_vertices * 4 }, { firsts_out, n_vertices * 4 }, { vertices_out, n_vertices * rec }, { indices_out, n_faces * 12 },
                               { face_firsts_out, n_faces * 4 } }))) return r;
    if (mem_kind == TRGL_MEM_HOST) {
        if (!all_below(indices, 3 * n_faces, n_vertices)) return fail(c, TRGL_E_INVALID, w + "index out of range");
        return no_bad_alloc(c, w, [&] {
            uint64_t k[2];
            host_mesh_simplify(*P, vertices, n_vertices, indices, n_faces, remap_out, firsts_out, vertices_out, indices_out, face_firsts_out, k);
            if (counts) { counts[0] = k[0]; counts[1] = k[1]; }
            return TRGL_OK;
        });
    }
    CHKCTX(c);
    if ((r = end_pending_raster(c))) return r;
    // the arrays between the weld, the mean and the clean: the weld's map, first occurrences, indices and records, the clean's two maps,
    // the referenced words of the mean
    const uint32_t n = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    const size_t words = scratch_align256((size_t)n * 4), rec_bytes = vertices_out ? scratch_align256((size_t)(n_vertices * rec)) : 0;
    size_t weld_bytes = 0, clean_bytes = 0;
    HIPCHK(c, mesh_weld_scratch_bytes(n, c->weld_hash_bits, &weld_bytes));
    HIPCHK(c, mesh_clean_scratch_bytes(F, n, c->lod_hash_bits, &clean_bytes));
    if ((r = c->weld_scratch.grow(c, weld_bytes)) || (r = c->lod_scratch.grow(c, clean_bytes)) ||
        (r = c->lod_work.grow(c, 5 * words + scratch_align256((size_t)F * 12) + rec_bytes))) return r;
    uint8_t* p = c->lod_work.p;
    uint32_t* weld_remap = (uint32_t*)p; uint32_t* weld_firsts = (uint32_t*)(p + words); uint32_t* vremap = (uint32_t*)(p + 2 * words);
    uint32_t* vfirsts = (uint32_t*)(p + 3 * words); uint32_t* referenced = (uint32_t*)(p + 4 * words);
    uint32_t* weld_indices = (uint32_t*)(p + 5 * words);
    double* records = vertices_out ? (double*)(p + 5 * words + scratch_align256((size_t)F * 12)) : nullptr;
    WeldArgs k; std::memset(&k, 0, sizeof(k));
    k.P.vertex_stride = P->vertex_stride; k.P.key_offset = 0; k.P.key_count = 3; k.P.cell = P->cell;
    k.vertices = vertices; k.indices = F ? indices : nullptr;
    k.remap_out = weld_remap; k.firsts_out = weld_firsts; k.vertices_out = records; k.indices_out = F ? weld_indices : nullptr;
    k.n = n; k.n_idx = 3 * F; k.hash_bits = c->weld_hash_bits;
    const unsigned long long* unused = nullptr;
    HIPCHK(c, launch_mesh_weld(c->stream, k, c->weld_scratch.p, c->weld_scratch.cap, &unused));
    if (P->mean_count > 0 && records)
        HIPCHK(c, launch_lod_mean(c->stream, vertices, P->vertex_stride, P->mean_count, n, indices, 3 * F, c->weld_scratch.p, c->weld_hash_bits, referenced,
                                  records));
    CleanArgs q; std::memset(&q, 0, sizeof(q));
    q.P.vertex_stride = P->vertex_stride; q.P.flags = TRGL_CLEAN_DUPLICATES | TRGL_CLEAN_VERTICES; q.P.fill = P->fill;
    q.indices = weld_indices; q.vertices = records;
    q.indices_out = indices_out; q.face_firsts_out = face_firsts_out; q.vremap_out = vremap; q.vfirsts_out = vfirsts; q.vertices_out = vertices_out;
    q.n_faces = F; q.n_vertices = n; q.hash_bits = c->lod_hash_bits;
    const unsigned long long* totals = nullptr;
    HIPCHK(c, launch_mesh_clean(c->stream, q, c->lod_scratch.p, c->lod_scratch.cap, &totals));
    HIPCHK(c, launch_lod_compose(c->stream, n, weld_remap, vremap, remap_out, weld_firsts, vfirsts, firsts_out));
    if (counts) {
        unsigned long long got[2] = { 0, 0 };
        HIPCHK(c, hipMemcpyAsync(got, totals, sizeof(got), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // the one wait, at load time
        counts[0] = got[0]; counts[1] = got[1];
    }
    return TRGL_OK;
}

// Test hook, not part of include/trgl.h (tests/test_lod_gpu.py): later device cleans and simplifies of this context keep only the low
// `bits` bits of the face hash (0 .. 64; 64 is the default) and sort over that many - small values force the walk through a run of
// colliding triples, 0 puts every face in one run.  The outputs do not change with it.
int trgl_debug_lod_hash_bits(trgl_ctx* c, int bits) {
    CHKCTX(c);
    if (bits < 0 || bits > 64) return fail(c, TRGL_E_INVALID, "trgl_debug_lod_hash_bits: bits must be 0 .. 64");
    c->lod_hash_bits = bits;
    return TRGL_OK;
}

// Diagnostic, not part of include/trgl.h (profiles/lod_probe.py): the radix sort of the last trgl_mesh_clean call with these counts again,
// over the pairs it left in the context's scratch - the floor that call is measured against.  Queued, no wait.
int trgl_debug_lod_sort(trgl_ctx* c, uint64_t n_faces, uint64_t n_vertices) {
    CHKCTX(c);
    if (n_faces == 0 || n_faces > 0x7fffffffull / 3 || n_vertices == 0 || n_vertices > 0x7fffffffull || c->lod_hash_bits < 1)
        return fail(c, TRGL_E_INVALID, "trgl_debug_lod_sort: bad counts, or no hash bits to sort");
    size_t bytes = 0;
    HIPCHK(c, mesh_clean_scratch_bytes((uint32_t)n_faces, (uint32_t)n_vertices, c->lod_hash_bits, &bytes));
    if (c->lod_scratch.cap < bytes) return fail(c, TRGL_E_STATE, "trgl_debug_lod_sort: no trgl_mesh_clean call of this size came before");
    HIPCHK(c, launch_mesh_clean_sort(c->stream, (uint32_t)n_faces, (uint32_t)n_vertices, c->lod_hash_bits, c->lod_scratch.p, c->lod_scratch.cap));
    return TRGL_OK;
}

// Test hook, not part of include/trgl.h (tests/lod_cases.py): what the device path sorts face f of a host array by - lod_core.h's hash of
// its canonical triple, or of its own number when it is invalid or degenerate
int trgl_debug_lod_face_hash(const uint32_t* indices, uint64_t n_faces, uint64_t n_vertices, uint64_t* hashes_out) {
    const std::string w = "trgl_debug_lod_face_hash: ";
    if (int r = check_lod_counts(nullptr, w, n_vertices, n_faces)) return r;
    if (n_faces && (!indices || !hashes_out)) return fail(nullptr, TRGL_E_INVALID, w + "null array");
    for (uint64_t f = 0; f < n_faces; ++f) {
        const uint32_t a = indices[3 * f], b = indices[3 * f + 1], d = indices[3 * f + 2];
        hashes_out[f] = lod_face_class(a, b, d, (uint32_t)n_vertices) == LOD_FACE_CANDIDATE ? lod_face_hash(lod_canonical(a, b, d)) : lod_dropped_hash((uint32_t)f);
    }
    return TRGL_OK;
}

}  // extern "C"
