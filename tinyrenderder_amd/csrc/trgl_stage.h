// trgl_stage.h — what the entry points that run a stage in front of a draw share (trgl_stage_mesh.cpp, trgl_stage_instance.cpp,
// trgl_stage_rows.cpp; trgl_passes.cpp for check_mem): the memory-kind checks, the device memory of one call, the output rows of a
// stage in device and in host memory, overlap and alignment predicates.  Private like trgl_ctx.h: neither installed nor embedded.
// Helpers take the caller's prefix `w` ("trgl_x: ") and prepend it to every message.
#pragma once
#include <initializer_list>
#include <memory>
#include <new>

#include "trgl_ctx.h"

namespace trgl {
// check_kind_uniforms (trgl_api.cpp) for a caller known by its prefix
inline int check_kind_uniforms(trgl_ctx* c, const std::string& w, int kind, const trgl_uniforms* u) {
    return check_kind_uniforms(c, w.substr(0, w.size() - 2).c_str(), kind, u);
}

// `mem_kind` (an argument called `name`) is one of the two kinds, and TRGL_MEM_DEVICE comes with a context (a call that has run
// CHKCTX has one)
inline int check_mem(trgl_ctx* c, const std::string& w, int mem_kind, const char* name = "mem_kind") {
    if (!valid_mem_kind(mem_kind)) return fail(c, TRGL_E_INVALID, w + "bad " + name);
    if (mem_kind == TRGL_MEM_DEVICE && !c) return fail(c, TRGL_E_INVALID, w + "TRGL_MEM_DEVICE needs a context");
    return TRGL_OK;
}

// f(), with std::bad_alloc turned into TRGL_E_NOMEM
template <class F> int no_bad_alloc(trgl_ctx* c, const std::string& w, F&& f) {
    try { return f(); } catch (const std::bad_alloc&) { return fail(c, TRGL_E_NOMEM, w + "out of memory"); }
}

// two byte ranges share a byte (a null or empty one shares none)
inline bool arrays_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}
inline bool mul_fits(uint64_t a, uint64_t b, uint64_t limit) { return a == 0 || b <= limit / a; }
// every one of n numbers in host memory (indices, joints, list entries) is below `limit`
template <class T> bool all_below(const T* v, uint64_t n, uint64_t limit) {
    for (uint64_t k = 0; k < n; ++k) if (v[k] >= limit) return false;
    return true;
}
// every pointer of the list is a multiple of its alignment (a power of two; null pointers pass)
struct AlignedTo { const void* p; uintptr_t bytes; };
inline bool aligned(std::initializer_list<AlignedTo> list) {
    for (const AlignedTo& x : list) if ((uintptr_t)x.p & (x.bytes - 1)) return false;
    return true;
}

// a byte range of a call, and the rule that every output lies apart from every input and from every other output
struct ByteRange { const void* p; uint64_t bytes; };
inline int check_apart(trgl_ctx* c, const std::string& w, std::initializer_list<ByteRange> ins, std::initializer_list<ByteRange> outs) {
    for (const ByteRange& i : ins)
        for (const ByteRange& o : outs)
            if (arrays_overlap(i.p, i.bytes, o.p, o.bytes)) return fail(c, TRGL_E_INVALID, w + "an output overlaps an input");
    for (const ByteRange* x = outs.begin(); x != outs.end(); ++x)
        for (const ByteRange* y = x + 1; y != outs.end(); ++y)
            if (arrays_overlap(x->p, x->bytes, y->p, y->bytes)) return fail(c, TRGL_E_INVALID, w + "two outputs overlap");
    return TRGL_OK;
}

// The device memory of one call.  arena: the per-flush arena - a draw's, which must hold a StageHold until trgl_draw has its arrays.
// Else buffers of the call's own that go with this object (a stage-only call: nothing is left staged for a flush that may never come);
// work queued on them is waited for first: done() on the way out of a call that succeeded.
struct CallMem {
    trgl_ctx* c; bool arena;
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> own;
    CallMem(trgl_ctx* x, bool from_arena) : c(x), arena(from_arena) {}
    template <class T> int alloc(size_t n, T** out) {
        void* p = nullptr;
        if (arena) { if (int r = stage_alloc(c, n * sizeof(T), &p)) return r; }
        else {
            own.emplace_back(new DevBuf<uint8_t>());
            if (int r = own.back()->alloc(c, n ? n * sizeof(T) : 1)) return r;
            p = own.back()->p;
        }
        *out = static_cast<T*>(p);
        return TRGL_OK;
    }
    // n elements of host memory, on the device before copy returns (in the arena: the two steps of stage_copy)
    template <class T> int copy(const T* src, size_t n, const T** out) {
        T* p = nullptr;
        if (int r = alloc(n, &p)) return r;
        HIPCHK(c, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        *out = p;
        return TRGL_OK;
    }
    int done() { if (!own.empty()) HIPCHK(c, hipStreamSynchronize(c->stream)); return TRGL_OK; }
};

// The output rows of a stage: clip [rows, 12], vary [rows, K] (null when K = 0), colors [rows] (null without colours) ...
struct Rows { double* clip = nullptr; double* vary = nullptr; uint32_t* colors = nullptr; };
inline int alloc_rows(CallMem& m, uint64_t rows, int K, bool has_colors, Rows* o) {
    int r;
    if ((r = m.alloc(rows * 12, &o->clip)) || (K && (r = m.alloc(rows * (size_t)K, &o->vary)))) return r;
    return has_colors ? m.alloc(rows, &o->colors) : TRGL_OK;
}
// ... and the same in host memory, as `o` (std::bad_alloc: no_bad_alloc)
struct HostRows {
    std::vector<double> clip, vary; std::vector<uint32_t> colors; Rows o;
    HostRows(uint64_t rows, int K, bool has_colors) : clip(rows * 12), vary(rows * (size_t)K), colors(has_colors ? rows : 0) {
        o = Rows{ clip.data(), K ? vary.data() : nullptr, has_colors ? colors.data() : nullptr };
    }
};

// trgl_stage_mesh.cpp: what the calls that run a vertex stage check alike (w: their prefix); K of the stage comes back in *K
int check_vertex_call(trgl_ctx* c, const std::string& w, int vs, bool builtin_ok, const trgl_uniforms* u, const double* projection,
                      const double* vertices, int stride, uint64_t n_vertices, const uint32_t* indices, uint64_t n_faces, int mem_kind, int* K);
}  // namespace trgl
