// trgl_gl.h — the reference's our_gl.h surface (our_gl.h:17-61) over the C ABI of include/trgl.h.
//
// Same names, argument meaning and (silent) error behaviour as the reference:
//   globals  ModelView / Perspective / Viewport / zbuffer        (our_gl.h:17-20)
//   lookat, init_perspective, init_viewport, init_zbuffer        (our_gl.h:25-31)
//   struct IShader, typedef Triangle, rasterize(), print_render_stats()  (our_gl.h:36-61)
//   struct Frustum with createFromMatrix / intersects                    (our_gl.h:68-86), over the Plane / AABB of the geometry header in use
// What changes for a caller, and why:
//   * rasterize() is DEFERRED: it snapshots the clip coordinates, the shader's varyings and the uniforms that can
//     change between calls (the global ModelView is read inside fragment(), main.cpp:116) and batches them; the GPU
//     runs them in submission order.  `zbuffer` is a proxy whose accessors complete the pending work first, so the
//     reference's direct uses of it (main.cpp:700,730,751,759) need no edit; the framebuffer is the caller's own TGAImage,
//     so gl_flush(framebuffer) goes before the places that read its pixels (main.cpp:743,773).
//   * gl_draw_model(model, shader, framebuffer) replaces a whole face loop (main.cpp:660-666,692-698,715-721): the
//     vertex stage runs on the device from Model::vertices / indices (trgl_draw_indexed), 112 B per vertex + 12 B per face
//     cross PCIe instead of 288 + 96 B per face.
//   * a C++ virtual cannot be called from a kernel: IShader gains describe(), returning the POD descriptor of a
//     shader kind the device implements (trgl_shaders.h: FlatShader, GouraudShader, PhongShader, EyeShader).
//     A subclass without one makes rasterize() fail loudly — there is NO CPU fallback.
//   * a fragment stage the device does not implement is a user shader: HIP C++ source registered with gl_register_shader()
//     (compiled at run time for the GPU; the contract is in include/trgl.h) and drawn through a UserShader (trgl_shaders.h);
//     a fragment() that can discard is one too, registered with may_discard = true.  Its kind stays the same when the shim
//     recreates its context for a framebuffer of another size.
//   * a vertex() the device does not implement is a user vertex shader: source registered with gl_register_vertex_shader() and named
//     by UserShader::vertex_kind (trgl_shader_desc::vertex_kind); gl_draw_model() / gl_draw_indexed() then run it in place of the
//     built-in vertex stage, for a shader of any kind with as many varyings.
//   * gl_zbuffer_snapshot(slot) / gl_zbuffer_restore(slot) do what `saved = zbuffer;` / `zbuffer = saved;` (main.cpp:700,730) do without
//     the depths crossing PCIe twice; gl_mesh_bounds(model) is Model::computeAABB (model.cpp:15-40) for a model of the caller's own.
//     gl_mesh_normals(model) / gl_mesh_tangents(model) are Model::generateNormalsIfNeeded / computeTangentsIfNeeded (model.cpp:269-388).
//   * gl_gaussian_blur(framebuffer, radius) is framebuffer.gaussian_blur(radius) (tgaimage.cpp:271-324) on the frame in HBM, byte for
//     byte; TGAImage::scale / gaussian_blur themselves are host loops in trgl_image.h, as in the reference.
//   * shadows (new; the reference has none): gl_shadow_matrix / gl_shadow_mask / gl_modulate turn the depths of a light's view, kept with
//     gl_zbuffer_snapshot, into a mask and multiply it into the frame in HBM (see below, and include/trgl.h).
//   * supersampling and render-to-texture (new; the reference has neither): gl_resolve(framebuffer, factor, &out) box-filters the frame
//     in HBM into a small image, gl_texture_from_framebuffer(framebuffer, slot, factor) makes the filtered frame a texture without
//     leaving HBM, gl_downsample(image, factor, &out) is the same exact filter on the host (see below, and include/trgl.h).
//   * clipping (new; the reference has none): gl_clip_plane(&plane) cuts everything drawn from then on against a plane in clip space
//     before it is rasterized (include/trgl.h, trgl_clip_stage); gl_clip_plane(nullptr) returns to the reference's behaviour.
//   * gl_instance_boxes(local, matrices) / gl_frustum_test(frustum, boxes[, codes]) are getWorldAABB and frustum.intersects for a
//     whole vector of models (trgl_instance_boxes / trgl_frustum_boxes); the codes plug into gl_occlusion_draw and gl_draw_instanced.
//   * one framebuffer at a time: the frame in HBM is that of the TGAImage last named.  An image of another size or bpp gets a context of
//     its own - what was pending for the old image is drawn on the old context first, its pixels come back only through gl_flush(old) in
//     front of the switch, and print_render_stats() counts from zero again; an image of the same size takes the frame over through
//     gl_flush(A); gl_framebuffer_modified(B); ("One framebuffer at a time").
//   * errors of the C ABI (out of memory, a flush beyond 2^32 triangle-tile pairs, a HIP error ...) do not end the process: the
//     call that met one drops its work, gl_flush() / gl_draw_model() / gl_draw_indexed() / gl_postprocess() return false, and
//     gl_last_error() / gl_last_error_message() tell which (sticky until gl_clear_error()).  Only a programming error - an
//     IShader without describe() - still aborts.
// Header-only (C++17 inline variables); link with -ltrgl.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <cstring>

#include "../../include/trgl.h"
// the caller's own value types (the reference's geometry.h) or the repo's minimal ones
#ifdef TRGL_GEOMETRY_HEADER
#include TRGL_GEOMETRY_HEADER
#else
#include "trgl_geometry.h"
#endif
#ifdef TRGL_IMAGE_HEADER
#include TRGL_IMAGE_HEADER
#else
#include "trgl_image.h"
#endif

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
// rasterize() hands its batch to the device when it holds this many triangles
#ifndef TRGL_SHIM_BATCH_TRIS
#define TRGL_SHIM_BATCH_TRIS (std::size_t(1) << 20)
#endif

inline mat<4, 4> ModelView = mat<4, 4>::identity();
inline mat<4, 4> Perspective = mat<4, 4>::identity();
inline mat<4, 4> Viewport = mat<4, 4>::identity();

// The reference's global `std::vector<double> zbuffer` (our_gl.h:20) with the depths living in HBM: every accessor first
// completes what rasterize() has batched and brings the depths to the host copy; anything that can modify the host copy
// marks it, and the next draw uploads it.  `std::vector<double> saved = zbuffer;` (main.cpp:700), `zbuffer = saved;`
// (main.cpp:730), `zbuffer[idx]`, `zbuffer.size()` and passing it as `const std::vector<double>&` (main.cpp:751,759)
// compile and behave as with the vector.
class trgl_zbuffer_proxy {
    std::vector<double> host_;
    void pull() const;                       // pending draws -> device -> host_
    void touched();                          // the caller may have written host_
public:
    operator const std::vector<double>&() const { pull(); return host_; }
    trgl_zbuffer_proxy& operator=(const std::vector<double>& v) { pull(); host_ = v; touched(); return *this; }
    double operator[](std::size_t i) const { pull(); return host_[i]; }
    // `zbuffer[i]` on the (non-const) global: reading it must not mark the host copy as modified - that would upload all W * H
    // depths again before the next draw - so the element comes back as a small reference object that marks on ASSIGNMENT only
    class element {
        trgl_zbuffer_proxy& z_; std::size_t i_;
    public:
        element(trgl_zbuffer_proxy& z, std::size_t i) : z_(z), i_(i) {}
        operator double() const { z_.pull(); return z_.host_[i_]; }
        element& operator=(double v) { z_.pull(); z_.host_[i_] = v; z_.touched(); return *this; }
        element& operator=(const element& o) { return *this = double(o); }
    };
    element operator[](std::size_t i) { return element(*this, i); }
    std::size_t size() const { return host_.size(); }
    bool empty() const { return host_.empty(); }
    const double* data() const { pull(); return host_.data(); }
    double* data() { pull(); touched(); return host_.data(); }
    std::vector<double>::const_iterator begin() const { pull(); return host_.begin(); }
    std::vector<double>::const_iterator end() const { pull(); return host_.end(); }     // (begin() and end() may be evaluated in either order)
    void assign(std::size_t n, double v);    // init_zbuffer (our_gl.cpp:72-74)
    void resize(std::size_t n) { host_.resize(n); }
    std::vector<double>& raw() { return host_; }   // the shim's own access: no synchronisation
};
inline trgl_zbuffer_proxy zbuffer;

// What a shader hands to the device: kind + uniforms + this triangle's varyings/colour (include/trgl.h).
struct trgl_shader_desc {
    int kind = TRGL_SHADER_FLAT;
    trgl_uniforms uniforms{};
    const double* varyings = nullptr;   // K doubles for `kind`, valid until rasterize() returns
    std::uint32_t color = 0xffffffffu;  // FLAT / GOURAUD
    int vertex_kind = -1;               // gl_draw_indexed() / gl_draw_model(): a user vertex shader (gl_register_vertex_shader), -1 = the built-in stage
};

struct IShader {
    static TGAColor sample2D(const TGAImage& img, const vec2& uv) {
        int x = std::min<int>(img.width() - 1, std::max<int>(0, int(uv.x * img.width())));
        int y = std::min<int>(img.height() - 1, std::max<int>(0, int(uv.y * img.height())));
        return img.get(x, y);
    }
    virtual vec4 vertex(int, int) { return vec4(); }
    // Executed on the device; never called on the host.
    virtual std::pair<bool, TGAColor> fragment(const vec3) const {
        std::fprintf(stderr, "trgl: IShader::fragment() runs on the GPU; give the shader a describe()\n");
        std::abort();
    }
    virtual bool describe(trgl_shader_desc&) const { return false; }
    virtual ~IShader() = default;
};

typedef vec<4> Triangle[3];

namespace trgl_shim {

// The image type is the caller's (the reference's TGAImage keeps its bytes-per-pixel private and buffer() non-const,
// tgaimage.h:67-104): everything the shim needs goes through these three.
template <class Img> inline int image_bpp(const Img& im) { return (im.width() > 0 && im.height() > 0) ? int(im.get(0, 0).bytespp) : 0; }   // TGAColor(p, bpp), tgaimage.h:46-50
template <class Img> inline std::uint8_t* image_bytes(const Img& im) { return const_cast<Img&>(im).buffer(); }
inline std::uint32_t pack_bgra(const TGAColor& c) {
    return std::uint32_t(c.bgra[0]) | (std::uint32_t(c.bgra[1]) << 8) | (std::uint32_t(c.bgra[2]) << 16) | (std::uint32_t(c.bgra[3]) << 24);
}

struct State {
    trgl_ctx* ctx = nullptr;
    int w = 0, h = 0, bpp = 0;
    bool zbuffer_dirty_on_host = false;   // init_zbuffer()/host writes not yet on the device
    bool zbuffer_stale_on_host = false;   // the device drew since the host copy was fetched
    bool have_batch = false;
    int kind = 0;
    trgl_uniforms uniforms{};
    std::vector<double> clip, vary;
    std::vector<std::uint32_t> colors;
    mat<4, 4> viewport_at_batch;
    struct UserSource { std::string source; int n_varyings; std::uint32_t flags; };   // flags: TRGL_SHADER_*
    std::vector<UserSource> user;         // gl_register_shader(): registered on every context, in order (kind = USER_FIRST + index)
    struct VertexSource { std::string source; int n_varyings; };
    std::vector<VertexSource> vertex;     // gl_register_vertex_shader(): likewise (vertex kind = index)
    bool clip_on = false;                 // gl_clip_plane(): draws go through the clipped entry points
    double clip_plane[4] = { 0, 0, 0, 0 };
    struct ClipLayout { int kind; std::vector<trgl_clip_attr> attrs; };
    std::vector<ClipLayout> clip_layouts; // gl_clip_layout(): the attribute lists of user kinds
    int err = TRGL_OK;                    // first C-ABI error since gl_clear_error() (a TRGL_E_* code)
    std::string err_msg;
};
inline State& state() { static State s; return s; }

// a C-ABI call failed: remember the first error (code + message); the caller of the shim asks gl_last_error()
inline bool fail(const char* what, int code, trgl_ctx* c) {
    State& s = state();
    if (s.err == TRGL_OK) { s.err = code; s.err_msg = std::string(what) + ": " + trgl_last_error(c); }
    return false;
}
// evaluates to true when the call succeeded
#define TRGL_SHIM_OK(call) ([&]() -> bool { const int rc_ = (call); return rc_ == TRGL_OK ? true : ::trgl_shim::fail(#call, rc_, ::trgl_shim::state().ctx); }())

inline int device_from_env() { const char* e = std::getenv("TRGL_DEVICE"); return e ? std::atoi(e) : 0; }

// make sure a context matching the framebuffer exists and holds the host's current pixels / depths
inline bool bind(TGAImage& fb) {
    State& s = state();
    const int fb_bpp = image_bpp(fb);
    if (s.ctx && (s.w != fb.width() || s.h != fb.height() || s.bpp != fb_bpp)) {
        // one framebuffer at a time: what was batched or queued for the old one runs on ITS context, under its own Viewport, and the depths
        // come to the host copy as the reference's global holds them (the old image's pixels are not fetched: gl_flush(old) does that)
        (void)static_cast<const trgl_zbuffer_proxy&>(zbuffer).data();
        trgl_destroy(s.ctx); s.ctx = nullptr;
    }
    if (!s.ctx) {
        const int rc = trgl_create(device_from_env(), fb.width(), fb.height(), fb_bpp, &s.ctx);
        if (rc != TRGL_OK) { s.ctx = nullptr; return fail("trgl_create", rc, nullptr); }
        s.w = fb.width(); s.h = fb.height(); s.bpp = fb_bpp;
        // the user shaders, with the kinds they had on earlier contexts (a context that misses one is not kept: the next bind()
        // tries again with a new one)
        for (std::size_t i = 0; i < s.user.size(); ++i) {
            int kind = -1;
            bool ok = TRGL_SHIM_OK(trgl_register_shader_ex(s.ctx, s.user[i].source.c_str(), s.user[i].n_varyings, s.user[i].flags, &kind));
            if (ok && kind != TRGL_SHADER_USER_FIRST + int(i)) ok = fail("gl_register_shader: kinds out of order", TRGL_E_STATE, nullptr);
            if (!ok) { trgl_destroy(s.ctx); s.ctx = nullptr; return false; }
        }
        for (std::size_t i = 0; i < s.vertex.size(); ++i) {
            int vs = -1;
            bool ok = TRGL_SHIM_OK(trgl_register_vertex_shader(s.ctx, s.vertex[i].source.c_str(), s.vertex[i].n_varyings, &vs));
            if (ok && vs != int(i)) ok = fail("gl_register_vertex_shader: vertex kinds out of order", TRGL_E_STATE, nullptr);
            if (!ok) { trgl_destroy(s.ctx); s.ctx = nullptr; return false; }
        }
        if (!TRGL_SHIM_OK(trgl_write_framebuffer(s.ctx, fb.buffer()))) return false;
        s.zbuffer_dirty_on_host = true;
    }
    if (s.zbuffer_dirty_on_host) {
        std::vector<double>& hz = zbuffer.raw();
        if (hz.size() != std::size_t(s.w) * s.h) hz.assign(std::size_t(s.w) * s.h, std::numeric_limits<double>::infinity());
        if (!TRGL_SHIM_OK(trgl_write_zbuffer(s.ctx, hz.data()))) return false;
        s.zbuffer_dirty_on_host = false;
        s.zbuffer_stale_on_host = false;
    }
    return true;
}

// the clip attribute list of a kind: gl_clip_layout()'s, else n = -1, the kind's built-in layout (which a user kind with varyings
// does not have: the C ABI refuses the draw, reported through gl_last_error())
inline const trgl_clip_attr* clip_layout_of(int kind, int* n) {
    for (const State::ClipLayout& l : state().clip_layouts)
        if (l.kind == kind) { *n = int(l.attrs.size()); return l.attrs.data(); }
    *n = -1;
    return nullptr;
}

// hand the batched triangles to the device (on an error the batch is dropped: the call that met it reports false)
inline bool submit_batch() {
    State& s = state();
    if (!s.have_batch) return true;
    double vp[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = s.viewport_at_batch[r][c];
    bool ok = s.ctx && TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp));
    const double* vary = s.vary.empty() ? nullptr : s.vary.data();
    if (ok && s.clip_on) {                                      // (a change of plane ends the batch: the plane is the batch's)
        int n_attrs = -1;
        const trgl_clip_attr* attrs = clip_layout_of(s.kind, &n_attrs);
        ok = TRGL_SHIM_OK(trgl_draw_clipped(s.ctx, s.kind, &s.uniforms, s.clip_plane, attrs, n_attrs, s.clip.data(), vary, s.colors.data(),
                                            s.clip.size() / 12, TRGL_MEM_HOST));
    } else if (ok) {
        ok = TRGL_SHIM_OK(trgl_draw(s.ctx, s.kind, &s.uniforms, s.clip.data(), vary, s.colors.data(), s.clip.size() / 12, TRGL_MEM_HOST));
    }
    s.clip.clear(); s.vary.clear(); s.colors.clear();
    s.have_batch = false;
    s.zbuffer_stale_on_host = true;
    return ok;
}

inline int vary_count(int kind) {
    const State& s = state();
    if (kind >= TRGL_SHADER_USER_FIRST && kind - TRGL_SHADER_USER_FIRST < int(s.user.size())) return s.user[kind - TRGL_SHADER_USER_FIRST].n_varyings;
    return kind == TRGL_SHADER_GOURAUD ? TRGL_VARY_GOURAUD : (kind == TRGL_SHADER_PHONG || kind == TRGL_SHADER_EYE) ? TRGL_VARY_PHONG : 0;   // FLAT, CHECKER: 0
}
inline bool same_matrix(const mat<4, 4>& a, const mat<4, 4>& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

}  // namespace trgl_shim

// The first C-ABI error since the last gl_clear_error() (TRGL_OK = none) and its message.
inline int gl_last_error() { return trgl_shim::state().err; }
inline const char* gl_last_error_message() { return trgl_shim::state().err_msg.c_str(); }
inline void gl_clear_error() { trgl_shim::State& s = trgl_shim::state(); s.err = TRGL_OK; s.err_msg.clear(); }

// Clipping (include/trgl.h, trgl_clip_stage).  gl_clip_plane(&p): every triangle drawn from now on - rasterize(), gl_draw_indexed(),
// gl_draw_model() - is cut against the plane p in clip space before it is rasterized (inside: dot(p, v) >= 0; the near plane of
// init_perspective is (0, 0, 1, 1)); gl_clip_plane(nullptr) switches clipping off.  A change of plane ends the current batch.
// The counters then count the triangles that reach the rasterizer, and each clipped submission waits for the GPU once (trgl_draw_clipped).
inline void gl_clip_plane(const vec4* plane) {
    trgl_shim::State& s = trgl_shim::state();
    double p[4] = { 0, 0, 0, 0 };
    if (plane) for (int k = 0; k < 4; ++k) p[k] = (*plane)[k];
    if (s.clip_on == (plane != nullptr) && std::memcmp(p, s.clip_plane, sizeof(p)) == 0) return;
    trgl_shim::submit_batch();
    s.clip_on = plane != nullptr;
    std::memcpy(s.clip_plane, p, sizeof(p));
}
// Which varyings of a user kind belong to vertices: n attributes {offset, components}, each 3 * components doubles, vertex-major (the
// memory image of `vecC varying_x[3]`); the other varyings are per-triangle constants.  Built-in kinds have their layouts.  A user kind
// with varyings and no layout cannot be clipped: its draws fail through gl_last_error().
inline void gl_clip_layout(int kind, const trgl_clip_attr* attrs, int n) {
    trgl_shim::State& s = trgl_shim::state();
    trgl_shim::submit_batch();
    for (std::size_t i = 0; i < s.clip_layouts.size(); ++i)
        if (s.clip_layouts[i].kind == kind) { s.clip_layouts.erase(s.clip_layouts.begin() + i); break; }
    s.clip_layouts.push_back({ kind, std::vector<trgl_clip_attr>(attrs, attrs + (n > 0 ? n : 0)) });
}

// A user shader (include/trgl.h, "User shaders"): HIP C++ source defining trgl_fragment, with n_varyings doubles of varyings per
// triangle.  The source is compiled at once (a compile error is reported through gl_last_error(), with the compiler's log, and
// -1 comes back); the kind returned is what UserShader::kind takes, and it stays valid on every context the shim creates.
// may_discard: the source's trgl_fragment returns trgl_frag_out, the std::pair<bool, TGAColor> of IShader::fragment, and runs for
// every fragment that passes the z-test, in order (TRGL_SHADER_MAY_DISCARD).
// gl_register_shader_flags: the same with the whole TRGL_SHADER_* flag word, for a fragment() that blends: with
// TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST its in.dst is what framebuffer.get(x, y) holds when it runs, and with
// TRGL_SHADER_NO_DEPTH_WRITE it leaves the z-buffer alone.  Submission order is kept, nothing is sorted: opaque geometry first, then
// translucent geometry back to front.
inline int gl_register_shader_flags(const char* source, int n_varyings, std::uint32_t flags) {
    trgl_shim::State& s = trgl_shim::state();
    if (s.user.size() >= TRGL_MAX_USER_SHADERS) { trgl_shim::fail("gl_register_shader", TRGL_E_INVALID, nullptr); return -1; }
    std::string log(4096, '\0');
    const int rc = trgl_shader_compile_ex(source, n_varyings, flags, &log[0], log.size());
    if (rc != TRGL_OK) {
        if (s.err == TRGL_OK) { s.err = rc; s.err_msg = std::string("gl_register_shader: ") + log.c_str(); }
        return -1;
    }
    s.user.push_back({ source, n_varyings, flags });
    const int kind = TRGL_SHADER_USER_FIRST + int(s.user.size()) - 1;
    if (s.ctx) {
        trgl_shim::submit_batch();
        int k = -1;
        if (!TRGL_SHIM_OK(trgl_register_shader_ex(s.ctx, source, n_varyings, flags, &k))) { s.user.pop_back(); return -1; }
    }
    return kind;
}
inline int gl_register_shader(const char* source, int n_varyings, bool may_discard = false) {
    return gl_register_shader_flags(source, n_varyings, may_discard ? TRGL_SHADER_MAY_DISCARD : 0u);
}

// A user vertex shader (include/trgl.h, "User vertex shaders"): HIP C++ source defining trgl_vertex - the body of an
// IShader::vertex(face, nth) the device does not implement - that leaves n_varyings doubles of varyings per triangle.  Compiled at
// once, errors as for gl_register_shader; the number returned is what UserShader::vertex_kind takes (from 0, counted apart from the
// fragment kinds), valid on every context the shim creates.
inline int gl_register_vertex_shader(const char* source, int n_varyings) {
    trgl_shim::State& s = trgl_shim::state();
    if (s.vertex.size() >= TRGL_MAX_USER_VERTEX_SHADERS) { trgl_shim::fail("gl_register_vertex_shader", TRGL_E_INVALID, nullptr); return -1; }
    std::string log(4096, '\0');
    const int rc = trgl_vertex_shader_compile(source, n_varyings, &log[0], log.size());
    if (rc != TRGL_OK) {
        if (s.err == TRGL_OK) { s.err = rc; s.err_msg = std::string("gl_register_vertex_shader: ") + log.c_str(); }
        return -1;
    }
    s.vertex.push_back({ source, n_varyings });
    if (s.ctx) {
        trgl_shim::submit_batch();
        int vs = -1;
        if (!TRGL_SHIM_OK(trgl_register_vertex_shader(s.ctx, source, n_varyings, &vs))) { s.vertex.pop_back(); return -1; }
    }
    return int(s.vertex.size()) - 1;
}

// ---- our_gl.h:25-31 ------------------------------------------------------------------------------
inline void lookat(const vec3 eye, const vec3 center, const vec3 up) {            // our_gl.cpp:25-41
    vec3 z = normalized(eye - center), x = normalized(cross(up, z)), y = cross(z, x);
    ModelView = mat<4, 4>::identity();
    for (int i = 0; i < 3; ++i) { ModelView[0][i] = x[i]; ModelView[1][i] = y[i]; ModelView[2][i] = z[i]; }
    ModelView[0][3] = -dot(x, eye); ModelView[1][3] = -dot(y, eye); ModelView[2][3] = -dot(z, eye);
}
inline void init_perspective(double fov_deg, double aspect, double znear, double zfar) {   // our_gl.cpp:44-56
    double t = std::tan(fov_deg * M_PI / 180.0 / 2.0);
    Perspective = mat<4, 4>::identity();
    Perspective[0][0] = 1.0 / (aspect * t);
    Perspective[1][1] = 1.0 / t;
    Perspective[2][2] = (zfar + znear) / (znear - zfar);
    Perspective[2][3] = (2.0 * zfar * znear) / (znear - zfar);
    Perspective[3][2] = -1.0;
    Perspective[3][3] = 0.0;
}
inline void init_viewport(int x, int y, int w, int h) {                           // our_gl.cpp:59-69
    Viewport = mat<4, 4>::identity();
    Viewport[0][0] = w / 2.0; Viewport[1][1] = h / 2.0;
    Viewport[0][3] = x + w / 2.0; Viewport[1][3] = y + h / 2.0;
    Viewport[2][2] = 1.0; Viewport[2][3] = 0.0;
}
inline void init_zbuffer(int width, int height) {                                 // our_gl.cpp:72-74
    zbuffer.assign(std::size_t(width) * height, std::numeric_limits<double>::infinity());
}

inline void trgl_zbuffer_proxy::pull() const {
    trgl_shim::State& s = trgl_shim::state();
    if (!s.ctx) return;
    trgl_shim::submit_batch();                                  // triangles batched so far are drawn against the depths as they are now
    if (!s.zbuffer_stale_on_host || s.zbuffer_dirty_on_host) return;
    std::vector<double>& hz = const_cast<std::vector<double>&>(host_);
    hz.resize(std::size_t(s.w) * s.h);
    if (TRGL_SHIM_OK(trgl_read_zbuffer(s.ctx, hz.data()))) s.zbuffer_stale_on_host = false;
}
inline void trgl_zbuffer_proxy::touched() { trgl_shim::state().zbuffer_dirty_on_host = true; }
inline void trgl_zbuffer_proxy::assign(std::size_t n, double v) {
    trgl_shim::State& s = trgl_shim::state();
    if (s.ctx) { trgl_shim::submit_batch(); (void)TRGL_SHIM_OK(trgl_flush(s.ctx)); }   // earlier draws see the old depths
    host_.assign(n, v);
    s.zbuffer_dirty_on_host = true; s.zbuffer_stale_on_host = false;
}

// Tell the shim the host changed the depths behind the proxy's back (through zbuffer.raw()) or the framebuffer's pixels.
inline void gl_zbuffer_modified() {
    trgl_shim::State& s = trgl_shim::state();
    if (s.ctx) { trgl_shim::submit_batch(); (void)TRGL_SHIM_OK(trgl_flush(s.ctx)); }   // what was batched was drawn against the OLD depths
    s.zbuffer_dirty_on_host = true;
}
inline void gl_framebuffer_modified(TGAImage& fb) {
    trgl_shim::State& s = trgl_shim::state();
    if (!s.ctx) return;                                         // (the first bind() uploads the image as it is then)
    // an image of another size or bpp: the context's frame is not its size - bind() makes the context anew from the image's bytes
    if (s.w != fb.width() || s.h != fb.height() || s.bpp != trgl_shim::image_bpp(fb)) { (void)trgl_shim::bind(fb); return; }
    trgl_shim::submit_batch();
    (void)TRGL_SHIM_OK(trgl_write_framebuffer(s.ctx, fb.buffer()));
}

// Model textures live on the device: TGAImage::buffer() layout, one slot per map (include/trgl.h).
inline bool gl_upload_texture(TGAImage& framebuffer, int slot, const TGAImage& img) {
    if (!trgl_shim::bind(framebuffer)) return false;
    const bool ok = trgl_shim::submit_batch();
    return TRGL_SHIM_OK(trgl_upload_texture(trgl_shim::state().ctx, slot, trgl_shim::image_bytes(img), img.width(), img.height(), trgl_shim::image_bpp(img))) && ok;
}

// ---- our_gl.h:58 ---------------------------------------------------------------------------------
inline void rasterize(const Triangle& clip, const IShader& shader, TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    trgl_shader_desc d;
    if (!shader.describe(d)) {                                    // a programming error, not a run-time condition
        std::fprintf(stderr, "trgl: rasterize(): this IShader subclass has no device descriptor (describe()); "
                             "the fragment stage runs on the GPU and there is no CPU fallback\n");
        std::abort();
    }
    if (!bind(framebuffer)) return;                               // (reported through gl_last_error(); rasterize() is void, our_gl.h:58)
    const int K = vary_count(d.kind);
    if (K && !d.varyings) {                                       // (a UserShader whose varyings are not its K doubles)
        std::fprintf(stderr, "trgl: rasterize(): shader kind %d needs %d doubles of varyings per triangle\n", d.kind, K);
        std::abort();
    }
    if (s.have_batch && (s.kind != d.kind || std::memcmp(&s.uniforms, &d.uniforms, sizeof(trgl_uniforms)) != 0 ||
                         !same_matrix(s.viewport_at_batch, Viewport)))
        submit_batch();
    if (!s.have_batch) { s.have_batch = true; s.kind = d.kind; s.uniforms = d.uniforms; s.viewport_at_batch = Viewport; }
    static_assert(sizeof(Triangle) == 12 * sizeof(double), "Triangle must be 12 packed doubles");
    const double* cp = reinterpret_cast<const double*>(&clip[0]);
    s.clip.insert(s.clip.end(), cp, cp + 12);                   // the Triangle memory image (our_gl.h:55)
    if (K) s.vary.insert(s.vary.end(), d.varyings, d.varyings + K);
    s.colors.push_back(d.color);
    if (s.clip.size() >= std::size_t(12) * (TRGL_SHIM_BATCH_TRIS)) submit_batch();   // bound host memory: 1 Mi triangles per batch
}

// A whole face loop in one call (main.cpp:660-666, 692-698, 715-721):
//     for face: for v in 0..2: clip[v] = shader.vertex(face, v);  rasterize(clip, shader, framebuffer);
// The shader's describe() supplies kind + uniforms (ModelView at call time, lights, texture slots); the vertex stage
// (main.cpp:71-90 = 199-218: eye = ModelView*(p,1), normal_eye = ModelView*(n,0), clip = Perspective*eye) runs on the
// device over the indexed mesh.  `vertices`: nv rows of `stride` doubles starting with position[3], normal[3], uv[2]
// (the reference's Vertex, model.h:14-20, has stride 14); `indices`: 3 per face.
// A shader whose describe() names a user vertex shader (trgl_shader_desc::vertex_kind >= 0, UserShader::vertex_kind) has that
// shader's trgl_vertex run instead (trgl_draw_indexed_vs): then any kind - built-in ones included - with as many varyings as the
// vertex shader is drawn, every face with the descriptor's colour, and the vertex records are whatever trgl_vertex reads.
inline bool gl_draw_indexed(const IShader& shader, const double* vertices, int stride, std::size_t nv,
                            const unsigned int* indices, std::size_t nfaces, TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    const bool described = shader.describe(d);
    double vp[16], pj[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { vp[4 * r + c] = Viewport[r][c]; pj[4 * r + c] = Perspective[r][c]; }
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    if (described && d.vertex_kind >= 0) {
        if (d.vertex_kind >= int(s.vertex.size()) || s.vertex[d.vertex_kind].n_varyings != vary_count(d.kind)) {
            std::fprintf(stderr, "trgl: gl_draw_indexed(): vertex kind %d is not a registered vertex shader with the %d varyings of shader kind %d\n",
                         d.vertex_kind, vary_count(d.kind), d.kind);
            std::abort();
        }
        const std::vector<std::uint32_t> colors(nfaces, d.color);
        int n_attrs = -1;
        const trgl_clip_attr* attrs = clip_layout_of(d.kind, &n_attrs);
        ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) &&
             (s.clip_on ? TRGL_SHIM_OK(trgl_draw_indexed_vs_clipped(s.ctx, d.vertex_kind, d.kind, &d.uniforms, pj, s.clip_plane, attrs, n_attrs, vertices, stride, nv,
                                                                    reinterpret_cast<const std::uint32_t*>(indices), nfaces, colors.data(), TRGL_MEM_HOST))
                        : TRGL_SHIM_OK(trgl_draw_indexed_vs(s.ctx, d.vertex_kind, d.kind, &d.uniforms, pj, vertices, stride, nv,
                                                            reinterpret_cast<const std::uint32_t*>(indices), nfaces, colors.data(), TRGL_MEM_HOST))) && ok;
        s.zbuffer_stale_on_host = true;
        return ok;
    }
    // (a user kind registered with K = 24 takes the varyings the device vertex stage writes: the PHONG layout)
    if (!described || (d.kind != TRGL_SHADER_PHONG && d.kind != TRGL_SHADER_EYE &&
                                !(d.kind >= TRGL_SHADER_USER_FIRST && vary_count(d.kind) == TRGL_VARY_PHONG))) {
        std::fprintf(stderr, "trgl: gl_draw_indexed(): needs a PHONG or EYE shader, or a user shader with 24 varyings, with a device descriptor\n");
        std::abort();
    }
    int n_attrs = -1;
    const trgl_clip_attr* attrs = d.kind >= TRGL_SHADER_USER_FIRST ? clip_layout_of(d.kind, &n_attrs) : nullptr;
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) &&
         (s.clip_on ? TRGL_SHIM_OK(trgl_draw_indexed_vs_clipped(s.ctx, -1, d.kind, &d.uniforms, pj, s.clip_plane, attrs, n_attrs, vertices, stride, nv,
                                                                reinterpret_cast<const std::uint32_t*>(indices), nfaces, nullptr, TRGL_MEM_HOST))
                    : TRGL_SHIM_OK(trgl_draw_indexed(s.ctx, d.kind, &d.uniforms, pj, vertices, stride, nv,
                                                     reinterpret_cast<const std::uint32_t*>(indices), nfaces, TRGL_MEM_HOST))) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}
// ... for a model that keeps `vertices` (records of packed doubles) and `indices` as the reference's Model does (model.h:114-115)
template <class ModelT> inline bool gl_draw_model(const ModelT& model, const IShader& shader, TGAImage& framebuffer) {
    using V = typename std::decay<decltype(model.vertices[0])>::type;
    static_assert(sizeof(V) % sizeof(double) == 0, "vertex records must be packed doubles");
    return gl_draw_indexed(shader, reinterpret_cast<const double*>(model.vertices.data()), int(sizeof(V) / sizeof(double)),
                    model.vertices.size(), model.indices.data(), model.indices.size() / 3, framebuffer);
}

// The loop over models of main.cpp:647-736 for ONE mesh under many model matrices, in one call (include/trgl.h, trgl_draw_instanced):
//     for m in models: if (visible(m)) { ModelView = ModelView * m.matrix; <the face loop of gl_draw_indexed> }
// The shader's describe() is taken ONCE, under the ModelView of the call: the vertex stage of instance i runs under ModelView *
// model_matrices[i] (geometry.h:196-205), the fragment stage of every instance under the ModelView and lights of that one descriptor -
// the reference's loop with the shader constructed once, in front of it.  codes: one byte per matrix, drawn when bit 0 is set - what
// gl_occlusion_test returns plugs in as it is; null: every instance.  A shader with a user vertex shader (vertex_kind >= 0) receives
// the matrix as in.inst (16 doubles, row-major) and the instance's number as in.instance, and every face gets the descriptor's colour.
// Clipping (gl_clip_plane) does not apply to instanced draws.
namespace trgl_shim {
inline bool draw_instanced(const IShader& shader, const double* vertices, int stride, std::size_t nv, const unsigned int* indices, std::size_t nfaces,
                           const double* matrices, int matrix_stride, std::size_t n, const std::uint8_t* codes, int instance_mem_kind,
                           TGAImage& framebuffer, const std::uint32_t* order = nullptr, std::size_t n_order = 0, int order_mem_kind = TRGL_MEM_HOST) {
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: gl_draw_instanced(): needs a shader with a device descriptor\n");
        std::abort();
    }
    if (s.clip_on) return fail("gl_draw_instanced: a clip plane is set, and instanced draws are not clipped", TRGL_E_UNSUPPORTED, nullptr);
    double vp[16], pj[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { vp[4 * r + c] = Viewport[r][c]; pj[4 * r + c] = Perspective[r][c]; }
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    const std::vector<std::uint32_t> colors(d.vertex_kind >= 0 ? nfaces : 0, d.color);
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) && ok;
    if (!order)                                                 // (an empty list is no list: the call the shim made before there were lists)
        ok = TRGL_SHIM_OK(trgl_draw_instanced(s.ctx, d.vertex_kind >= 0 ? d.vertex_kind : -1, d.kind, &d.uniforms, pj, vertices, stride, nv,
                                              reinterpret_cast<const std::uint32_t*>(indices), nfaces, d.vertex_kind >= 0 ? colors.data() : nullptr, TRGL_MEM_HOST,
                                              matrices, matrix_stride, n, nullptr, codes, instance_mem_kind)) && ok;
    else
        ok = TRGL_SHIM_OK(trgl_draw_instanced_ordered(s.ctx, d.vertex_kind >= 0 ? d.vertex_kind : -1, d.kind, &d.uniforms, pj, vertices, stride, nv,
                                                      reinterpret_cast<const std::uint32_t*>(indices), nfaces, d.vertex_kind >= 0 ? colors.data() : nullptr,
                                                      TRGL_MEM_HOST, matrices, matrix_stride, n, nullptr, codes, instance_mem_kind,
                                                      order, n_order, order_mem_kind)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}
}  // namespace trgl_shim
inline bool gl_draw_instanced(const IShader& shader, const double* vertices, int stride, std::size_t nv, const unsigned int* indices, std::size_t nfaces,
                              const std::vector<mat<4, 4>>& model_matrices, TGAImage& framebuffer, const std::uint8_t* codes = nullptr) {
    std::vector<double> m(model_matrices.size() * 16);
    for (std::size_t i = 0; i < model_matrices.size(); ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[16 * i + 4 * r + c] = model_matrices[i][r][c];
    return trgl_shim::draw_instanced(shader, vertices, stride, nv, indices, nfaces, m.data(), 16, model_matrices.size(), codes, TRGL_MEM_HOST, framebuffer);
}
// ... with the instances in DEVICE memory: `matrices` (n records of matrix_stride >= 16 doubles, the matrix first, 8-byte aligned) and
// `codes` (n bytes - as trgl_occlusion_boxes leaves them with TRGL_MEM_DEVICE - or null).  One memory kind covers both arrays in the C
// ABI, so codes that stay on the device ask for matrices that live there too.  The call waits once, for the count of drawn instances.
struct gl_device_instances { const double* matrices; int matrix_stride; std::size_t count; const std::uint8_t* codes; };
inline bool gl_draw_instanced(const IShader& shader, const double* vertices, int stride, std::size_t nv, const unsigned int* indices, std::size_t nfaces,
                              const gl_device_instances& instances, TGAImage& framebuffer) {
    return trgl_shim::draw_instanced(shader, vertices, stride, nv, indices, nfaces, instances.matrices, instances.matrix_stride, instances.count,
                                     instances.codes, TRGL_MEM_DEVICE, framebuffer);
}

// Depth-ordered instanced draws (include/trgl.h, trgl_instance_depths / trgl_depth_order / trgl_draw_instanced_ordered): what a caller
// of the reference does by sorting its models on the host before the loop of main.cpp:647-736.
// gl_instance_depths: the view-space z of `point` (a point of the mesh in model space) under ModelView * model_matrices[i], one double per
// matrix.  gl_depth_order: the order to draw such depths in - farthest first (translucent shaders), or with front_to_back nearest first
// (fewer fragment() calls of an opaque one); equal depths keep their order either way.  Both run on the host and need no context; a call
// that fails (gl_last_error()) answers zeros / the order 0 .. n-1.
inline std::vector<double> gl_instance_depths(const std::vector<mat<4, 4>>& model_matrices, const vec3& point) {
    std::vector<double> m(model_matrices.size() * 16), depths(model_matrices.size(), 0.0);
    for (std::size_t i = 0; i < model_matrices.size(); ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[16 * i + 4 * r + c] = model_matrices[i][r][c];
    double mv[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) mv[4 * r + c] = ModelView[r][c];
    const double p[3] = { point.x, point.y, point.z };
    const int rc = trgl_instance_depths(nullptr, mv, p, m.data(), 16, m.size() / 16, TRGL_MEM_HOST, depths.data());
    if (rc != TRGL_OK) trgl_shim::fail("gl_instance_depths", rc, nullptr);
    return depths;
}
inline std::vector<std::uint32_t> gl_depth_order(const std::vector<double>& depths, bool front_to_back = false) {
    std::vector<std::uint32_t> order(depths.size());
    for (std::size_t i = 0; i < order.size(); ++i) order[i] = std::uint32_t(i);
    const int rc = trgl_depth_order(nullptr, depths.data(), depths.size(), front_to_back ? TRGL_ORDER_FRONT_TO_BACK : TRGL_ORDER_BACK_TO_FRONT,
                                    TRGL_MEM_HOST, order.data());
    if (rc != TRGL_OK) trgl_shim::fail("gl_depth_order", rc, nullptr);
    return order;
}
// gl_draw_instanced with the matrices visited in the order the list names them: model_matrices[order[0]] first.  A matrix named twice is
// drawn twice, one that is not named is not drawn; an entry that is no matrix fails the call (TRGL_E_INVALID).  A shader with a user
// vertex shader still sees the matrix's own number as in.instance.  A set clip plane is TRGL_E_UNSUPPORTED, as for gl_draw_instanced.
inline bool gl_draw_instanced_ordered(const IShader& shader, const double* vertices, int stride, std::size_t nv, const unsigned int* indices,
                                      std::size_t nfaces, const std::vector<mat<4, 4>>& model_matrices, const std::vector<std::uint32_t>& order,
                                      TGAImage& framebuffer, const std::uint8_t* codes = nullptr) {
    std::vector<double> m(model_matrices.size() * 16);
    for (std::size_t i = 0; i < model_matrices.size(); ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[16 * i + 4 * r + c] = model_matrices[i][r][c];
    if (order.empty()) return true;                             // (no position to visit: nothing is drawn)
    return trgl_shim::draw_instanced(shader, vertices, stride, nv, indices, nfaces, m.data(), 16, model_matrices.size(), codes, TRGL_MEM_HOST, framebuffer,
                                     order.data(), order.size(), TRGL_MEM_HOST);
}
// ... with the instances and the list in DEVICE memory (order: n_order uint32, 4-byte aligned - as trgl_depth_order leaves them with
// TRGL_MEM_DEVICE; entries that are no instance are skipped).  The call waits once, for the count of drawn instances.
inline bool gl_draw_instanced_ordered(const IShader& shader, const double* vertices, int stride, std::size_t nv, const unsigned int* indices,
                                      std::size_t nfaces, const gl_device_instances& instances, const std::uint32_t* order, std::size_t n_order,
                                      TGAImage& framebuffer) {
    if (n_order == 0) return true;
    return trgl_shim::draw_instanced(shader, vertices, stride, nv, indices, nfaces, instances.matrices, instances.matrix_stride, instances.count,
                                     instances.codes, TRGL_MEM_DEVICE, framebuffer, order, n_order, TRGL_MEM_DEVICE);
}

// Depth-ordered triangle draws (include/trgl.h, trgl_triangle_depths / trgl_draw_ordered): what a caller of the reference does by
// sorting the triangles of a translucent mesh on the host before its rasterize() loop.
// gl_triangle_depths: one depth per group of `group` consecutive triangles, from the clip w of the group's vertices (mode: one of
// TRGL_TRI_DEPTH_*), ascending the way gl_depth_order expects: pass the result to it as it is.  Runs on the host and needs no context;
// a call that fails (gl_last_error()) answers zeros.
inline std::vector<double> gl_triangle_depths(const Triangle* clip, std::size_t n, std::uint32_t group = 1, int mode = TRGL_TRI_DEPTH_CENTROID) {
    static_assert(sizeof(Triangle) == 12 * sizeof(double), "Triangle must be 12 packed doubles");
    std::vector<double> depths(group ? n / group : 0, 0.0);
    const int rc = trgl_triangle_depths(nullptr, reinterpret_cast<const double*>(clip), n, group, mode, TRGL_MEM_HOST, depths.data());
    if (rc != TRGL_OK) trgl_shim::fail("gl_triangle_depths", rc, nullptr);
    return depths;
}
// gl_draw_ordered: `for p in order: for t in 0 .. group-1: rasterize(clip[order[p] * group + t], shader, framebuffer)` over the n triangles
// at clip (each the Triangle memory image, our_gl.h:55), in one call.  The
// shader's describe() is taken once: every triangle gets its kind, uniforms, colour and varyings.  A group named twice is drawn twice,
// one that is not named is not drawn; an entry that is no group fails the call (TRGL_E_INVALID).  A set clip plane is
// TRGL_E_UNSUPPORTED: ordered draws are not clipped.
inline bool gl_draw_ordered(const Triangle* clip, std::size_t n, const IShader& shader, const std::vector<std::uint32_t>& order,
                            TGAImage& framebuffer, std::uint32_t group = 1) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: gl_draw_ordered(): needs a shader with a device descriptor\n");
        std::abort();
    }
    if (s.clip_on) return fail("gl_draw_ordered: a clip plane is set, and ordered draws are not clipped", TRGL_E_UNSUPPORTED, nullptr);
    if (order.empty()) return ok;                               // (no position to visit: nothing is drawn)
    const int K = vary_count(d.kind);
    if (K && !d.varyings) {
        std::fprintf(stderr, "trgl: gl_draw_ordered(): shader kind %d needs %d doubles of varyings per triangle\n", d.kind, K);
        std::abort();
    }
    std::vector<double> vary;
    for (std::size_t i = 0; K && i < n; ++i) vary.insert(vary.end(), d.varyings, d.varyings + K);
    const std::vector<std::uint32_t> colors(n, d.color);
    double vp[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = Viewport[r][c];
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) && ok;
    ok = TRGL_SHIM_OK(trgl_draw_ordered(s.ctx, d.kind, &d.uniforms, reinterpret_cast<const double*>(clip), K ? vary.data() : nullptr, colors.data(), n,
                                        TRGL_MEM_HOST, order.data(), order.size(), group, TRGL_MEM_HOST)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}

// Point sprites and wide lines (include/trgl.h, trgl_sprite_stage / trgl_line_stage): a point or a segment becomes the two triangles of a
// quad under the globals ModelView, Perspective and Viewport as they stand at the call - what a caller of the reference would build by
// hand in front of its rasterize() loop.
// gl_sprite_params: size in eye-space units (TRGL_SPRITE_VIEW) or in pixels of the global Viewport (TRGL_SPRITE_SCREEN); size_offset >= 0
// takes each point's size from that column of its row instead.  gl_line_params: width in pixels of the global Viewport; the segment is
// cut where its clip w falls below w_min (init_perspective's znear).
inline trgl_sprite_params gl_sprite_params(double size, int mode = TRGL_SPRITE_VIEW, int size_offset = -1, int attr_offset = 0, int n_attr = 0) {
    trgl_sprite_params p{};
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { p.model_view[4 * r + c] = ModelView[r][c]; p.projection[4 * r + c] = Perspective[r][c]; }
    p.size = size; p.scale[0] = 1.0 / Viewport[0][0]; p.scale[1] = 1.0 / Viewport[1][1];
    p.mode = mode; p.size_offset = size_offset; p.attr_offset = attr_offset; p.n_attr = n_attr;
    return p;
}
inline trgl_line_params gl_line_params(double width, double w_min) {
    trgl_line_params p{};
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { p.model_view[4 * r + c] = ModelView[r][c]; p.projection[4 * r + c] = Perspective[r][c]; }
    p.width = width; p.half_extent[0] = Viewport[0][0]; p.half_extent[1] = Viewport[1][1]; p.w_min = w_min;
    return p;
}
// The stages alone, on the host, no context needed: clip_out receives 2 n Triangles as 12 doubles each (reinterpret_cast<const Triangle*>
// (clip_out.data()) is what rasterize() takes), vary_out 2 n rows of 6 + n_attr (lines: 6) varyings; a call that fails (gl_last_error())
// leaves the vectors empty.
inline bool gl_sprite_stage(const trgl_sprite_params& params, const double* points, int stride, std::size_t n,
                            std::vector<double>& clip_out, std::vector<double>& vary_out) {
    static_assert(sizeof(Triangle) == 12 * sizeof(double), "Triangle must be 12 packed doubles");
    clip_out.assign(2 * n * 12, 0.0);
    vary_out.assign(2 * n * std::size_t(6 + (params.n_attr > 0 ? params.n_attr : 0)), 0.0);
    const int rc = trgl_sprite_stage(nullptr, &params, points, stride, nullptr, n, TRGL_MEM_HOST, clip_out.data(), vary_out.data(), nullptr);
    if (rc != TRGL_OK) { clip_out.clear(); vary_out.clear(); return trgl_shim::fail("gl_sprite_stage", rc, nullptr); }
    return true;
}
inline bool gl_line_stage(const trgl_line_params& params, const double* points, int stride, std::size_t n_points, const std::uint32_t* indices,
                          std::size_t n_segments, std::vector<double>& clip_out, std::vector<double>& vary_out) {
    clip_out.assign(2 * n_segments * 12, 0.0);
    vary_out.assign(2 * n_segments * 6, 0.0);
    const int rc = trgl_line_stage(nullptr, &params, points, stride, n_points, indices, nullptr, n_segments, TRGL_MEM_HOST,
                                   clip_out.data(), vary_out.data(), nullptr);
    if (rc != TRGL_OK) { clip_out.clear(); vary_out.clear(); return trgl_shim::fail("gl_line_stage", rc, nullptr); }
    return true;
}
// gl_draw_sprites / gl_draw_lines: the stage and `for t in 0 .. 2 n - 1: rasterize(quad triangle t, shader, framebuffer)` in one call.
// The shader's describe() is taken once: its kind takes no varyings, or the 6 + n_attr (lines: 6) that the stage makes; colors: one per
// point or segment, or null for the descriptor's colour.  A set clip plane is TRGL_E_UNSUPPORTED: these draws are not clipped.
namespace trgl_shim {
inline bool draw_quads(const char* who, const IShader& shader, TGAImage& framebuffer, std::size_t n, const std::uint32_t* colors,
                       const trgl_sprite_params* sprites, const trgl_line_params* lines, const double* points, int stride, std::size_t n_points,
                       const std::uint32_t* indices) {
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: %s(): needs a shader with a device descriptor\n", who);
        std::abort();
    }
    if (s.clip_on) return fail(who, TRGL_E_UNSUPPORTED, nullptr);
    std::vector<std::uint32_t> own;
    if (!colors) { own.assign(n, d.color); colors = own.data(); }
    double vp[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = Viewport[r][c];
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) && ok;
    ok = TRGL_SHIM_OK(sprites ? trgl_draw_sprites(s.ctx, d.kind, &d.uniforms, sprites, points, stride, colors, n, TRGL_MEM_HOST)
                              : trgl_draw_lines(s.ctx, d.kind, &d.uniforms, lines, points, stride, n_points, indices, colors, n, TRGL_MEM_HOST)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}
}  // namespace trgl_shim
inline bool gl_draw_sprites(const trgl_sprite_params& params, const double* points, int stride, std::size_t n, const std::uint32_t* colors,
                            const IShader& shader, TGAImage& framebuffer) {
    return trgl_shim::draw_quads("gl_draw_sprites", shader, framebuffer, n, colors, &params, nullptr, points, stride, n, nullptr);
}
inline bool gl_draw_lines(const trgl_line_params& params, const double* points, int stride, std::size_t n_points, const std::uint32_t* indices,
                          std::size_t n_segments, const std::uint32_t* colors, const IShader& shader, TGAImage& framebuffer) {
    return trgl_shim::draw_quads("gl_draw_lines", shader, framebuffer, n_segments, colors, nullptr, &params, points, stride, n_points, indices);
}

// Skeletal animation (include/trgl.h, trgl_skin_stage / trgl_pose_palette / trgl_draw_skinned): the bones and weights that Assimp
// delivers and the reference's Model::processMesh drops.  joints / weights: n_influences per vertex; a palette: one mat<4,4> per joint.
inline trgl_skin_params gl_skin_params(int vertex_stride, int n_influences, std::size_t n_joints, std::uint32_t flags = TRGL_SKIN_NORMAL) {
    trgl_skin_params p{};
    p.vertex_stride = vertex_stride; p.n_influences = n_influences; p.n_joints = std::uint32_t(n_joints); p.flags = flags; p.n_poses = 1;
    return p;
}
// palette_j = world_j * inverse_bind_j with world_j = world_parent * local_j (parents[j]: -1, or a joint below j), on the host, no
// context needed; inverse_bind may be empty (palette = world).  A call that fails (gl_last_error()) leaves `palette` empty.
inline bool gl_pose_palette(const std::vector<std::int32_t>& parents, const std::vector<mat<4, 4>>& inverse_bind, const std::vector<mat<4, 4>>& local,
                            std::vector<mat<4, 4>>& palette) {
    static_assert(sizeof(mat<4, 4>) == 16 * sizeof(double), "mat<4,4> must be 16 packed doubles");
    palette.assign(parents.size(), mat<4, 4>());
    const int rc = (local.size() != parents.size() || (!inverse_bind.empty() && inverse_bind.size() != parents.size())) ? TRGL_E_INVALID
        : trgl_pose_palette(nullptr, parents.data(), inverse_bind.empty() ? nullptr : reinterpret_cast<const double*>(inverse_bind.data()),
                            std::uint32_t(parents.size()), reinterpret_cast<const double*>(local.data()), 0, 1, TRGL_MEM_HOST,
                            reinterpret_cast<double*>(palette.data()), 0);
    if (rc != TRGL_OK) { palette.clear(); return trgl_shim::fail("gl_pose_palette", rc, nullptr); }
    return true;
}
// The skinned copy of `vertices` (nv records of params.vertex_stride doubles) under one palette, on the host, no context needed; a call
// that fails leaves `out` empty.
inline bool gl_skin_stage(trgl_skin_params params, const double* vertices, std::size_t nv, const std::uint16_t* joints, const double* weights,
                          const std::vector<mat<4, 4>>& palette, std::vector<double>& out) {
    params.n_joints = std::uint32_t(palette.size()); params.n_poses = 1; params.palette_stride = 0;
    out.assign(nv * std::size_t(params.vertex_stride > 0 ? params.vertex_stride : 0), 0.0);
    const int rc = trgl_skin_stage(nullptr, &params, vertices, nv, joints, weights, reinterpret_cast<const double*>(palette.data()), TRGL_MEM_HOST, out.data());
    if (rc != TRGL_OK) { out.clear(); return trgl_shim::fail("gl_skin_stage", rc, nullptr); }
    return true;
}
// gl_skin_stage and gl_draw_indexed of its output in one call (trgl_draw_skinned): the shader's describe() is taken as gl_draw_indexed
// takes it.  A set clip plane is TRGL_E_UNSUPPORTED: this draw is not clipped.
inline bool gl_draw_skinned(const IShader& shader, trgl_skin_params params, const double* vertices, std::size_t nv, const std::uint16_t* joints,
                            const double* weights, const std::vector<mat<4, 4>>& palette, const unsigned int* indices, std::size_t nfaces,
                            TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: gl_draw_skinned(): needs a shader with a device descriptor\n");
        std::abort();
    }
    if (s.clip_on) return fail("gl_draw_skinned", TRGL_E_UNSUPPORTED, nullptr);
    params.n_joints = std::uint32_t(palette.size()); params.n_poses = 1; params.palette_stride = 0;
    double vp[16], pj[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { vp[4 * r + c] = Viewport[r][c]; pj[4 * r + c] = Perspective[r][c]; }
    const bool user_vs = d.vertex_kind >= 0;
    const std::vector<std::uint32_t> colors(user_vs ? nfaces : 0, d.color);
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) &&
         TRGL_SHIM_OK(trgl_draw_skinned(s.ctx, user_vs ? d.vertex_kind : -1, d.kind, &d.uniforms, pj, &params, vertices, nv, joints, weights,
                                        reinterpret_cast<const double*>(palette.data()), reinterpret_cast<const std::uint32_t*>(indices), nfaces,
                                        user_vs ? colors.data() : nullptr, TRGL_MEM_HOST)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}

// Mesh edges (include/trgl.h, trgl_mesh_edges / trgl_edge_select / trgl_draw_outline): the distinct edges of an indexed mesh, their
// classes under an eye in model space - boundary, silhouette, crease - and the selected ones as wide lines.
// gl_edge_params: eye (x, y, z, w) in model space, w = 1 a camera position, w = 0 a direction; class_color: ANY, BOUNDARY, SILHOUETTE, CREASE.
inline trgl_edge_params gl_edge_params(const double eye[4], double crease_cos, std::uint32_t select, const std::uint32_t class_color[4]) {
    trgl_edge_params p{};
    for (int a = 0; a < 4; ++a) { p.eye[a] = eye[a]; p.class_color[a] = class_color[a]; }
    p.crease_cos = crease_cos; p.select = select;
    return p;
}
// The edge records {lo, hi, f0, f1} of nfaces faces, on the host, no context needed: `edges` receives exactly the edges, four words
// each (once per mesh; the records do not depend on the vertices).  A call that fails (gl_last_error()) leaves it empty.
inline bool gl_mesh_edges(const unsigned int* indices, std::size_t nfaces, std::size_t nvertices, std::vector<std::uint32_t>& edges) {
    edges.assign(12 * nfaces, 0u);
    std::uint64_t n = 0;
    const int rc = trgl_mesh_edges(nullptr, reinterpret_cast<const std::uint32_t*>(indices), nfaces, nvertices, TRGL_MEM_HOST, edges.data(), &n);
    if (rc != TRGL_OK) { edges.clear(); return trgl_shim::fail("gl_mesh_edges", rc, nullptr); }
    edges.resize(4 * std::size_t(n));
    return true;
}
// The classes of those edges under `params`: codes one byte per edge; segments (index pairs into the vertices) and colors hold the
// selected edges only, in edge order - what gl_draw_lines takes.  A call that fails leaves the vectors empty.
inline bool gl_edge_select(trgl_edge_params params, const double* vertices, int stride, std::size_t nvertices, const unsigned int* indices,
                           std::size_t nfaces, const std::vector<std::uint32_t>& edges, std::vector<std::uint8_t>& codes,
                           std::vector<std::uint32_t>& segments, std::vector<std::uint32_t>& colors) {
    const std::size_t n = edges.size() / 4;
    codes.assign(n, 0); segments.assign(2 * n, 0u); colors.assign(n, 0u);
    params.compact = 1;
    std::uint64_t selected = 0;
    const int rc = trgl_edge_select(nullptr, &params, vertices, stride, nvertices, reinterpret_cast<const std::uint32_t*>(indices), nfaces, edges.data(), n,
                                    TRGL_MEM_HOST, codes.data(), segments.data(), colors.data(), &selected);
    if (rc != TRGL_OK) { codes.clear(); segments.clear(); colors.clear(); return trgl_shim::fail("gl_edge_select", rc, nullptr); }
    segments.resize(2 * std::size_t(selected)); colors.resize(std::size_t(selected));
    return true;
}
// gl_edge_select and gl_draw_lines of the selected edges in their class colours in one call (trgl_draw_outline), under the globals
// ModelView, Perspective and Viewport; width in pixels, w_min as for gl_line_params.  The lines lie in the surface they outline: a
// caller who wants them in front draws under a Perspective whose depth row is slightly nearer.  The shader's kind takes no varyings
// or the line stage's 6.  A set clip plane is TRGL_E_UNSUPPORTED: this draw is not clipped.
inline bool gl_draw_outline(const trgl_edge_params& params, double width, double w_min, const double* vertices, int stride, std::size_t nvertices,
                            const unsigned int* indices, std::size_t nfaces, const std::vector<std::uint32_t>& edges, const IShader& shader,
                            TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: gl_draw_outline(): needs a shader with a device descriptor\n");
        std::abort();
    }
    if (s.clip_on) return fail("gl_draw_outline", TRGL_E_UNSUPPORTED, nullptr);
    const trgl_line_params lines = gl_line_params(width, w_min);
    double vp[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = Viewport[r][c];
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) &&
         TRGL_SHIM_OK(trgl_draw_outline(s.ctx, d.kind, &d.uniforms, &lines, &params, vertices, stride, nvertices,
                                        reinterpret_cast<const std::uint32_t*>(indices), nfaces, edges.data(), edges.size() / 4, TRGL_MEM_HOST)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}

// Mesh subdivision (include/trgl.h, trgl_subdiv_topology / trgl_subdiv_vertices / trgl_draw_subdivided): one level of Loop or linear
// refinement of an indexed mesh, on the host, no context needed.  Where Model keeps `vertices` (records of `stride` doubles) and
// `indices`: gl_mesh_edges(indices) once, gl_subdiv_topology once - refined_indices replaces the index vector, 4 faces per face -, then
// gl_subdiv_vertices per pose, whose output replaces the vertex vector: nvertices + edges.size() / 4 records of the same stride.
// A second level is the same three calls on the refined mesh.  Normals are not part of the rule: smooth = 3 and the mesh-normal call.
inline trgl_subdiv_params gl_subdiv_params(int vertex_stride, std::uint32_t mode = TRGL_SUBDIV_LOOP, int smooth = 3) {
    trgl_subdiv_params p{};
    p.vertex_stride = vertex_stride; p.smooth = smooth; p.mode = mode;
    return p;
}
// `edges`: what gl_mesh_edges left for these indices.  A call that fails (gl_last_error()) leaves the vectors empty.
inline bool gl_subdiv_topology(const unsigned int* indices, std::size_t nfaces, std::size_t nvertices, const std::vector<std::uint32_t>& edges,
                               std::vector<unsigned int>& refined_indices, std::vector<std::uint32_t>& stencils) {
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    const std::size_t n = edges.size() / 4;
    refined_indices.assign(12 * nfaces, 0u); stencils.assign(std::size_t(trgl_subdiv_stencil_words(nvertices, n)), 0u);
    const int rc = trgl_subdiv_topology(nullptr, reinterpret_cast<const std::uint32_t*>(indices), nfaces, nvertices, edges.data(), n, TRGL_MEM_HOST,
                                        reinterpret_cast<std::uint32_t*>(refined_indices.data()), stencils.data());
    if (rc != TRGL_OK) { refined_indices.clear(); stencils.clear(); return trgl_shim::fail("gl_subdiv_topology", rc, nullptr); }
    return true;
}
// nedges: edges.size() / 4 of the gl_subdiv_topology call that made `stencils`
inline bool gl_subdiv_vertices(const trgl_subdiv_params& params, const double* vertices, std::size_t nvertices, const std::vector<std::uint32_t>& stencils,
                               std::size_t nedges, std::vector<double>& out) {
    out.assign((nvertices + nedges) * std::size_t(params.vertex_stride > 0 ? params.vertex_stride : 0), 0.0);
    const int rc = trgl_subdiv_vertices(nullptr, &params, vertices, nvertices, stencils.data(), nedges, TRGL_MEM_HOST, out.data());
    if (rc != TRGL_OK) { out.clear(); return trgl_shim::fail("gl_subdiv_vertices", rc, nullptr); }
    return true;
}
// gl_subdiv_vertices and gl_draw_indexed of its output with the refined indices in one call (trgl_draw_subdivided): the shader's
// describe() is taken as gl_draw_indexed takes it.  A set clip plane is TRGL_E_UNSUPPORTED: this draw is not clipped.
inline bool gl_draw_subdivided(const IShader& shader, const trgl_subdiv_params& params, const double* vertices, std::size_t nvertices,
                               const std::vector<std::uint32_t>& stencils, std::size_t nedges, const unsigned int* refined_indices,
                               std::size_t nrefined, TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    bool ok = submit_batch();                                   // earlier rasterize() calls come first
    trgl_shader_desc d;
    if (!shader.describe(d)) {
        std::fprintf(stderr, "trgl: gl_draw_subdivided(): needs a shader with a device descriptor\n");
        std::abort();
    }
    if (s.clip_on) return fail("gl_draw_subdivided", TRGL_E_UNSUPPORTED, nullptr);
    double vp[16], pj[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { vp[4 * r + c] = Viewport[r][c]; pj[4 * r + c] = Perspective[r][c]; }
    const bool user_vs = d.vertex_kind >= 0;
    const std::vector<std::uint32_t> colors(user_vs ? nrefined : 0, d.color);
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) &&
         TRGL_SHIM_OK(trgl_draw_subdivided(s.ctx, user_vs ? d.vertex_kind : -1, d.kind, &d.uniforms, pj, &params, vertices, nvertices, stencils.data(),
                                           nedges, reinterpret_cast<const std::uint32_t*>(refined_indices), nrefined,
                                           user_vs ? colors.data() : nullptr, TRGL_MEM_HOST)) && ok;
    s.zbuffer_stale_on_host = true;
    return ok;
}

// Mesh welding (include/trgl.h, trgl_mesh_weld): what stands where Model asked Assimp for aiProcess_JoinIdenticalVertices - on the host,
// no context needed.  The vertices (records of `stride` doubles) whose key - key_count doubles from key_offset on; cell > 0: their grid
// cells - is identical become one: `vertices` shrinks to the distinct records in their first order, every entry of `indices` (3 per
// face; may be empty for a soup) is renumbered, and remap[v] is the new number of old vertex v - what gathers arrays kept beside the
// records.  Faces are kept, degenerate ones included.  A call that fails (gl_last_error()) leaves the three vectors as they were.
inline trgl_weld_params gl_weld_params(int vertex_stride, int key_offset = 0, int key_count = 3, double cell = 0.0) {
    trgl_weld_params p{};
    p.vertex_stride = vertex_stride; p.key_offset = key_offset; p.key_count = key_count; p.cell = cell;
    return p;
}
inline bool gl_mesh_weld(const trgl_weld_params& params, std::vector<double>& vertices, std::vector<unsigned int>& indices, std::vector<std::uint32_t>& remap) {
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    const std::size_t stride = std::size_t(params.vertex_stride > 0 ? params.vertex_stride : 1), n = vertices.size() / stride;
    std::vector<double> welded(vertices.size());
    std::vector<unsigned int> renumbered(indices.size());
    std::vector<std::uint32_t> map(n);
    std::uint64_t unique = 0;
    const int rc = trgl_mesh_weld(nullptr, &params, vertices.data(), n, indices.empty() ? nullptr : reinterpret_cast<const std::uint32_t*>(indices.data()),
                                  indices.size() / 3, TRGL_MEM_HOST, map.data(), nullptr, welded.data(),
                                  indices.empty() ? nullptr : reinterpret_cast<std::uint32_t*>(renumbered.data()), &unique);
    if (rc != TRGL_OK) return trgl_shim::fail("gl_mesh_weld", rc, nullptr);
    welded.resize(std::size_t(unique) * stride);
    vertices.swap(welded); indices.swap(renumbered); remap.swap(map);
    return true;
}

// Mesh levels of detail (include/trgl.h, trgl_mesh_clean / trgl_mesh_simplify): what stands where Model would have asked Assimp for
// aiProcess_FindDegenerates- and aiProcess_OptimizeMeshes-style steps - on the host, no context needed.
// gl_mesh_clean: the faces of `indices` (3 per face) with two equal indices are dropped, and with `duplicates` those whose three indices,
// rotated, an earlier face has (a mirrored face stays); then the vertices (records of `stride` doubles) that no kept face names:
// both vectors shrink, the kept faces and vertices stay in their order, and remap[v] is the new number of old vertex v or 0xFFFFFFFF.
// gl_mesh_simplify: one level of vertex clustering - the vertices whose positions (the first 3 doubles) share a cell of the grid of width
// `cell` become one, the first mean_count doubles of its record the mean of the cell's vertices that a face names, the rest the lowest-
// numbered one's; then gl_mesh_clean.  A call that fails (gl_last_error()) leaves the three vectors as they were.
inline bool gl_mesh_clean(int stride, std::vector<double>& vertices, std::vector<unsigned int>& indices, std::vector<std::uint32_t>& remap,
                          bool duplicates = true) {
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    trgl_clean_params p{};
    p.vertex_stride = stride; p.flags = TRGL_CLEAN_VERTICES | (duplicates ? TRGL_CLEAN_DUPLICATES : 0u); p.fill = TRGL_CLEAN_FILL_NONE;
    const std::size_t n = vertices.size() / std::size_t(stride > 0 ? stride : 1);
    std::vector<double> kept(vertices.size());
    std::vector<unsigned int> faces(indices.size());
    std::vector<std::uint32_t> map(n);
    std::uint64_t counts[2] = { 0, 0 };
    const int rc = trgl_mesh_clean(nullptr, &p, indices.empty() ? nullptr : reinterpret_cast<const std::uint32_t*>(indices.data()), indices.size() / 3,
                                   vertices.data(), n, TRGL_MEM_HOST, indices.empty() ? nullptr : reinterpret_cast<std::uint32_t*>(faces.data()), nullptr,
                                   map.data(), nullptr, kept.data(), counts);
    if (rc != TRGL_OK) return trgl_shim::fail("gl_mesh_clean", rc, nullptr);
    faces.resize(std::size_t(counts[0]) * 3); kept.resize(std::size_t(counts[1]) * std::size_t(stride));
    vertices.swap(kept); indices.swap(faces); remap.swap(map);
    return true;
}
inline bool gl_mesh_simplify(int stride, double cell, int mean_count, std::vector<double>& vertices, std::vector<unsigned int>& indices,
                             std::vector<std::uint32_t>& remap) {
    static_assert(sizeof(unsigned int) == sizeof(std::uint32_t), "indices are 32-bit");
    trgl_simplify_params p{};
    p.vertex_stride = stride; p.mean_count = mean_count; p.fill = TRGL_CLEAN_FILL_NONE; p.cell = cell;
    const std::size_t n = vertices.size() / std::size_t(stride > 0 ? stride : 1);
    std::vector<double> kept(vertices.size());
    std::vector<unsigned int> faces(indices.size());
    std::vector<std::uint32_t> map(n);
    std::uint64_t counts[2] = { 0, 0 };
    const int rc = trgl_mesh_simplify(nullptr, &p, vertices.data(), n, indices.empty() ? nullptr : reinterpret_cast<const std::uint32_t*>(indices.data()),
                                      indices.size() / 3, TRGL_MEM_HOST, map.data(), nullptr, kept.data(),
                                      indices.empty() ? nullptr : reinterpret_cast<std::uint32_t*>(faces.data()), nullptr, counts);
    if (rc != TRGL_OK) return trgl_shim::fail("gl_mesh_simplify", rc, nullptr);
    faces.resize(std::size_t(counts[0]) * 3); kept.resize(std::size_t(counts[1]) * std::size_t(stride));
    vertices.swap(kept); indices.swap(faces); remap.swap(map);
    return true;
}

// Run everything submitted so far and bring the pixels back into the caller's TGAImage (before framebuffer.get(),
// write_tga_file(), main.cpp:743,773).  The depths follow on demand through the `zbuffer` proxy.
// false: something submitted since the last gl_flush() failed (gl_last_error()); the pixels hold what could be drawn.
inline bool gl_flush(TGAImage& framebuffer) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    return TRGL_SHIM_OK(trgl_read_framebuffer(s.ctx, framebuffer.buffer())) && ok && s.err == TRGL_OK;
}

// main.cpp:751-785 on the device (z-buffer never leaves HBM): fills the three images the reference writes as
// zbuffer.tga, ao.tga and final.tga.  Any of the pointers may be null.
inline bool gl_postprocess(TGAImage& framebuffer, TGAImage* zbuffer_image, TGAImage* ao_map, TGAImage* final_result) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    auto prep = [&](TGAImage* img) -> std::uint8_t* {
        if (!img) return nullptr;
        if (img->width() != s.w || img->height() != s.h || image_bpp(*img) != 3) *img = TGAImage(s.w, s.h, TGAImage::RGB);
        return img->buffer();
    };
    return TRGL_SHIM_OK(trgl_postprocess(s.ctx, nullptr, prep(zbuffer_image), prep(ao_map), prep(final_result))) && ok;
}

// ---- our_gl.h:68-86 ------------------------------------------------------------------------------
// The reference's Frustum (our_gl.cpp:212-280) over trgl_frustum_from_matrix / trgl_frustum_intersects, so that the shim, the C ABI
// and Python cull alike.  Plane and AABB come from the geometry header in use (the reference's own, or trgl_geometry.h).
struct Frustum {
    Plane planes[6];            // left, right, bottom, top, near, far
    enum PlaneIndex { LEFT = 0, RIGHT = 1, BOTTOM = 2, TOP = 3, NEAR = 4, FAR = 5 };
    static Frustum createFromMatrix(const mat<4, 4>& matrix) {
        double m[16], p[24];
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = matrix[r][c];
        trgl_frustum_from_matrix(m, p);
        Frustum f;
        for (int i = 0; i < 6; ++i) { for (int a = 0; a < 3; ++a) f.planes[i].normal[a] = p[4 * i + a]; f.planes[i].d = p[4 * i + 3]; }
        return f;
    }
    bool intersects(const AABB& aabb) const {
        double p[24], lo[3], hi[3];
        for (int i = 0; i < 6; ++i) { for (int a = 0; a < 3; ++a) p[4 * i + a] = planes[i].normal[a]; p[4 * i + 3] = planes[i].d; }
        for (int a = 0; a < 3; ++a) { lo[a] = aabb.min[a]; hi[a] = aabb.max[a]; }
        return trgl_frustum_intersects(p, lo, hi) == 1;
    }
};

// Model::computeAABB (model.cpp:15-40) for a model that keeps `vertices` as records of packed doubles starting with the position
// (model.h:14-20,114): what the reference leaves in Model::localAABB.  Host memory, no GPU (trgl_mesh_bounds).
template <class ModelT> inline AABB gl_mesh_bounds(const ModelT& model) {
    using V = typename std::decay<decltype(model.vertices[0])>::type;
    static_assert(sizeof(V) % sizeof(double) == 0 && sizeof(V) >= 3 * sizeof(double), "vertex records must be packed doubles starting with the position");
    double lo[3], hi[3];
    trgl_mesh_bounds(nullptr, reinterpret_cast<const double*>(model.vertices.data()), int(sizeof(V) / sizeof(double)), model.vertices.size(),
                     TRGL_MEM_HOST, lo, hi);
    AABB b;
    for (int a = 0; a < 3; ++a) { b.min[a] = lo[a]; b.max[a] = hi[a]; }
    return b;
}

// Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388) for such a model with
// `indices` as packed 32-bit numbers (model.h:114-115), in place: what Model::load does behind the loader (model.cpp:59-62).  Host
// memory, no GPU (trgl_mesh_normals / trgl_mesh_tangents).  Return whether the arrays were rewritten; false also when the call was
// refused (an index past the last vertex), which gl_last_error() / gl_last_error_message() then tell, as for every C-ABI error.
template <bool TANGENTS, class ModelT> inline bool gl_mesh_attr(ModelT& model) {
    using V = typename std::decay<decltype(model.vertices[0])>::type;
    static_assert(sizeof(V) % sizeof(double) == 0 && sizeof(V) >= (TANGENTS ? 14 : 6) * sizeof(double),
                  "vertex records must be packed doubles: position, normal (and for tangents texcoord, tangent, bitangent)");
    static_assert(sizeof(model.indices[0]) == sizeof(std::uint32_t), "indices must be 32-bit");
    int generated = 0;
    const int rc = (TANGENTS ? trgl_mesh_tangents : trgl_mesh_normals)(
        nullptr, reinterpret_cast<double*>(model.vertices.data()), int(sizeof(V) / sizeof(double)), model.vertices.size(),
        reinterpret_cast<const std::uint32_t*>(model.indices.data()), model.indices.size() / 3, TRGL_MEM_HOST, &generated);
    if (rc != TRGL_OK) return trgl_shim::fail(TANGENTS ? "trgl_mesh_tangents" : "trgl_mesh_normals", rc, nullptr);   // (no context: the message is the creation error's)
    return generated != 0;
}
template <class ModelT> inline bool gl_mesh_normals(ModelT& model) { return gl_mesh_attr<false>(model); }
template <class ModelT> inline bool gl_mesh_tangents(ModelT& model) { return gl_mesh_attr<true>(model); }

// `std::vector<double> zbuffer_before_eyes = zbuffer;` (main.cpp:700) and `zbuffer = zbuffer_before_eyes;` (main.cpp:730) with the
// depths staying in HBM: slot 0..TRGL_MAX_Z_SNAPSHOTS-1 names the copy.  Triangles batched so far are drawn first, as the proxy's
// accessors do; depths the host wrote through the proxy are uploaded before a snapshot; after a restore the host copy is stale.
inline bool gl_zbuffer_snapshot(TGAImage& framebuffer, int slot = 0) {
    using namespace trgl_shim;
    if (!bind(framebuffer)) return false;                       // (uploads a host copy still marked dirty)
    const bool ok = submit_batch();
    return TRGL_SHIM_OK(trgl_zbuffer_snapshot(state().ctx, slot)) && ok;
}
inline bool gl_zbuffer_restore(TGAImage& framebuffer, int slot = 0) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();                             // the batched triangles see the depths as they are now
    if (!TRGL_SHIM_OK(trgl_zbuffer_restore(s.ctx, slot))) return false;
    s.zbuffer_stale_on_host = true; s.zbuffer_dirty_on_host = false;
    return ok;
}

// framebuffer.gaussian_blur(radius) (tgaimage.cpp:271-324) on the frame where it lives, in HBM: triangles batched so far are drawn first,
// then trgl_framebuffer_blur runs on the device without waiting.  The caller's TGAImage still holds the old pixels; a later
// gl_flush(framebuffer) hands back the blurred ones.  (An image that is not the framebuffer: TGAImage::gaussian_blur, on the host.)
inline bool gl_gaussian_blur(TGAImage& framebuffer, int radius) {
    using namespace trgl_shim;
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    return TRGL_SHIM_OK(trgl_framebuffer_blur(state().ctx, radius)) && ok;
}

// Supersampling and render-to-texture (include/trgl.h, "box-filter resolve and frames as textures"; new work - the reference samples once
// per pixel and its textures come from files).  The filter is exact: (sum of factor x factor bytes + factor * factor / 2) /
// (factor * factor) per channel, factor in 1..TRGL_MAX_BOX_FACTOR.
//   gl_resolve                   the frame in HBM - drawn at factor times the wanted size - box-filtered into `out`, which becomes a
//                                (W / factor) x (H / factor) image of the framebuffer's format (trgl_framebuffer_resolve): triangles batched so
//                                far are drawn first, only the small image crosses PCIe, the call waits for it.  The frame stays as it is.
//   gl_texture_from_framebuffer  the same filtered frame becomes the texture of `slot` without leaving HBM and without a wait
//                                (trgl_texture_from_framebuffer): a snapshot that later draws of any frame of this size sample - a mirror,
//                                a screen in the scene.  Triangles batched so far are drawn first and are part of it.
//   gl_downsample                the filter for an image that is not the framebuffer: on the host, no GPU is touched
inline bool gl_resolve(TGAImage& framebuffer, int factor, TGAImage* out) {
    using namespace trgl_shim;
    State& s = state();
    if (!out) return fail("gl_resolve: out is null", TRGL_E_INVALID, nullptr);
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    if (factor < 1 || factor > TRGL_MAX_BOX_FACTOR || s.w / factor == 0 || s.h / factor == 0)
        return fail("gl_resolve: factor must be 1..16 and at most the framebuffer's width and height", TRGL_E_INVALID, nullptr);
    if (out->width() != s.w / factor || out->height() != s.h / factor || image_bpp(*out) != s.bpp) *out = TGAImage(s.w / factor, s.h / factor, s.bpp);
    return TRGL_SHIM_OK(trgl_framebuffer_resolve(s.ctx, factor, out->buffer(), TRGL_MEM_HOST)) && ok;
}
inline bool gl_texture_from_framebuffer(TGAImage& framebuffer, int slot, int factor = 1) {
    using namespace trgl_shim;
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    return TRGL_SHIM_OK(trgl_texture_from_framebuffer(state().ctx, slot, factor)) && ok;
}
inline bool gl_downsample(const TGAImage& src, int factor, TGAImage* out) {
    using namespace trgl_shim;
    if (!out || out == &src) return fail("gl_downsample: out must be another image", TRGL_E_INVALID, nullptr);
    const int bpp = image_bpp(src);
    if (factor < 1 || factor > TRGL_MAX_BOX_FACTOR || src.width() / factor == 0 || src.height() / factor == 0)
        return fail("gl_downsample: factor must be 1..16 and at most the image's width and height", TRGL_E_INVALID, nullptr);
    if (out->width() != src.width() / factor || out->height() != src.height() / factor || image_bpp(*out) != bpp)
        *out = TGAImage(src.width() / factor, src.height() / factor, bpp);
    const int rc = trgl_image_downsample(nullptr, image_bytes(src), src.width(), src.height(), bpp, factor, out->buffer(), TRGL_MEM_HOST);
    return rc == TRGL_OK ? true : fail("trgl_image_downsample", rc, nullptr);
}

// Mipmapped textures (include/trgl.h, "Mipmapped textures"; new work, the reference has none).
//   gl_texture_mipmaps   builds the mip chain of the texture in `slot` in HBM (trgl_texture_mipmaps): triangles batched so far are drawn
//                        first and sample one level; user shaders of later triangles reach the levels through trgl_sample2D_level,
//                        _linear and _trilinear.  Any call that replaces the slot's texels drops the chain.
//   gl_lod_stage         the four level-of-detail doubles of n triangles in host arrays, from the global Viewport (trgl_lod_stage on the
//                        host: no GPU is touched): clip [n][12], vary [n][K], uv at uv_offset, the result at out_offset.  A UserShader
//                        hands them to its fragment body as four more varyings, which the body passes to trgl_mip_lod.
//   gl_image_sample      the filtered samplers on the host, over an image and the chain TGAImage-side code built with
//                        trgl_image::mipmaps (shim/trgl_image.h): out receives 5 bytes a sample (b, g, r, a, bytespp)
inline bool gl_texture_mipmaps(TGAImage& framebuffer, int slot) {
    using namespace trgl_shim;
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    return TRGL_SHIM_OK(trgl_texture_mipmaps(state().ctx, slot)) && ok;
}
inline bool gl_lod_stage(const double* clip, double* vary, uint64_t n, int K, int uv_offset, int out_offset) {
    using namespace trgl_shim;
    double vp[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = Viewport[r][c];
    const int rc = trgl_lod_stage(nullptr, vp, clip, vary, n, K, uv_offset, out_offset, TRGL_MEM_HOST);
    return rc == TRGL_OK ? true : fail("trgl_lod_stage", rc, nullptr);
}
inline bool gl_image_sample(const TGAImage& img, const std::vector<uint8_t>& chain, const double* uv, const double* lod, int mode, uint64_t n, uint8_t* out) {
    using namespace trgl_shim;
    const int rc = trgl_image_sample(image_bytes(img), chain.empty() ? nullptr : chain.data(), img.width(), img.height(), image_bpp(img),
                                     chain.empty() ? 1 : TRGL_MAX_MIP_LEVELS, uv, lod, mode, n, out);
    return rc == TRGL_OK ? true : fail("trgl_image_sample", rc, nullptr);
}

// Shadow mapping as a post-pass (include/trgl.h, "shadow mapping as a post-pass"; new work, the reference has none).  Draw the light's
// view, gl_zbuffer_snapshot(framebuffer, slot), clear, draw the camera's view, then:
//   gl_shadow_matrix   the matrix of trgl_shadow_params::screen_to_light from the two views' ModelView / Perspective / Viewport as they
//                      were when each was drawn; false for a singular camera matrix (gl_last_error())
//   gl_shadow_mask     the mask of the depths in HBM against the snapshot in `slot` (trgl_shadow_mask): triangles batched so far are drawn
//                      first.  `mask` becomes a W x H GRAYSCALE image holding it (the call waits for those bytes); a caller may soften it
//                      with TGAImage::gaussian_blur.  The shim's images are host objects: a null `mask` is an error (TRGL_E_INVALID), and the
//                      sequence that keeps the mask in HBM is the C ABI's (trgl_shadow_mask with TRGL_MEM_DEVICE).
//   gl_modulate        the frame in HBM multiplied by the mask (trgl_framebuffer_modulate), without waiting; the caller's TGAImage still
//                      holds the old pixels, a later gl_flush(framebuffer) hands back the darkened ones.
inline bool gl_shadow_matrix(const mat<4, 4>& light_mv, const mat<4, 4>& light_proj, const mat<4, 4>& light_vp,
                             const mat<4, 4>& cam_mv, const mat<4, 4>& cam_proj, const mat<4, 4>& cam_vp, mat<4, 4>& out) {
    const mat<4, 4>* in[6] = { &light_mv, &light_proj, &light_vp, &cam_mv, &cam_proj, &cam_vp };
    double m[6][16], o[16];
    for (int k = 0; k < 6; ++k) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[k][4 * r + c] = (*in[k])[r][c];
    const int rc = trgl_shadow_matrix(m[0], m[1], m[2], m[3], m[4], m[5], o);
    if (rc != TRGL_OK) return trgl_shim::fail("trgl_shadow_matrix", rc, nullptr);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[r][c] = o[4 * r + c];
    return true;
}
inline bool gl_shadow_mask(TGAImage& framebuffer, const trgl_shadow_params& params, int slot, TGAImage* mask) {
    using namespace trgl_shim;
    State& s = state();
    if (!mask) return fail("gl_shadow_mask: mask is null", TRGL_E_INVALID, nullptr);
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    if (mask->width() != s.w || mask->height() != s.h || image_bpp(*mask) != 1) *mask = TGAImage(s.w, s.h, TGAImage::GRAYSCALE);
    return TRGL_SHIM_OK(trgl_shadow_mask(s.ctx, &params, slot, mask->buffer(), TRGL_MEM_HOST)) && ok;
}
inline bool gl_modulate(TGAImage& framebuffer, const TGAImage& mask) {
    using namespace trgl_shim;
    State& s = state();
    if (!bind(framebuffer)) return false;
    const bool ok = submit_batch();
    if (mask.width() != s.w || mask.height() != s.h || image_bpp(mask) != 1)
        return fail("gl_modulate: the mask must be a GRAYSCALE image of the framebuffer's size", TRGL_E_INVALID, nullptr);
    return TRGL_SHIM_OK(trgl_framebuffer_modulate(s.ctx, image_bytes(mask), TRGL_MEM_HOST)) && ok;
}

// Occlusion culling of model boxes (include/trgl.h, "occlusion culling of model boxes"; new work - the reference culls with
// frustum.intersects alone, main.cpp:647,680,706).  gl_occlusion_test asks for every box - world-space boxes with
// view_proj = Perspective * ModelView, main.cpp:623 - whether it is hidden behind the depths in HBM (snapshot_slot = -1: the z-buffer as it
// is once the triangles batched so far are drawn; else the depths kept by gl_zbuffer_snapshot) under the current Viewport; the call waits
// for the codes, one TRGL_OCCL_* byte per box.  gl_occlusion_draw(code) is the other half of `if (frustum.intersects(box))`.  A call
// that fails (gl_last_error()) answers TRGL_OCCL_UNDECIDED for every box: draw them all.
inline std::vector<std::uint8_t> gl_occlusion_test(const std::vector<AABB>& boxes, const mat<4, 4>& view_proj, int snapshot_slot = -1) {
    using namespace trgl_shim;
    State& s = state();
    std::vector<std::uint8_t> codes(boxes.size(), std::uint8_t(TRGL_OCCL_UNDECIDED));
    if (boxes.empty()) return codes;
    if (!s.ctx) { fail("gl_occlusion_test: nothing has been drawn yet", TRGL_E_STATE, nullptr); return codes; }
    bool ok = submit_batch();
    if (s.zbuffer_dirty_on_host && zbuffer.raw().size() == std::size_t(s.w) * s.h) {      // depths the host wrote since the last draw, as bind() uploads them
        ok = TRGL_SHIM_OK(trgl_write_zbuffer(s.ctx, zbuffer.raw().data())) && ok;
        s.zbuffer_dirty_on_host = false; s.zbuffer_stale_on_host = false;
    }
    double vp[16];                                              // (a batch carries the Viewport it was drawn under; the query takes today's)
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) vp[4 * r + c] = Viewport[r][c];
    ok = TRGL_SHIM_OK(trgl_set_viewport(s.ctx, vp)) && ok;
    std::vector<double> b(boxes.size() * 6);
    for (size_t i = 0; i < boxes.size(); ++i)
        for (int a = 0; a < 3; ++a) { b[6 * i + a] = boxes[i].min[a]; b[6 * i + 3 + a] = boxes[i].max[a]; }
    double m[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = view_proj[r][c];
    if (!(TRGL_SHIM_OK(trgl_occlusion_boxes(s.ctx, m, b.data(), b.size() / 6, TRGL_MEM_HOST, snapshot_slot, codes.data(), TRGL_MEM_HOST)) && ok))
        codes.assign(boxes.size(), std::uint8_t(TRGL_OCCL_UNDECIDED));
    return codes;
}
inline bool gl_occlusion_draw(std::uint8_t code) { return (code & 1) != 0; }

// World boxes and frustum codes of many models at once (include/trgl.h, trgl_instance_boxes / trgl_frustum_boxes): the array forms of
// `model.getWorldAABB(modelMatrix)` and `frustum.intersects(worldAABB)` (main.cpp:555-557, 647).  Both run on the host and need no context.
// gl_instance_boxes: AABB::transform of `local` (gl_mesh_bounds) under every matrix, bit for bit local.transform(model_matrices[i]).
// gl_frustum_test(frustum, boxes): one byte per box, TRGL_OCCL_VISIBLE where the frustum intersects it and TRGL_OCCL_OUTSIDE where not.
// gl_frustum_test(frustum, boxes, codes): merges into the codes gl_occlusion_test returned - a culled box becomes TRGL_OCCL_OUTSIDE, every
// other byte stays - so that gl_occlusion_draw(codes[i]) answers both tests, and the vector is the `visible` of gl_draw_instanced.
// A call that fails (gl_last_error()) answers empty boxes at the origin / leaves the codes as they are (SET: UNDECIDED, draw them all).
inline std::vector<AABB> gl_instance_boxes(const AABB& local, const std::vector<mat<4, 4>>& model_matrices) {
    const std::size_t n = model_matrices.size();
    std::vector<double> m(n * 16), b(n * 6, 0.0);
    for (std::size_t i = 0; i < n; ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[16 * i + 4 * r + c] = model_matrices[i][r][c];
    const double box[6] = { local.min[0], local.min[1], local.min[2], local.max[0], local.max[1], local.max[2] };
    const int rc = trgl_instance_boxes(nullptr, box, 0, m.data(), 16, n, TRGL_MEM_HOST, b.data());
    if (rc != TRGL_OK) trgl_shim::fail("gl_instance_boxes", rc, nullptr);
    std::vector<AABB> boxes(n);
    for (std::size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) { boxes[i].min[a] = b[6 * i + a]; boxes[i].max[a] = b[6 * i + 3 + a]; }
    return boxes;
}
namespace trgl_shim {
inline bool frustum_codes(const Frustum& frustum, const std::vector<AABB>& boxes, int mode, std::uint8_t* codes) {
    double p[24];
    for (int i = 0; i < 6; ++i) { for (int a = 0; a < 3; ++a) p[4 * i + a] = frustum.planes[i].normal[a]; p[4 * i + 3] = frustum.planes[i].d; }
    std::vector<double> b(boxes.size() * 6);
    for (std::size_t i = 0; i < boxes.size(); ++i)
        for (int a = 0; a < 3; ++a) { b[6 * i + a] = boxes[i].min[a]; b[6 * i + 3 + a] = boxes[i].max[a]; }
    const int rc = trgl_frustum_boxes(nullptr, p, b.data(), boxes.size(), mode, TRGL_MEM_HOST, codes);
    return rc == TRGL_OK || fail(mode == TRGL_FRUSTUM_SET ? "gl_frustum_test" : "gl_frustum_test (merge)", rc, nullptr);
}
}  // namespace trgl_shim
inline std::vector<std::uint8_t> gl_frustum_test(const Frustum& frustum, const std::vector<AABB>& boxes) {
    std::vector<std::uint8_t> codes(boxes.size(), std::uint8_t(TRGL_OCCL_UNDECIDED));
    trgl_shim::frustum_codes(frustum, boxes, TRGL_FRUSTUM_SET, codes.data());
    return codes;
}
inline bool gl_frustum_test(const Frustum& frustum, const std::vector<AABB>& boxes, std::vector<std::uint8_t>& codes) {
    if (codes.size() != boxes.size()) return trgl_shim::fail("gl_frustum_test: one code per box is needed to merge into", TRGL_E_INVALID, nullptr);
    return trgl_shim::frustum_codes(frustum, boxes, TRGL_FRUSTUM_MERGE, codes.data());
}

inline void print_render_stats() {                                                // our_gl.cpp:204-210
    trgl_shim::State& s = trgl_shim::state();
    trgl_stats st{};
    if (s.ctx && (trgl_shim::submit_batch(), TRGL_SHIM_OK(trgl_get_stats(s.ctx, &st)))) { }
    else { st.min_x = st.min_y = INT32_MAX; st.max_x = st.max_y = INT32_MIN; st.min_z = std::numeric_limits<double>::infinity(); st.max_z = -st.min_z; }
    char line[1024];
    trgl_format_stats(&st, line, sizeof line);
    std::fputs(line, stderr);
}
inline void gl_shutdown() { trgl_shim::State& s = trgl_shim::state(); if (s.ctx) { trgl_destroy(s.ctx); s.ctx = nullptr; } }
