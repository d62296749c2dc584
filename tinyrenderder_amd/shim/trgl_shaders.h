// trgl_shaders.h — the shader kinds the device implements, as IShader subclasses with the reference's member
// names (main.cpp:39-90, 176-218) so a main.cpp-shaped face loop compiles unchanged:
//     for v in 0..2: clip[v] = shader.vertex(face, v);  rasterize(clip, shader, framebuffer);
// vertex() runs on the host (3 mat*vec per vertex, as in the reference) - or, through gl_draw_model(), on the device: the built-in
// stage, or a user vertex shader (UserShader::vertex_kind); fragment() runs on the GPU, selected by describe().  `ModelT` is anything with vert(face,v), normal(face,v), uv(face,v) and texture slots.
#pragma once
#include "trgl_gl.h"

struct FlatShader : IShader {
    TGAColor color;
    bool describe(trgl_shader_desc& d) const override { d.kind = TRGL_SHADER_FLAT; d.color = trgl_shim::pack_bgra(color); return true; }
};

// the shader that DISCARDS (our_gl.h:51: fragment() returns { true, ... } and rasterize() skips the fragment, our_gl.cpp:187-188):
// a flat colour on the even cells of a cells x cells checker over the perspective-correct barycentrics (include/trgl.h)
struct CheckerShader : IShader {
    TGAColor color; int cells = 8;
    bool describe(trgl_shader_desc& d) const override {
        d.kind = TRGL_SHADER_CHECKER; d.color = trgl_shim::pack_bgra(color); d.uniforms.reserved = cells; return true;
    }
};

// classic tinyrenderer Gouraud: per-vertex intensity, colour = base * intensity (TGAColor::operator*, tgaimage.h:55-62)
struct GouraudShader : IShader {
    TGAColor base = TGAColor(255, 255, 255);
    double varying_intensity[3] = { 0, 0, 0 };
    bool describe(trgl_shader_desc& d) const override {
        d.kind = TRGL_SHADER_GOURAUD; d.color = trgl_shim::pack_bgra(base); d.varyings = varying_intensity; return true;
    }
};

// A user shader (gl_register_shader, include/trgl.h "User shaders"): `kind` is what gl_register_shader returned; per triangle,
// `varyings` holds the K doubles it was registered with and `color` is what trgl_frag_in::color receives.  `uniforms` is passed
// as it is (texture slots -1 by default).  Varyings of another size are a programming error: rasterize() aborts.  Through
// gl_draw_model() / gl_draw_indexed() (a kind registered with K = 24) the device vertex stage makes the varyings: `varyings` and
// `color` are not used there (trgl_frag_in::color is 0xffffffff).
// vertex_kind: a user vertex shader (gl_register_vertex_shader), -1 = none.  With one, gl_draw_model() / gl_draw_indexed() run its
// trgl_vertex over the mesh in place of the built-in stage; `kind` may then also be a BUILT-IN kind (TRGL_SHADER_GOURAUD with a
// vertex shader of 3 varyings, say), the varyings are the vertex shader's, and every face gets `color`.
struct UserShader : IShader {
    int kind = -1;
    int vertex_kind = -1;
    std::vector<double> varyings;
    TGAColor color = TGAColor(255, 255, 255);
    trgl_uniforms uniforms{};
    UserShader() { uniforms.tex_diffuse = uniforms.tex_normal = uniforms.tex_specular = -1; }
    explicit UserShader(int k) : UserShader() { kind = k; }
    bool describe(trgl_shader_desc& d) const override {
        const bool builtin = vertex_kind >= 0 && kind >= 0 && kind < TRGL_NUM_SHADERS;        // (drawn through the vertex shader only)
        if (!builtin && (kind < TRGL_SHADER_USER_FIRST || kind - TRGL_SHADER_USER_FIRST >= int(trgl_shim::state().user.size()))) {
            std::fprintf(stderr, "trgl: UserShader: kind %d is not a registered user shader\n", kind);
            return false;
        }
        d.kind = kind; d.uniforms = uniforms; d.color = trgl_shim::pack_bgra(color); d.vertex_kind = vertex_kind;
        d.varyings = int(varyings.size()) == trgl_shim::vary_count(kind) ? varyings.data() : nullptr;   // (rasterize() checks)
        return true;
    }
};

namespace trgl_shim {
inline void fill_lights(trgl_uniforms& u, const vec3& key, const vec3& fill, const vec3& rim) {
    for (int i = 0; i < 3; ++i) { u.key_light_dir_eye[i] = key[i]; u.fill_light_dir_eye[i] = fill[i]; u.rim_light_dir_eye[i] = rim[i]; }
}
inline vec3 light_to_eye(const vec3& world) {                      // main.cpp:58-68: upper-left 3x3 of ModelView
    mat<3, 3> nm;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) nm[i][j] = ModelView[i][j];
    return normalized(nm * world);
}
}  // namespace trgl_shim

template <class ModelT> struct PhongShaderT : IShader {            // main.cpp:39-171
    const ModelT* model;
    vec3 key_light_dir_eye, fill_light_dir_eye, rim_light_dir_eye;
    // one contiguous block in the order include/trgl.h documents: uv[3], position_eye[3], normal_eye[3]
    struct { vec2 varying_uv[3]; vec3 varying_position_eye[3]; vec3 varying_normal_eye[3]; } v;
    double normal_map_strength = 1.0;
    explicit PhongShaderT(const ModelT* m) : model(m) {}
    void initLightDirections(const vec3& key, const vec3& fill, const vec3& rim) {
        key_light_dir_eye = trgl_shim::light_to_eye(key);
        fill_light_dir_eye = trgl_shim::light_to_eye(fill);
        rim_light_dir_eye = trgl_shim::light_to_eye(rim);
    }
    vec4 vertex(int face, int nth) override {                      // main.cpp:71-90
        vec3 p = model->vert(face, nth), n = model->normal(face, nth);
        v.varying_uv[nth] = model->uv(face, nth);
        vec4 pe = ModelView * make_vec4(p[0], p[1], p[2], 1.0);
        v.varying_position_eye[nth] = pe.xyz();
        v.varying_normal_eye[nth] = (ModelView * make_vec4(n[0], n[1], n[2], 0.0)).xyz();
        return Perspective * pe;
    }
    bool describe(trgl_shader_desc& d) const override {
        static_assert(sizeof(v) == 24 * sizeof(double), "varyings block must be 24 packed doubles");
        d.kind = TRGL_SHADER_PHONG;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) d.uniforms.model_view[4 * r + c] = ModelView[r][c];  // main.cpp:116
        trgl_shim::fill_lights(d.uniforms, key_light_dir_eye, fill_light_dir_eye, rim_light_dir_eye);
        d.uniforms.normal_map_strength = normal_map_strength;
        d.uniforms.tex_diffuse = model->diffuse_slot(); d.uniforms.tex_normal = model->normal_slot();
        d.uniforms.tex_specular = model->specular_slot(); d.uniforms.reserved = 0;
        d.varyings = reinterpret_cast<const double*>(&v);
        return true;
    }
};

template <class ModelT> struct EyeShaderT : IShader {              // main.cpp:176-262
    const ModelT* model;
    vec3 key_light_dir_eye, rim_light_dir_eye;
    struct { vec2 varying_uv[3]; vec3 varying_position_eye[3]; vec3 varying_normal_eye[3]; } v;
    explicit EyeShaderT(const ModelT* m) : model(m) {}
    void initLightDirections(const vec3& key, const vec3& rim) {
        key_light_dir_eye = trgl_shim::light_to_eye(key);
        rim_light_dir_eye = trgl_shim::light_to_eye(rim);
    }
    vec4 vertex(int face, int nth) override {                      // main.cpp:199-218
        vec3 p = model->vert(face, nth), n = model->normal(face, nth);
        v.varying_uv[nth] = model->uv(face, nth);
        vec4 pe = ModelView * make_vec4(p[0], p[1], p[2], 1.0);
        v.varying_position_eye[nth] = pe.xyz();
        v.varying_normal_eye[nth] = (ModelView * make_vec4(n[0], n[1], n[2], 0.0)).xyz();
        return Perspective * pe;
    }
    bool describe(trgl_shader_desc& d) const override {
        d.kind = TRGL_SHADER_EYE;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) d.uniforms.model_view[4 * r + c] = ModelView[r][c];
        trgl_shim::fill_lights(d.uniforms, key_light_dir_eye, vec3(), rim_light_dir_eye);
        d.uniforms.normal_map_strength = 1.0;
        d.uniforms.tex_diffuse = model->diffuse_slot(); d.uniforms.tex_normal = -1;
        d.uniforms.tex_specular = model->specular_slot(); d.uniforms.reserved = 0;
        d.varyings = reinterpret_cast<const double*>(&v);
        return true;
    }
};
