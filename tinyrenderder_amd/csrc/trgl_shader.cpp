// trgl_shader.cpp — run-time shader registration: fragment kinds (trgl_register_shader, trgl_register_shader_ex) and vertex shaders
// (trgl_register_vertex_shader), compiled by user_shaders.cpp and loaded as modules of the context.
// The entry points that run a vertex shader live in trgl_stage_mesh.cpp and trgl_stage_instance.cpp.
#include "trgl_ctx.h"
#include "user_shaders.h"

extern "C" {

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

}  // extern "C"
