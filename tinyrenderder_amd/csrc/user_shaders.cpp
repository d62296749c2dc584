// user_shaders.cpp — user shaders compiled at run time (include/trgl.h, "User shaders").
//
// The source of a user shader is compiled by hiprtc between the prelude (user_prelude.h) and a kernel template: the shade kernel
// (shade_user.h), for a shader that may discard the raster kernel (raster_user.h), or for a vertex shader the vertex-stage kernel
// (vertex_user.h).  Those and the headers they include are built
// into the library as text (tools/embed_sources.py) and handed to hiprtc as in-memory headers, with three stand-ins for the C headers
// hiprtc does not have.  libhiprtc is loaded when first needed, as librccl is: without it the library loads and everything but the
// compile calls here works.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/trgl.h"
#include "user_shaders.h"
#include "user_shader_sources.inc"

#ifndef TRGL_ARCH
#error "TRGL_ARCH (the offload architecture of the library) must be defined"
#endif

namespace {

struct Hiprtc {
    void* lib = nullptr;
    decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
    decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
    decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
    decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
    decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
    decltype(&hiprtcGetCode) GetCode = nullptr;
    decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
    bool ok = false;
};
Hiprtc& hiprtc() {          // (called with the cache's mutex held)
    static Hiprtc r;
    if (!r.lib) {
        r.lib = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
        if (!r.lib) r.lib = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (r.lib) {
            r.CreateProgram = reinterpret_cast<decltype(r.CreateProgram)>(dlsym(r.lib, "hiprtcCreateProgram"));
            r.CompileProgram = reinterpret_cast<decltype(r.CompileProgram)>(dlsym(r.lib, "hiprtcCompileProgram"));
            r.GetProgramLogSize = reinterpret_cast<decltype(r.GetProgramLogSize)>(dlsym(r.lib, "hiprtcGetProgramLogSize"));
            r.GetProgramLog = reinterpret_cast<decltype(r.GetProgramLog)>(dlsym(r.lib, "hiprtcGetProgramLog"));
            r.GetCodeSize = reinterpret_cast<decltype(r.GetCodeSize)>(dlsym(r.lib, "hiprtcGetCodeSize"));
            r.GetCode = reinterpret_cast<decltype(r.GetCode)>(dlsym(r.lib, "hiprtcGetCode"));
            r.DestroyProgram = reinterpret_cast<decltype(r.DestroyProgram)>(dlsym(r.lib, "hiprtcDestroyProgram"));
            r.ok = r.CreateProgram && r.CompileProgram && r.GetProgramLogSize && r.GetProgramLog && r.GetCodeSize && r.GetCode &&
                   r.DestroyProgram;
        }
    }
    return r;
}

// the library's own flags (csrc/Makefile), for its own architecture: the plain target, never an xnack+ one
const char* const kOptions[] = { "--offload-arch=" TRGL_ARCH, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                                 "-fhip-fp32-correctly-rounded-divide-sqrt" };
constexpr int kNumOptions = sizeof(kOptions) / sizeof(kOptions[0]);

// what hiprtc lacks of the C headers trgl_device.h and trgl.h include
const char* const kStubNames[] = { "limits.h", "stddef.h", "stdint.h" };
const char* const kStubs[] = { "#pragma once\n#define INT_MIN (-2147483647 - 1)\n#define INT32_MAX 2147483647\n#define INT32_MIN (-2147483647 - 1)\n",
                               "#pragma once\n#define offsetof(t, m) __builtin_offsetof(t, m)\n",
                               "#pragma once\nusing namespace __hip_internal;\n" };

struct Compiled { std::vector<char> code; std::string log; };   // the code object and the compiler's log (its warnings)
struct Cache {
    std::mutex mu;
    std::unordered_map<std::string, std::unique_ptr<Compiled>> entries;   // key: stage (fragment flags, or vertex), K and source
};
Cache& cache() { static Cache c; return c; }

int compile(Hiprtc& rtc, const std::string& program, std::string* log, std::vector<char>* code) {
    std::vector<const char*> headers, names;
    for (const auto& e : trgl_embedded) { headers.push_back(e.text); names.push_back(e.name); }
    for (int i = 0; i < 3; ++i) { headers.push_back(kStubs[i]); names.push_back(kStubNames[i]); }
    hiprtcProgram p = nullptr;
    if (rtc.CreateProgram(&p, program.c_str(), "trgl_user_shader.hip", (int)headers.size(), headers.data(), names.data()) != HIPRTC_SUCCESS) {
        *log = "hiprtcCreateProgram failed";
        return TRGL_E_UNSUPPORTED;
    }
    const hiprtcResult rc = rtc.CompileProgram(p, kNumOptions, const_cast<const char**>(kOptions));
    size_t n = 0;
    if (rtc.GetProgramLogSize(p, &n) == HIPRTC_SUCCESS && n > 1) {
        std::vector<char> buf(n + 1, 0);
        if (rtc.GetProgramLog(p, buf.data()) == HIPRTC_SUCCESS) *log = buf.data();
    }
    int r = TRGL_OK;
    if (rc != HIPRTC_SUCCESS) {
        if (log->empty()) *log = "hiprtc: compilation failed";
        r = TRGL_E_INVALID;
    } else if (rtc.GetCodeSize(p, &n) != HIPRTC_SUCCESS || n == 0) {
        *log = "hiprtc: no code object";
        r = TRGL_E_INVALID;
    } else {
        code->resize(n);
        if (rtc.GetCode(p, code->data()) != HIPRTC_SUCCESS) { *log = "hiprtcGetCode failed"; r = TRGL_E_INVALID; }
    }
    rtc.DestroyProgram(&p);
    return r;
}

}  // namespace

namespace trgl {

// the code object of `program` from the cache, or compiled now; `key_head` tells programs of different stages apart
static int cached_code(const std::string& key_head, const std::string& program, std::string* log, const std::vector<char>** code) {
    std::string key = key_head + '\n';
    for (const char* o : kOptions) { key += o; key += ' '; }
    key += '\n'; key += program;
    Cache& c = cache();
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.entries.find(key);
    if (it != c.entries.end()) { *code = &it->second->code; *log = it->second->log; return TRGL_OK; }   // (the warnings again)
    Hiprtc& rtc = hiprtc();
    if (!rtc.ok) { *log = "libhiprtc could not be loaded: user shaders are not available"; return TRGL_E_UNSUPPORTED; }
    std::unique_ptr<Compiled> obj(new Compiled());
    const int r = compile(rtc, program, log, &obj->code);
    if (r) return r;                            // (failures are not cached)
    obj->log = *log;
    *code = &obj->code;
    c.entries.emplace(key, std::move(obj));
    return TRGL_OK;
}

static bool source_and_k_ok(const char* source, int K, std::string* log) {
    log->clear();
    if (!source) { *log = "source is null"; return false; }
    if (K < 0 || K > TRGL_MAX_USER_VARY) { *log = "n_varyings must be in 0.." + std::to_string(TRGL_MAX_USER_VARY); return false; }
    return true;
}

int user_shader_code(const char* source, int K, uint32_t flags, std::string* log, const std::vector<char>** code) {
    if (!source_and_k_ok(source, K, log)) return TRGL_E_INVALID;
    const uint32_t known = TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE;
    if (flags & ~known) { *log = "unknown flag bits " + std::to_string(flags & ~known); return TRGL_E_INVALID; }
    const bool may_discard = (flags & TRGL_SHADER_MAY_DISCARD) != 0;
    if (!may_discard && flags) {                // (both need the kernel that runs the fragments of a pixel in order)
        *log = "flag bits " + std::to_string(flags) + ": TRGL_SHADER_READS_DEST and TRGL_SHADER_NO_DEPTH_WRITE are only valid with TRGL_SHADER_MAY_DISCARD";
        return TRGL_E_INVALID;
    }
    // the user's lines keep their own numbers in the log (#line)
    const std::string program = "#include \"user_prelude.h\"\n#define TRGL_USER_VARY " + std::to_string(K) +
                                "\n#define TRGL_USER_MAY_DISCARD " + (may_discard ? "1" : "0") +
                                "\n#define TRGL_USER_READS_DEST " + ((flags & TRGL_SHADER_READS_DEST) ? "1" : "0") +
                                "\n#define TRGL_USER_DEPTH_WRITE " + ((flags & TRGL_SHADER_NO_DEPTH_WRITE) ? "0" : "1") +
                                "\n#line 1 \"user_shader\"\n" + source + "\n#include \"" + (may_discard ? "raster_user.h" : "shade_user.h") + "\"\n";
    return cached_code("flags " + std::to_string(flags), program, log, code);
}

int user_vertex_shader_code(const char* source, int K, std::string* log, const std::vector<char>** code) {
    if (!source_and_k_ok(source, K, log)) return TRGL_E_INVALID;
    const std::string program = "#include \"user_prelude.h\"\n#define TRGL_USER_VARY " + std::to_string(K) +
                                "\n#line 1 \"user_shader\"\n" + source + "\n#include \"vertex_user.h\"\n";
    return cached_code("vertex", program, log, code);       // (a fragment program's key starts with "flags")
}

}  // namespace trgl

extern "C" int trgl_shader_compile_ex(const char* source, int n_varyings, uint32_t flags, char* log, size_t log_len) {
    std::string msg;
    const std::vector<char>* code = nullptr;
    const int r = trgl::user_shader_code(source, n_varyings, flags, &msg, &code);
    if (r) trgl::set_global_error("trgl_shader_compile: " + msg);
    if (log && log_len) {
        const size_t n = msg.size() < log_len - 1 ? msg.size() : log_len - 1;
        std::memcpy(log, msg.data(), n);
        log[n] = '\0';
    }
    return r;
}

extern "C" int trgl_shader_compile(const char* source, int n_varyings, char* log, size_t log_len) {
    return trgl_shader_compile_ex(source, n_varyings, 0u, log, log_len);
}

extern "C" int trgl_vertex_shader_compile(const char* source, int n_varyings, char* log, size_t log_len) {
    std::string msg;
    const std::vector<char>* code = nullptr;
    const int r = trgl::user_vertex_shader_code(source, n_varyings, &msg, &code);
    if (r) trgl::set_global_error("trgl_vertex_shader_compile: " + msg);
    if (log && log_len) {
        const size_t n = msg.size() < log_len - 1 ? msg.size() : log_len - 1;
        std::memcpy(log, msg.data(), n);
        log[n] = '\0';
    }
    return r;
}
