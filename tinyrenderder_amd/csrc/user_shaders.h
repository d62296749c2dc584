// user_shaders.h — run-time compilation of user shaders (user_shaders.cpp) for the registration code of trgl_shader.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace trgl {
// The code object (for the architecture the library is built for) of the kernel of `source` with K varyings and the
// TRGL_SHADER_* flags `flags` - the shade kernel, or with TRGL_SHADER_MAY_DISCARD the raster kernel - compiled with hiprtc or
// taken from the process-wide cache.  TRGL_OK, TRGL_E_INVALID (bad K, unknown flags or a blending flag without MAY_DISCARD, compile error: the log says why) or
// TRGL_E_UNSUPPORTED (no hiprtc).  *code stays valid for the life of the process; *log is the compiler's log (a cached entry
// returns the log of its compilation, warnings included).
int user_shader_code(const char* source, int n_varyings, uint32_t flags, std::string* log, const std::vector<char>** code);
// The same for a user vertex shader (vertex_user.h behind the source, which defines trgl_vertex); its cache entries are apart from
// those of fragment shaders with the same text.
int user_vertex_shader_code(const char* source, int n_varyings, std::string* log, const std::vector<char>** code);
// the message trgl_last_error(NULL) returns (trgl_host.cpp)
void set_global_error(const std::string& msg);
// the name of the kernel in that code object: shade_user.h, or raster_user.h with TRGL_SHADER_MAY_DISCARD
constexpr const char* USER_SHADE_KERNEL = "trgl_shade_user";
constexpr const char* USER_RASTER_KERNEL = "trgl_raster_user";
constexpr const char* USER_VERTEX_KERNEL = "trgl_vertex_user";       // vertex_user.h
constexpr const char* USER_VERTEX_INSTANCED_KERNEL = "trgl_vertex_user_instanced";     // ... its second kernel, in the same code object
}  // namespace trgl
