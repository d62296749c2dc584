// user_shaders.h — run-time compilation of user shaders (user_shaders.cpp) for the context code of trgl_api.cpp.
#pragma once
#include <string>
#include <vector>

namespace trgl {
// The code object (for the architecture the library is built for) of the shade kernel of `source` with K varyings, compiled
// with hiprtc or taken from the process-wide cache.  TRGL_OK, TRGL_E_INVALID (bad K, compile error: the log says why) or
// TRGL_E_UNSUPPORTED (no hiprtc).  *code stays valid for the life of the process; *log is the compiler's log (a cached entry
// returns the log of its compilation, warnings included).
int user_shader_code(const char* source, int n_varyings, std::string* log, const std::vector<char>** code);
// the message trgl_last_error(NULL) returns (trgl_api.cpp)
void set_global_error(const std::string& msg);
// the name of the kernel in that code object
constexpr const char* USER_SHADE_KERNEL = "trgl_shade_user";
}  // namespace trgl
