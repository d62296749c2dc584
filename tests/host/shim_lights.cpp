// The shim's PhongShaderT / EyeShaderT::initLightDirections (tinyrenderder_amd/shim/trgl_shaders.h) against the reference's own
// PhongShader / EyeShader::initLightDirections (main.cpp:55-69, 187-197), recorded in tests/golden/lights_golden.bin by
// tests/golden/make_shader_golden.py: int32 count, int32 0, then per item 25 input doubles (ModelView[16], key, fill, rim in
// world space) and 15 output doubles (Phong key, fill, rim, Eye key, rim in eye space).  Bit-exact; exit status 0 = all equal.
//   g++ -std=c++17 -O2 -ffp-contract=off -I tinyrenderder_amd/shim -I include tests/host/shim_lights.cpp -o shim_lights
//   ./shim_lights tests/golden/lights_golden.bin
#include "trgl_shaders.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

struct NoModel {
    vec3 vert(int, int) const { return vec3(); } vec3 normal(int, int) const { return vec3(); } vec2 uv(int, int) const { return vec2(); }
    int diffuse_slot() const { return -1; } int normal_slot() const { return -1; } int specular_slot() const { return -1; }
};

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: shim_lights lights_golden.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<char> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (buf.size() < 8) return 2;
    int32_t count; std::memcpy(&count, buf.data(), 4);
    if (buf.size() != 8 + (size_t)count * 40 * 8) { std::fprintf(stderr, "bad fixture size\n"); return 2; }
    const double* rows = reinterpret_cast<const double*>(buf.data() + 8);
    int bad = 0;
    for (int i = 0; i < count; ++i) {
        const double* r = rows + (size_t)i * 40;
        for (int a = 0; a < 4; ++a) for (int c = 0; c < 4; ++c) ModelView[a][c] = r[4 * a + c];
        vec3 d[3];
        for (int k = 0; k < 3; ++k) for (int c = 0; c < 3; ++c) d[k][c] = r[16 + 3 * k + c];
        NoModel m;
        PhongShaderT<NoModel> p(&m); p.initLightDirections(d[0], d[1], d[2]);
        EyeShaderT<NoModel> e(&m); e.initLightDirections(d[0], d[2]);
        const vec3 got[5] = { p.key_light_dir_eye, p.fill_light_dir_eye, p.rim_light_dir_eye, e.key_light_dir_eye, e.rim_light_dir_eye };
        for (int k = 0; k < 5; ++k) for (int c = 0; c < 3; ++c) {
            const double g = got[k][c], w = r[25 + 3 * k + c];
            if (std::memcmp(&g, &w, 8) != 0) {
                if (bad++ < 5) std::fprintf(stderr, "item %d direction %d[%d]: %.17g != %.17g\n", i, k, c, g, w);
            }
        }
    }
    if (bad) std::fprintf(stderr, "%d components differ\n", bad);
    return bad ? 1 : 0;
}
