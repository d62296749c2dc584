// demo_mesh_attr.cpp — what Model::load does behind the loader (model.cpp:59-62) for a model that arrives without normals and tangents:
// gl_mesh_normals, gl_mesh_tangents and gl_mesh_bounds on the host arrays, then one Phong draw through the shim.
//   demo_mesh_attr <scene.bin> <out.bin>
// scene.bin has demo_scene's layout with one model (tests/test_mesh_attr_gpu.py writes it).  out.bin = the two `generated` answers and
// (answer, gl_last_error()) of a model with an index out of range as int32, the vertex records as they are after the two calls,
// framebuffer bytes, z-buffer.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

struct Reader {
    std::vector<unsigned char> buf; size_t pos = 0;
    bool load(const char* p) { std::ifstream in(p, std::ios::binary); if (!in) return false; buf.assign(std::istreambuf_iterator<char>(in), {}); return true; }
    template <class T> T get() { T v; std::memcpy(&v, &buf[pos], sizeof(T)); pos += sizeof(T); return v; }
    void read(void* dst, size_t n) { std::memcpy(dst, &buf[pos], n); pos += n; }
};

struct Vertex { vec3 position, normal; vec2 texcoord; vec3 tangent, bitangent; };      // model.h:14-20
struct Model {
    std::vector<Vertex> vertices;
    std::vector<unsigned int> indices;
    AABB localAABB;
    int nfaces() const { return int(indices.size() / 3); }
    vec3 vert(int f, int v) const { return vertices[indices[f * 3 + v]].position; }
    vec3 normal(int f, int v) const { return vertices[indices[f * 3 + v]].normal; }
    vec2 uv(int f, int v) const { return vertices[indices[f * 3 + v]].texcoord; }
    int diffuse_slot() const { return -1; }
    int normal_slot() const { return -1; }
    int specular_slot() const { return -1; }
};
using PhongShader = PhongShaderT<Model>;

static mat<4, 4> read_mat(Reader& r) { mat<4, 4> m; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[i][j] = r.get<double>(); return m; }

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: demo_mesh_attr <scene.bin> <out.bin>\n"); return 1; }
    Reader r;
    if (!r.load(argv[1]) || std::memcmp(&r.buf[0], "TRGSCN01", 8) != 0) { std::fprintf(stderr, "bad scene file\n"); return 2; }
    r.pos = 8;
    const int WIDTH = r.get<int32_t>(), HEIGHT = r.get<int32_t>(), bpp = r.get<int32_t>(); r.get<int32_t>();
    const mat<4, 4> view = read_mat(r), proj = read_mat(r);
    vec3 key_light_dir, fill_light_dir, rim_light_dir;
    for (int i = 0; i < 3; ++i) key_light_dir[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) fill_light_dir[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) rim_light_dir[i] = r.get<double>();
    static_assert(sizeof(Vertex) == 14 * sizeof(double), "Vertex must be 14 packed doubles");
    Model model;
    const int nv = r.get<int32_t>(), nf = r.get<int32_t>();
    const mat<4, 4> modelMatrix = read_mat(r);
    model.vertices.resize(nv); model.indices.resize(size_t(nf) * 3);
    r.read(model.vertices.data(), size_t(nv) * sizeof(Vertex));
    r.read(model.indices.data(), model.indices.size() * 4);

    const int32_t generated[2] = { gl_mesh_normals(model), gl_mesh_tangents(model) };   // model.cpp:59,62
    model.localAABB = gl_mesh_bounds(model);                                             // model.cpp:65

    TGAImage framebuffer(WIDTH, HEIGHT, bpp);
    init_zbuffer(WIDTH, HEIGHT);
    ModelView = view * modelMatrix;
    Perspective = proj;
    init_viewport(0, 0, WIDTH, HEIGHT);
    PhongShader shader(&model);
    shader.initLightDirections(key_light_dir, fill_light_dir, rim_light_dir);
    gl_draw_model(model, shader, framebuffer);
    if (!gl_flush(framebuffer)) {
        std::fprintf(stderr, "demo_mesh_attr: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 4;
    }
    // a model whose last index names no vertex: the call is refused, nothing is written, and the shim tells why
    Model broken = model;
    broken.indices.back() = (unsigned int)broken.vertices.size();
    const int32_t refused[2] = { gl_mesh_normals(broken), gl_last_error() };
    std::fprintf(stderr, "demo_mesh_attr: refused as expected: %s\n", gl_last_error_message());
    gl_clear_error();
    std::ofstream out(argv[2], std::ios::binary);
    out.write(reinterpret_cast<const char*>(generated), sizeof generated);
    out.write(reinterpret_cast<const char*>(refused), sizeof refused);
    out.write(reinterpret_cast<const char*>(model.vertices.data()), std::streamsize(model.vertices.size() * sizeof(Vertex)));
    out.write(reinterpret_cast<const char*>(framebuffer.buffer()), std::streamsize(size_t(WIDTH) * HEIGHT * bpp));
    const std::vector<double>& depths = zbuffer;
    out.write(reinterpret_cast<const char*>(depths.data()), std::streamsize(depths.size() * 8));
    gl_shutdown();
    return out ? 0 : 3;
}
