// demo_scene.cpp — the scene logic of the reference's render section (main.cpp:555-557,606-799) around the MI355X rasterizer: three
// models with model matrices, getWorldAABB -> frustum.intersects -> draw or count as culled, the depth snapshot around the eyes,
// the post-process and the culling statistics.  Same globals and names as main.cpp, through the shim headers.
//   demo_scene <scene.bin> <out.bin>
// scene.bin is written by tests/test_scene_demo.py (procedural models: the reference's obj/ assets are absent).  out.bin = framebuffer
// bytes, z-buffer, the three post-process images, then the stats line and the culling statistics as text.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

struct Reader {
    std::vector<unsigned char> buf; size_t pos = 0;
    bool load(const char* p) { std::ifstream in(p, std::ios::binary); if (!in) return false; buf.assign(std::istreambuf_iterator<char>(in), {}); return true; }
    template <class T> T get() { T v; std::memcpy(&v, &buf[pos], sizeof(T)); pos += sizeof(T); return v; }
    void read(void* dst, size_t n) { std::memcpy(dst, &buf[pos], n); pos += n; }
    void align8() { pos = (pos + 7) & ~size_t(7); }
};

// stands in for the reference's Model (model.h:46-131): the indexed mesh (Vertex = model.h:14-20), no texture maps, and the box
// that Model::load leaves in localAABB
struct Vertex { vec3 position, normal; vec2 texcoord; vec3 tangent, bitangent; };
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
    AABB getWorldAABB(const mat<4, 4>& modelMatrix) const { return localAABB.transform(modelMatrix); }   // model.h:94-96
};
using PhongShader = PhongShaderT<Model>;
using EyeShader = EyeShaderT<Model>;

static mat<4, 4> read_mat(Reader& r) { mat<4, 4> m; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[i][j] = r.get<double>(); return m; }
static void read_model(Reader& r, Model& m, mat<4, 4>& modelMatrix) {
    static_assert(sizeof(Vertex) == 14 * sizeof(double), "Vertex must be 14 packed doubles");
    const int nv = r.get<int32_t>(), nf = r.get<int32_t>();
    modelMatrix = read_mat(r);
    m.vertices.resize(nv); m.indices.resize(size_t(nf) * 3);
    r.read(m.vertices.data(), size_t(nv) * sizeof(Vertex));
    r.read(m.indices.data(), m.indices.size() * 4); r.align8();
    m.localAABB = gl_mesh_bounds(m);                             // Model::computeAABB, model.cpp:15-40
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: demo_scene <scene.bin> <out.bin>\n"); return 1; }
    Reader r;
    if (!r.load(argv[1]) || std::memcmp(&r.buf[0], "TRGSCN01", 8) != 0) { std::fprintf(stderr, "bad scene file\n"); return 2; }
    r.pos = 8;
    const int WIDTH = r.get<int32_t>(), HEIGHT = r.get<int32_t>(), bpp = r.get<int32_t>(); r.get<int32_t>();
    const mat<4, 4> view = read_mat(r), proj = read_mat(r);
    vec3 key_light_dir, fill_light_dir, rim_light_dir;
    for (int i = 0; i < 3; ++i) key_light_dir[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) fill_light_dir[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) rim_light_dir[i] = r.get<double>();
    Model sponza_model, head_model, eye_model;
    mat<4, 4> sponzaModelMatrix, headModelMatrix, eyeModelMatrix;
    read_model(r, sponza_model, sponzaModelMatrix);
    read_model(r, head_model, headModelMatrix);
    read_model(r, eye_model, eyeModelMatrix);

    // ---- main.cpp:555-557 ----
    AABB sponzaWorldAABB = sponza_model.getWorldAABB(sponzaModelMatrix);
    AABB headWorldAABB = head_model.getWorldAABB(headModelMatrix);
    AABB eyeWorldAABB = eye_model.getWorldAABB(eyeModelMatrix);

    // ---- main.cpp:606-612 ----
    TGAImage framebuffer(WIDTH, HEIGHT, bpp);
    init_zbuffer(WIDTH, HEIGHT);
    ModelView = view;
    Perspective = proj;
    init_viewport(0, 0, WIDTH, HEIGHT);

    // ---- main.cpp:623-629 ----
    mat<4, 4> viewProjection = Perspective * ModelView;
    Frustum frustum = Frustum::createFromMatrix(viewProjection);
    int models_culled = 0, models_rendered = 0, total_triangles = 0, culled_triangles = 0;

    // ---- sponza, main.cpp:647-674 ----
    if (frustum.intersects(sponzaWorldAABB)) {
        models_rendered++;
        mat<4, 4> originalModelView = ModelView;
        ModelView = ModelView * sponzaModelMatrix;
        PhongShader sponza_shader(&sponza_model);
        sponza_shader.initLightDirections(key_light_dir, fill_light_dir, rim_light_dir);
        sponza_shader.normal_map_strength = 0.5;
        total_triangles += sponza_model.nfaces();
        gl_draw_model(sponza_model, sponza_shader, framebuffer);           // the face loop of main.cpp:660-666
        ModelView = originalModelView;
    } else {
        models_culled++;
        culled_triangles += sponza_model.nfaces();
    }

    // ---- head and eyes, main.cpp:680-736 ----
    if (frustum.intersects(headWorldAABB)) {
        models_rendered++;
        mat<4, 4> originalModelView = ModelView;
        ModelView = ModelView * headModelMatrix;
        PhongShader head_shader(&head_model);
        head_shader.initLightDirections(key_light_dir, fill_light_dir, rim_light_dir);
        total_triangles += head_model.nfaces();
        gl_draw_model(head_model, head_shader, framebuffer);               // main.cpp:692-698

        gl_zbuffer_snapshot(framebuffer, 0);                               // main.cpp:700, without the depths leaving the device

        if (frustum.intersects(eyeWorldAABB)) {                            // (main.cpp:706 tests the head's box again; the eyes have their own here)
            models_rendered++;
            ModelView = originalModelView * eyeModelMatrix;                // (main.cpp:513 makes the eyes' matrix the head's and keeps ModelView)
            EyeShader eye_shader(&eye_model);
            eye_shader.initLightDirections(key_light_dir, rim_light_dir);
            total_triangles += eye_model.nfaces();
            gl_draw_model(eye_model, eye_shader, framebuffer);             // main.cpp:715-721
        } else {
            models_culled++;
            culled_triangles += eye_model.nfaces();
        }
        ModelView = originalModelView;
        gl_zbuffer_restore(framebuffer, 0);                                // main.cpp:730: SSAO sees the depths without the eyes
    } else {
        models_culled++;
        culled_triangles += head_model.nfaces();
    }

    if (!gl_flush(framebuffer)) {                                          // before main.cpp:743 reads the pixels
        std::fprintf(stderr, "demo_scene: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 4;
    }
    TGAImage zimg, ao_map, final_result;                                   // main.cpp:751-785
    if (!gl_postprocess(framebuffer, &zimg, &ao_map, &final_result)) {
        std::fprintf(stderr, "demo_scene: %s (code %d)\n", gl_last_error_message(), gl_last_error());
        return 4;
    }

    trgl_stats st{};
    trgl_get_stats(trgl_shim::state().ctx, &st);
    char line[512];
    trgl_format_stats(&st, line, sizeof line);
    print_render_stats();                                                  // main.cpp:792

    std::ostringstream cull;                                               // main.cpp:794-799
    cull << "\n=== Frustum Culling Statistics ===" << std::endl;
    cull << "  Total models: " << (models_rendered + models_culled) << std::endl;
    cull << "  Models rendered: " << models_rendered << std::endl;
    cull << "  Models culled: " << models_culled << std::endl;
    cull << "  Total triangles: " << total_triangles << std::endl;
    cull << "  Culled triangles: " << culled_triangles << std::endl;
    std::cout << cull.str();

    std::ofstream out(argv[2], std::ios::binary);
    const size_t npx = size_t(WIDTH) * HEIGHT;
    out.write(reinterpret_cast<const char*>(framebuffer.buffer()), std::streamsize(npx * bpp));
    const std::vector<double>& depths = zbuffer;                           // (the proxy fetches the restored depths)
    out.write(reinterpret_cast<const char*>(depths.data()), std::streamsize(depths.size() * 8));
    for (TGAImage* img : { &zimg, &ao_map, &final_result }) out.write(reinterpret_cast<const char*>(img->buffer()), std::streamsize(npx * 3));
    out.write(line, std::streamsize(std::strlen(line)));
    out << cull.str();
    gl_shutdown();
    return out ? 0 : 3;
}
