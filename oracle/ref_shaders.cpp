// ref_shaders.cpp — TEST INFRASTRUCTURE, NOT PRODUCT.
//
// The second reference binary (oracle/_ref/ref_shaders).  Where oracle/ref_harness.cpp shades PHONG / EYE draws with the
// C restatement, this one links the reference's own main.cpp, model.cpp, model_manager.cpp, our_gl.cpp and tgaimage.cpp,
// compiled in place from the reference tree (oracle/Makefile; nothing of the reference is copied here), and calls the
// reference's own code for everything the restatement oracle/trgl_oracle.c restates from main.cpp and model.cpp:
//   PhongShader / EyeShader ::fragment (main.cpp:92-170, 220-261) and ::initLightDirections (main.cpp:55-69, 187-197),
//   ::vertex (main.cpp:71-90, 199-218), save_zbuffer_image and compute_ssao_at (main.cpp:269-362), and the samplers
//   Model::diffuse / normal / specular (model.cpp:415-459) behind them.
//
// model.h includes Assimp, which is not available here: oracle/assimp_standin/ holds declarations of the names model.cpp
// uses and nothing else.  Assimp::Importer::ReadFile (defined below) returns a scene this harness fills in: one root node,
// one material without textures and, in mode "mesh", one mesh.  The material sends Model::loadTexture to its fallback files
// <stem>_diffuse.tga / _nm.tga / _spec.tga (model.cpp:230-266), which the harness writes into a temporary directory with the
// reference's own TGAImage::write_tga_file (rows top-down, checked
// to read back unchanged); the reference's read_tga_file, samplers and TGAImage::get do the rest.
//
// Modes (one process per scene: the reference's diagnostic counters are file-static, our_gl.cpp:18-22):
//   scene  <in> <out>   a frame, input and output as `ref_harness scene`; PHONG / EYE draws use the reference's shaders with
//                       their varying_* members set per triangle, ModelView, the eye-space light directions and
//                       normal_map_strength set from the draw's uniforms
//   frag   <in> <out>   single fragment() calls: per item kind, uniforms, 24 varyings, bary -> bgra[4], bytespp
//   lights <in> <out>   initLightDirections from world directions under a ModelView -> the eye-space directions
//   mesh   <in> <out>   a mesh handed to ReadFile, Model::load, shader.vertex(f, v) for every face, then rasterize() as
//                       main.cpp:692-698 does -> clip, varyings and the frame
//   zimage <in> <out>   save_zbuffer_image over a z-buffer, read back with TGAImage::read_tga_file (rows as it set them)
//   ssao   <in> <out>   compute_ssao_at over a z-buffer, in the loop of main.cpp:756-763

#define main reference_main_unused
#include "main.cpp"          // from -I<reference tree>
#undef main

#include "ref_scene.h"

#include <filesystem>
#include <map>
#include <memory>
#include <tuple>
#include <unistd.h>

// ---- the Importer declared in oracle/assimp_standin/assimp/Importer.hpp -------------------------------------------------------
namespace {
aiScene* g_scene = nullptr;            // what the next ReadFile returns
}
const aiScene* Assimp::Importer::ReadFile(const std::string&, unsigned int) { return g_scene; }
void Assimp::Importer::FreeScene() {}
const char* Assimp::Importer::GetErrorString() const { return "ref_shaders: no scene"; }

namespace {

using refscene::Reader;

struct TempDir {
    std::string path;
    TempDir() {
        char tmpl[] = "/tmp/ref_shaders_XXXXXX";
        if (!mkdtemp(tmpl)) { std::perror("mkdtemp"); std::exit(4); }
        path = tmpl;
    }
    ~TempDir() { std::error_code ec; std::filesystem::remove_all(path, ec); }
};

// A mesh in the layout aiMesh points at (float, as Assimp's aiVector3D).
struct MeshData {
    std::vector<aiVector3D> pos, nrm, uv;
    std::vector<unsigned int> idx;
    std::vector<aiFace> faces;
};

bool has_texels(const std::vector<orc_texture>& tex, int slot) {
    return !(slot < 0 || slot >= (int)tex.size() || !tex[slot].data || tex[slot].w <= 0);
}

// Model::load over the harness's scene.  tex[slot] for the diffuse / normal / specular slots (a slot outside the table or
// without texels: no file, so the material has no such map, as trgl's slot -1).
std::unique_ptr<Model> load_model(const std::string& dir, const std::string& stem, const std::vector<orc_texture>& tex,
                                  int sd, int sn, int ss, MeshData* mesh) {
    const struct { int slot; const char* suffix; } maps[3] = { { sd, "_diffuse.tga" }, { sn, "_nm.tga" }, { ss, "_spec.tga" } };
    for (const auto& m : maps) {
        if (!has_texels(tex, m.slot)) continue;
        const orc_texture& t = tex[m.slot];
        TGAImage img(t.w, t.h, t.bpp);
        std::memcpy(img.buffer(), t.data, (size_t)t.w * t.h * t.bpp);
        // vflip = false: the default (true) marks the file bottom-up without reordering the rows, and read_tga_file would
        // hand the texture back flipped (tgaimage.cpp:118, 176)
        if (!img.write_tga_file(dir + "/" + stem + m.suffix, false)) { std::fprintf(stderr, "cannot write texture\n"); std::exit(4); }
    }
    aiNode root; aiMaterial material; aiMaterial* materials[1] = { &material };
    aiMesh ai_mesh; aiMesh* meshes[1] = { &ai_mesh }; unsigned int mesh_ids[1] = { 0 };
    aiScene scene;
    scene.mRootNode = &root;
    scene.mNumMaterials = 1; scene.mMaterials = materials;
    if (mesh) {
        ai_mesh.mNumVertices = (unsigned)mesh->pos.size();
        ai_mesh.mVertices = mesh->pos.data(); ai_mesh.mNormals = mesh->nrm.data(); ai_mesh.mTextureCoords[0] = mesh->uv.data();
        mesh->faces.resize(mesh->idx.size() / 3);
        for (size_t f = 0; f < mesh->faces.size(); ++f) { mesh->faces[f].mNumIndices = 3; mesh->faces[f].mIndices = &mesh->idx[3 * f]; }
        ai_mesh.mNumFaces = (unsigned)mesh->faces.size(); ai_mesh.mFaces = mesh->faces.data();
        scene.mNumMeshes = 1; scene.mMeshes = meshes;
        root.mNumMeshes = 1; root.mMeshes = mesh_ids;
    }
    g_scene = &scene;
    auto model = std::make_unique<Model>(dir + "/" + stem + ".obj");
    const bool ok = model->load();
    g_scene = nullptr;
    if (!ok) { std::fprintf(stderr, "Model::load failed\n"); std::exit(4); }
    // the textures went through write_tga_file + read_tga_file: they must have come back unchanged
    const TGAImage* back[3] = { &model->getMaterial(0).diffuse, &model->getMaterial(0).normal, &model->getMaterial(0).specular };
    for (int k = 0; k < 3; ++k) {
        if (!has_texels(tex, maps[k].slot)) {
            if (back[k]->width() > 0) { std::fprintf(stderr, "unexpected texture\n"); std::exit(5); }
            continue;
        }
        const orc_texture& t = tex[maps[k].slot];
        if (back[k]->width() != t.w || back[k]->height() != t.h) { std::fprintf(stderr, "texture size changed\n"); std::exit(5); }
        for (int y = 0; y < t.h; ++y) for (int x = 0; x < t.w; ++x) {
            TGAColor c = back[k]->get(x, y);
            if (c.bytespp != t.bpp || std::memcmp(c.bgra, t.data + ((size_t)x + (size_t)y * t.w) * t.bpp, t.bpp) != 0) {
                std::fprintf(stderr, "texture bytes changed\n"); std::exit(5);
            }
        }
    }
    return model;
}

// One Model per (diffuse, normal, specular) slot triple, all from one temporary directory.
struct Models {
    TempDir dir;
    std::map<std::tuple<int, int, int>, std::unique_ptr<Model>> cache;
    const Model* get(const trgl_uniforms& u, const std::vector<orc_texture>& tex) {
        auto key = std::make_tuple(u.tex_diffuse, u.tex_normal, u.tex_specular);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second.get();
        std::string stem = "m" + std::to_string(cache.size());
        return (cache[key] = load_model(dir.path, stem, tex, u.tex_diffuse, u.tex_normal, u.tex_specular, nullptr)).get();
    }
};

vec3 v3(const double* p) { vec3 v; v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; return v; }

void set_model_view(const trgl_uniforms& u) {
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) ModelView[i][j] = u.model_view[i * 4 + j];
}

// varying_uv[3], varying_position_eye[3], varying_normal_eye[3] from the 24 varyings of include/trgl.h
template <class S> void set_varyings(S& s, const double* vary) {
    for (int v = 0; v < 3; ++v) {
        s.varying_uv[v][0] = vary[2 * v]; s.varying_uv[v][1] = vary[2 * v + 1];
        s.varying_position_eye[v] = v3(vary + 6 + 3 * v);
        s.varying_normal_eye[v] = v3(vary + 15 + 3 * v);
    }
}

// The uniforms' eye-space light directions and normal_map_strength (PHONG), set directly on the shader's public members.
void set_lights(PhongShader& s, const trgl_uniforms& u) {
    s.key_light_dir_eye = v3(u.key_light_dir_eye); s.fill_light_dir_eye = v3(u.fill_light_dir_eye);
    s.rim_light_dir_eye = v3(u.rim_light_dir_eye); s.normal_map_strength = u.normal_map_strength;
}
void set_lights(EyeShader& s, const trgl_uniforms& u) {
    s.key_light_dir_eye = v3(u.key_light_dir_eye); s.rim_light_dir_eye = v3(u.rim_light_dir_eye);
}

// PHONG / EYE draws of a scene with the reference's shaders.  ModelView is a global of our_gl.cpp read by PhongShader::fragment
// (main.cpp:116): each draw sets it from its uniforms.
struct ReferenceLit {
    Models models;
    std::unique_ptr<PhongShader> phong;
    std::unique_ptr<EyeShader> eye;
    bool is_phong = true;
    void draw(int kind, const trgl_uniforms& u, const std::vector<orc_texture>& tex) {
        const Model* m = models.get(u, tex);
        set_model_view(u);
        is_phong = kind == TRGL_SHADER_PHONG;
        if (is_phong) { phong = std::make_unique<PhongShader>(m); set_lights(*phong, u); }
        else { eye = std::make_unique<EyeShader>(m); set_lights(*eye, u); }
    }
    const IShader& triangle(const double* vary) {
        if (is_phong) { set_varyings(*phong, vary); return *phong; }
        set_varyings(*eye, vary); return *eye;
    }
};

int run_scene(const char* in_path, const char* out_path) {
    ReferenceLit lit;
    return refscene::run_scene(in_path, out_path, lit);
}

std::vector<orc_texture> read_textures(Reader& r, int ntex) {
    std::vector<orc_texture> tex(TRGL_MAX_TEXTURES, orc_texture{ nullptr, 0, 0, 0 });
    for (int t = 0; t < ntex; ++t) {
        int slot = r.get<int32_t>(), w = r.get<int32_t>(), h = r.get<int32_t>(), tb = r.get<int32_t>();
        tex[slot] = orc_texture{ r.take((size_t)w * h * tb), w, h, tb };
        r.align8();
    }
    return tex;
}

// frag: input "TRGFRG01", int32 ntex, count; textures as in a scene file; per item int32 kind, pad, trgl_uniforms, 24 + 3
// doubles (varyings, bary).  Output per item: bgra[4], bytespp, discard, 2 pad bytes.
int run_frag(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path) || std::memcmp(r.take(8), "TRGFRG01", 8) != 0) return 2;
    int ntex = r.get<int32_t>(), count = r.get<int32_t>();
    std::vector<orc_texture> tex = read_textures(r, ntex);
    Models models;
    std::ofstream out(out_path, std::ios::binary);
    for (int i = 0; i < count; ++i) {
        int kind = r.get<int32_t>(); r.get<int32_t>();
        trgl_uniforms u; std::memcpy(&u, r.take(sizeof(u)), sizeof(u));
        const double* vary = (const double*)r.take(24 * sizeof(double));
        vec3 bar = v3((const double*)r.take(3 * sizeof(double)));
        const Model* m = models.get(u, tex);
        set_model_view(u);
        std::pair<bool, TGAColor> res;
        if (kind == TRGL_SHADER_PHONG) {
            PhongShader s(m); set_lights(s, u); set_varyings(s, vary);
            res = s.fragment(bar);
        } else {
            EyeShader s(m); set_lights(s, u); set_varyings(s, vary);
            res = s.fragment(bar);
        }
        unsigned char rec[8] = { res.second.bgra[0], res.second.bgra[1], res.second.bgra[2], res.second.bgra[3],
                                 res.second.bytespp, (unsigned char)res.first, 0, 0 };
        out.write((const char*)rec, 8);
    }
    return out ? 0 : 3;
}

// lights: input int32 count, pad; per item ModelView[16], key, fill, rim [3 each] in world space.  Output per item:
// PhongShader::initLightDirections(key, fill, rim) -> key, fill, rim eye [9 doubles], EyeShader::initLightDirections(key, rim)
// -> key, rim eye [6 doubles].
int run_lights(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path)) return 2;
    int count = r.get<int32_t>(); r.get<int32_t>();
    std::ofstream out(out_path, std::ios::binary);
    for (int i = 0; i < count; ++i) {
        for (int a = 0; a < 4; ++a) for (int c = 0; c < 4; ++c) ModelView[a][c] = r.get<double>();
        vec3 k = v3((const double*)r.take(24)), f = v3((const double*)r.take(24)), rim = v3((const double*)r.take(24));
        PhongShader p(nullptr); p.initLightDirections(k, f, rim);
        EyeShader e(nullptr); e.initLightDirections(k, rim);
        const vec3 o[5] = { p.key_light_dir_eye, p.fill_light_dir_eye, p.rim_light_dir_eye, e.key_light_dir_eye, e.rim_light_dir_eye };
        for (const vec3& v : o) for (int c = 0; c < 3; ++c) { double d = v[c]; out.write((const char*)&d, 8); }
    }
    return out ? 0 : 3;
}

// mesh: input "TRGMSH01", int32 W, H, bpp, kind, ntex, nverts, nfaces, pad; Viewport[16], Perspective[16] doubles;
// trgl_uniforms (ModelView, eye-space lights, strength, texture slots); textures as in a scene file; nverts x 8 floats
// (position, normal, uv); nfaces x 3 uint32.  Output: nfaces x 12 clip doubles, nfaces x 24 varyings, then the frame as
// `scene` writes it (cleared to TGAColor(), z to +inf).
int run_mesh(const char* in_path, const char* out_path) {
    Reader r;
    if (!r.load(in_path) || std::memcmp(r.take(8), "TRGMSH01", 8) != 0) return 2;
    int W = r.get<int32_t>(), H = r.get<int32_t>(), bpp = r.get<int32_t>(), kind = r.get<int32_t>();
    int ntex = r.get<int32_t>(), nverts = r.get<int32_t>(), nfaces = r.get<int32_t>(); r.get<int32_t>();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Viewport[i][j] = r.get<double>();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Perspective[i][j] = r.get<double>();
    trgl_uniforms u; std::memcpy(&u, r.take(sizeof(u)), sizeof(u));
    std::vector<orc_texture> tex = read_textures(r, ntex);
    MeshData mesh;
    const float* vf = (const float*)r.take((size_t)nverts * 8 * sizeof(float));
    for (int v = 0; v < nverts; ++v) {
        const float* p = vf + 8 * v;
        mesh.pos.push_back(aiVector3D{ p[0], p[1], p[2] });
        mesh.nrm.push_back(aiVector3D{ p[3], p[4], p[5] });
        mesh.uv.push_back(aiVector3D{ p[6], p[7], 0.0f });
    }
    const uint32_t* ix = (const uint32_t*)r.take((size_t)nfaces * 3 * sizeof(uint32_t));
    mesh.idx.assign(ix, ix + (size_t)nfaces * 3);

    TempDir dir;
    std::unique_ptr<Model> model = load_model(dir.path, "mesh", tex, u.tex_diffuse, u.tex_normal, u.tex_specular, &mesh);
    if (model->nfaces() != nfaces) { std::fprintf(stderr, "face count changed\n"); return 5; }
    set_model_view(u);

    TGAImage framebuffer(W, H, bpp);
    init_zbuffer(W, H);
    std::vector<double> clip((size_t)nfaces * 12), vary((size_t)nfaces * 24);
    PhongShader phong(model.get()); set_lights(phong, u);
    EyeShader eye(model.get()); set_lights(eye, u);
    const bool is_phong = kind == TRGL_SHADER_PHONG;
    IShader& shader = is_phong ? (IShader&)phong : (IShader&)eye;
    for (int f = 0; f < nfaces; ++f) {
        vec4 tri[3];
        for (int v = 0; v < 3; ++v) tri[v] = shader.vertex(f, v);
        double* o = &vary[(size_t)f * 24];
        for (int v = 0; v < 3; ++v) {
            for (int c = 0; c < 4; ++c) clip[(size_t)f * 12 + v * 4 + c] = tri[v][c];
            const vec2& uv = is_phong ? phong.varying_uv[v] : eye.varying_uv[v];
            const vec3& pe = is_phong ? phong.varying_position_eye[v] : eye.varying_position_eye[v];
            const vec3& ne = is_phong ? phong.varying_normal_eye[v] : eye.varying_normal_eye[v];
            o[2 * v] = uv[0]; o[2 * v + 1] = uv[1];
            for (int c = 0; c < 3; ++c) { o[6 + 3 * v + c] = pe[c]; o[15 + 3 * v + c] = ne[c]; }
        }
        rasterize(tri, shader, framebuffer);
    }
    const std::string frame_path = dir.path + "/frame.bin";
    int rc = refscene::write_scene_output(frame_path.c_str(), framebuffer, W, H, bpp, 0.0);
    if (rc) return rc;
    std::ifstream in(frame_path, std::ios::binary);
    std::ofstream out(out_path, std::ios::binary);
    out.write((const char*)clip.data(), clip.size() * 8);
    out.write((const char*)vary.data(), vary.size() * 8);
    out << in.rdbuf();
    return out ? 0 : 3;
}

// zimage / ssao: input int32 W, H + W*H doubles; output W*H*3 bytes.
int run_zbuffer(const char* in_path, const char* out_path, bool ssao) {
    Reader r;
    if (!r.load(in_path)) return 2;
    int W = r.get<int32_t>(), H = r.get<int32_t>();
    std::vector<double> z((size_t)W * H);
    std::memcpy(z.data(), r.take(z.size() * 8), z.size() * 8);
    TGAImage img;
    if (!ssao) {
        TempDir dir;
        const std::string path = dir.path + "/zbuffer.tga";
        save_zbuffer_image(z, W, H, path.c_str());
        if (!img.read_tga_file(path)) return 4;
        // write_tga_file's default vflip marks the file bottom-up without reordering the rows (tgaimage.cpp:176), so reading
        // it flips them (tgaimage.cpp:118): flip back to the image save_zbuffer_image built
        img.flip_vertically();
    } else {
        img = TGAImage(W, H, TGAImage::RGB);
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {                // main.cpp:757-763
            double ao_value = compute_ssao_at(z, W, H, x, y);
            unsigned char intensity = (unsigned char)(255.0 * ao_value);
            img.set(x, y, TGAColor(intensity, intensity, intensity));
        }
    }
    if (img.width() != W || img.height() != H || img.get(0, 0).bytespp != 3) return 5;
    std::ofstream out(out_path, std::ios::binary);
    out.write((const char*)img.buffer(), (std::streamsize)W * H * 3);
    return out ? 0 : 3;
}

}  // namespace

int main(int argc, char** argv) {
    std::cout.rdbuf(nullptr);            // Model::load's progress lines
    if (argc == 4 && std::strcmp(argv[1], "scene") == 0) return run_scene(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "frag") == 0) return run_frag(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "lights") == 0) return run_lights(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "mesh") == 0) return run_mesh(argv[2], argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "zimage") == 0) return run_zbuffer(argv[2], argv[3], false);
    if (argc == 4 && std::strcmp(argv[1], "ssao") == 0) return run_zbuffer(argv[2], argv[3], true);
    std::fprintf(stderr, "usage: ref_shaders scene|frag|lights|mesh|zimage|ssao <in> <out>\n");
    return 1;
}
