// shim_program — runs one program of tests/shim_programs.py through the shim's public names, written the way a main.cpp-shaped
// caller writes them: the globals ModelView / Perspective / Viewport / zbuffer, rasterize() in a loop over triangles, direct uses of
// zbuffer, gl_flush() in front of the places that read pixels.  Every observation goes to the output file as a record
//     int32 tag, int32 operation index, uint64 byte count, bytes
// and print_render_stats() writes its line to stderr, where the test reads it.  The program file is the binary form that
// shim_programs.encode() makes of a program: int32 opcode, then the fields and arrays of the operation.
//     shim_program <program.bin> <observations.bin>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../tinyrenderder_amd/shim/trgl_shaders.h"

enum Op { END = 0, IMAGE, REGISTER_SHADER, RASTERIZE, MODELVIEW, INIT_VIEWPORT, Z_READ, Z_WRITE, Z_COPY, Z_SAVE, Z_LOAD, Z_ITER, Z_SIZE, Z_REF, INIT_ZBUFFER,
          FLUSH, FB_SET, FB_MODIFIED, UPLOAD_TEXTURE, CLIP_PLANE, DRAW_INDEXED, STATS, DUMP };
enum Tag { T_IMAGE = 1, T_DEPTHS, T_DOUBLE, T_SIZE, T_KIND, T_ERROR };
enum Kind { K_FLAT = 0, K_GOURAUD = 1, K_PHONG = 2, K_CHECKER = 4, K_USER = 100 };

struct Reader {
    std::vector<unsigned char> buf; size_t pos = 0;
    bool load(const char* p) {
        FILE* f = std::fopen(p, "rb"); if (!f) return false;
        std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        buf.resize(size_t(n)); const bool ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size(); std::fclose(f); return ok;
    }
    void read(void* d, size_t n) {
        if (pos + n > buf.size()) { std::fprintf(stderr, "shim_program: the program file ends inside an operation\n"); std::exit(3); }
        std::memcpy(d, &buf[pos], n); pos += n;
    }
    template <class T> T get() { T v; read(&v, sizeof v); return v; }
    template <class T> std::vector<T> array(size_t n) { std::vector<T> v(n); if (n) read(v.data(), n * sizeof(T)); return v; }
};

static FILE* g_out = nullptr;
static void record(int tag, int op, const void* bytes, size_t n) {
    const int32_t head[2] = { tag, op };
    const uint64_t size = n;
    std::fwrite(head, sizeof head, 1, g_out); std::fwrite(&size, sizeof size, 1, g_out);
    if (n) std::fwrite(bytes, 1, n, g_out);
}
static void record_image(int op, bool ok, TGAImage& img) {
    std::vector<unsigned char> b(8 + size_t(img.width()) * img.height() * img.bytespp());
    const int32_t head[2] = { ok ? 1 : 0, gl_last_error() };
    std::memcpy(b.data(), head, 8);
    if (b.size() > 8) std::memcpy(b.data() + 8, img.buffer(), b.size() - 8);
    record(T_IMAGE, op, b.data(), b.size());
}

// what PhongShaderT asks of a model: the slots of its maps (the driver sets the varyings itself, so vertex() is never called)
struct Maps {
    int slot[3] = { -1, -1, -1 };
    vec3 vert(int, int) const { return vec3(); }
    vec3 normal(int, int) const { return vec3(); }
    vec2 uv(int, int) const { return vec2(); }
    int diffuse_slot() const { return slot[0]; }
    int normal_slot() const { return slot[1]; }
    int specular_slot() const { return slot[2]; }
};
using PhongShader = PhongShaderT<Maps>;

static void read_phong(Reader& r, PhongShader& shader, Maps& maps) {
    for (int i = 0; i < 3; ++i) shader.key_light_dir_eye[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) shader.fill_light_dir_eye[i] = r.get<double>();
    for (int i = 0; i < 3; ++i) shader.rim_light_dir_eye[i] = r.get<double>();
    shader.normal_map_strength = r.get<double>();
    for (int i = 0; i < 3; ++i) maps.slot[i] = r.get<int32_t>();
}
static TGAColor color_of(uint32_t bgra) {
    unsigned char b[4] = { (unsigned char)(bgra), (unsigned char)(bgra >> 8), (unsigned char)(bgra >> 16), (unsigned char)(bgra >> 24) };
    return TGAColor(b, 4);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: shim_program <program.bin> <observations.bin>\n"); return 1; }
    Reader r;
    if (!r.load(argv[1]) || r.buf.size() < 8 || std::memcmp(r.buf.data(), "SHIMPRG1", 8) != 0) { std::fprintf(stderr, "bad program file\n"); return 2; }
    r.pos = 8;
    g_out = std::fopen(argv[2], "wb");
    if (!g_out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }

    std::map<int, TGAImage> images;
    std::vector<int> user_kinds;
    std::vector<double> saved;

    for (int op = 0;; ++op) {
        const int code = r.get<int32_t>();
        if (code == END) break;
        switch (code) {
        case IMAGE: {
            const int id = r.get<int32_t>(), w = r.get<int32_t>(), h = r.get<int32_t>(), bpp = r.get<int32_t>();
            unsigned char fill[4]; r.read(fill, 4);
            images[id] = TGAImage(w, h, bpp, TGAColor(fill, (unsigned char)bpp));
            break;
        }
        case REGISTER_SHADER: {
            const int K = r.get<int32_t>(), may_discard = r.get<int32_t>(), len = r.get<int32_t>();
            const std::vector<char> src = r.array<char>(size_t(len));
            const int32_t kind = gl_register_shader(std::string(src.begin(), src.end()).c_str(), K, may_discard != 0);
            user_kinds.push_back(kind);
            record(T_KIND, op, &kind, sizeof kind);
            break;
        }
        case RASTERIZE: {
            TGAImage& framebuffer = images.at(r.get<int32_t>());
            const int kind = r.get<int32_t>(), n = r.get<int32_t>(), cells = r.get<int32_t>();
            Maps maps; PhongShader phong(&maps);
            if (kind == K_PHONG) read_phong(r, phong, maps);
            const std::vector<double> clip = r.array<double>(size_t(n) * 12);
            const std::vector<uint32_t> colors = r.array<uint32_t>(size_t(n));
            const int K = kind == K_GOURAUD ? 3 : kind == K_PHONG ? 24 : 0;
            const std::vector<double> vary = r.array<double>(size_t(n) * K);
            FlatShader flat; GouraudShader gouraud; CheckerShader checker; UserShader user;
            for (int t = 0; t < n; ++t) {                           // the caller's face loop: one shader object, new members per triangle
                vec4 clip_space_triangle[3];
                for (int v = 0; v < 3; ++v) for (int k = 0; k < 4; ++k) clip_space_triangle[v][k] = clip[size_t(t) * 12 + 4 * v + k];
                if (kind == K_FLAT) { flat.color = color_of(colors[t]); rasterize(clip_space_triangle, flat, framebuffer); }
                else if (kind == K_GOURAUD) {
                    gouraud.base = color_of(colors[t]);
                    for (int v = 0; v < 3; ++v) gouraud.varying_intensity[v] = vary[size_t(t) * 3 + v];
                    rasterize(clip_space_triangle, gouraud, framebuffer);
                } else if (kind == K_CHECKER) { checker.color = color_of(colors[t]); checker.cells = cells; rasterize(clip_space_triangle, checker, framebuffer); }
                else if (kind == K_PHONG) {
                    static_assert(sizeof(phong.v) == 24 * sizeof(double), "the varyings block is 24 packed doubles");
                    std::memcpy(static_cast<void*>(&phong.v), &vary[size_t(t) * 24], sizeof(phong.v));
                    rasterize(clip_space_triangle, phong, framebuffer);
                } else {
                    user.kind = user_kinds.at(size_t(kind - K_USER)); user.color = color_of(colors[t]); user.uniforms.reserved = cells;
                    rasterize(clip_space_triangle, user, framebuffer);
                }
            }
            break;
        }
        case MODELVIEW:
            for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) ModelView[i][j] = r.get<double>();
            break;
        case INIT_VIEWPORT: {
            const int x = r.get<int32_t>(), y = r.get<int32_t>(), w = r.get<int32_t>(), h = r.get<int32_t>();
            init_viewport(x, y, w, h);
            break;
        }
        case Z_READ: { const int i = r.get<int32_t>(); double d = zbuffer[i]; record(T_DOUBLE, op, &d, sizeof d); break; }
        case Z_WRITE: { const int i = r.get<int32_t>(); const double v = r.get<double>(); zbuffer[i] = v; break; }
        case Z_COPY: { const int i = r.get<int32_t>(), j = r.get<int32_t>(); zbuffer[i] = zbuffer[j]; break; }
        case Z_SAVE: saved = zbuffer; break;
        case Z_LOAD: zbuffer = saved; break;
        case Z_ITER: {
            std::vector<double> seen;
            for (double d : zbuffer) seen.push_back(d);
            record(T_DEPTHS, op, seen.data(), seen.size() * sizeof(double));
            break;
        }
        case Z_SIZE: { const uint64_t n = zbuffer.size(); record(T_SIZE, op, &n, sizeof n); break; }
        case Z_REF: {
            const std::vector<double>& depths = zbuffer;
            record(T_DEPTHS, op, depths.data(), depths.size() * sizeof(double));
            break;
        }
        case INIT_ZBUFFER: { const int w = r.get<int32_t>(), h = r.get<int32_t>(); init_zbuffer(w, h); break; }
        case FLUSH: { TGAImage& framebuffer = images.at(r.get<int32_t>()); const bool ok = gl_flush(framebuffer); record_image(op, ok, framebuffer); break; }
        case FB_SET: {
            TGAImage& framebuffer = images.at(r.get<int32_t>());
            const int x = r.get<int32_t>(), y = r.get<int32_t>();
            unsigned char c[4]; r.read(c, 4);
            framebuffer.set(x, y, TGAColor(c, (unsigned char)framebuffer.bytespp()));
            break;
        }
        case FB_MODIFIED: gl_framebuffer_modified(images.at(r.get<int32_t>())); break;
        case UPLOAD_TEXTURE: {
            TGAImage& framebuffer = images.at(r.get<int32_t>());
            const int slot = r.get<int32_t>(), w = r.get<int32_t>(), h = r.get<int32_t>(), bpp = r.get<int32_t>();
            TGAImage texture(w, h, bpp);
            r.read(texture.buffer(), size_t(w) * h * bpp);
            gl_upload_texture(framebuffer, slot, texture);
            break;
        }
        case CLIP_PLANE: {
            const int on = r.get<int32_t>();
            vec4 plane; for (int k = 0; k < 4; ++k) plane[k] = r.get<double>();
            gl_clip_plane(on ? &plane : nullptr);
            break;
        }
        case DRAW_INDEXED: {
            TGAImage& framebuffer = images.at(r.get<int32_t>());
            Maps maps; PhongShader phong(&maps);
            read_phong(r, phong, maps);
            for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Perspective[i][j] = r.get<double>();
            const int stride = r.get<int32_t>(), nv = r.get<int32_t>(), nf = r.get<int32_t>();
            const std::vector<double> vertices = r.array<double>(size_t(nv) * stride);
            const std::vector<unsigned int> indices = r.array<unsigned int>(size_t(nf) * 3);
            gl_draw_indexed(phong, vertices.data(), stride, size_t(nv), indices.data(), size_t(nf), framebuffer);
            break;
        }
        case STATS: print_render_stats(); break;
        case DUMP: record_image(op, true, images.at(r.get<int32_t>())); break;       // the TGAImage as it is: no call into the shim
        default: std::fprintf(stderr, "shim_program: unknown opcode %d at operation %d\n", code, op); return 3;
        }
    }
    const std::string msg = gl_last_error_message();
    std::vector<unsigned char> b(4 + msg.size());
    const int32_t err = gl_last_error();
    std::memcpy(b.data(), &err, 4); std::memcpy(b.data() + 4, msg.data(), msg.size());
    record(T_ERROR, -1, b.data(), b.size());
    std::fclose(g_out);
    gl_shutdown();
    return 0;
}
