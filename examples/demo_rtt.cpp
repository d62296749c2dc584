// demo_rtt.cpp — supersampling and render-to-texture over the shim (new work; include/trgl.h, "box-filter resolve and frames as textures").
// A small scene is drawn at twice the wanted size, plus one spare column and row that the filter ignores.  Then
//   * gl_resolve(frame, 2, &small) box-filters it in HBM into the anti-aliased small image (SSAA 2 x 2): only that image crosses PCIe;
//   * gl_texture_from_framebuffer(frame, SLOT, 2) makes the same filtered frame a texture without leaving HBM;
//   * a second frame shows a quad that samples the slot - a screen in the scene - through a user shader calling trgl_sample2D.
//   demo_rtt device <big.tga> <ssaa.tga> <screen.tga>
//   demo_rtt host   <big.tga> <ssaa.tga> <screen.tga>     the route this replaces: gl_flush, gl_downsample on the host, gl_upload_texture
// Both modes write the same three files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

static const int SLOT = 3;

// the texel of slot 3 at the interpolated uv (varyings: u, v of the three vertices), opaque
static const char* kScreenSource = R"(
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (v[0] * in.bar[0] + v[2] * in.bar[1]) + v[4] * in.bar[2], (v[1] * in.bar[0] + v[3] * in.bar[1]) + v[5] * in.bar[2] };
    return trgl_sample2D(in, 3, uv).bgra | 0xff000000u;
}
)";

// thin slanted triangles: edges that show their stair-steps at one sample a pixel
static void draw_scene(TGAImage& fb) {
    init_viewport(0, 0, fb.width(), fb.height());
    const int n = 18;
    for (int i = 0; i < n; ++i) {
        const double a0 = 2 * M_PI * i / n, a1 = 2 * M_PI * (i + 0.45) / n;
        Triangle clip;
        clip[0] = make_vec4(0.05 * std::cos(a0), 0.05 * std::sin(a0), 0.1, 1.0);
        clip[1] = make_vec4(0.95 * std::cos(a0), 0.95 * std::sin(a0), 0.2, 1.0);
        clip[2] = make_vec4(0.95 * std::cos(a1), 0.95 * std::sin(a1), -0.3, 1.0);
        FlatShader s;
        s.color = TGAColor(uint8_t(40 + 11 * i), uint8_t(250 - 12 * i), uint8_t(90 + 7 * (i % 5)), 255);
        rasterize(clip, s, fb);
    }
}

static void draw_screen(TGAImage& fb, int kind) {
    init_viewport(0, 0, fb.width(), fb.height());
    const double x0 = -0.7, x1 = 0.8, y0 = -0.6, y1 = 0.75;
    const double corner[4][4] = { { x0, y0, 0, 0 }, { x1, y0, 1, 0 }, { x1, y1, 1, 1 }, { x0, y1, 0, 1 } };      // x, y, u, v
    const int tri[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
    for (int t = 0; t < 2; ++t) {
        Triangle clip;
        UserShader s(kind);
        for (int k = 0; k < 3; ++k) {
            const double* c = corner[tri[t][k]];
            clip[k] = make_vec4(c[0], c[1], 0.0, 1.0);
            s.varyings.push_back(c[2]);
            s.varyings.push_back(c[3]);
        }
        rasterize(clip, s, fb);
    }
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: demo_rtt device|host <big.tga> <ssaa.tga> <screen.tga>\n"); return 1; }
    const bool host = std::strcmp(argv[1], "host") == 0;
    const int W = 81, H = 59;
    const int kind = gl_register_shader(kScreenSource, 6);
    if (kind < 0) { std::fprintf(stderr, "gl_register_shader: %s\n", gl_last_error_message()); return 2; }

    TGAImage big(2 * W + 1, 2 * H + 1, TGAImage::RGB);
    init_zbuffer(big.width(), big.height());
    draw_scene(big);
    TGAImage ssaa;
    bool ok;
    if (host) {
        ok = gl_flush(big) && gl_downsample(big, 2, &ssaa) && gl_upload_texture(big, SLOT, ssaa);
    } else {
        ok = gl_resolve(big, 2, &ssaa) && gl_texture_from_framebuffer(big, SLOT, 2) && gl_flush(big);
    }
    if (!ok) { std::fprintf(stderr, "demo_rtt: first frame: %s\n", gl_last_error_message()); return 3; }

    // the second frame, of the same size: it takes the context over, and the slot with it
    TGAImage screen(big.width(), big.height(), TGAImage::RGB);
    for (int y = 0; y < screen.height(); ++y)
        for (int x = 0; x < screen.width(); ++x) screen.set(x, y, TGAColor(uint8_t(30 + y / 2), 20, uint8_t(60 + x / 3), 255));
    gl_framebuffer_modified(screen);
    init_zbuffer(screen.width(), screen.height());
    draw_screen(screen, kind);
    if (!gl_flush(screen)) { std::fprintf(stderr, "demo_rtt: second frame: %s\n", gl_last_error_message()); return 3; }
    gl_shutdown();
    return big.write_tga_file(argv[2]) && ssaa.write_tga_file(argv[3]) && screen.write_tga_file(argv[4]) ? 0 : 4;
}
