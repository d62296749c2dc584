// demo_blend.cpp — translucent geometry over the shim: a fragment() that blends, ported as a user shader that reads the pixel it is
// drawn over (TRGL_SHADER_READS_DEST) and leaves the z-buffer alone (TRGL_SHADER_NO_DEPTH_WRITE).
// The library keeps submission order and does not sort, so the frame is drawn the way a blending renderer draws it: the opaque
// triangles first (FlatShader: they write depth), then the translucent layers back to front.  Each translucent fragment is tested
// against the opaque depth only - a pane behind a wall is hidden, two panes in front of it both show - and composited with
// trgl_blend_over, source-over with the alpha of the triangle's colour.
//   demo_blend <out.tga> [width height]
// prints the print_render_stats() line and writes the frame.  Every coordinate is a dyadic fraction, so the scene is the same
// doubles wherever it is restated (tests/test_blend_demo_gpu.py draws it through the Python binding).
#include <cstdio>
#include <cstdlib>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

static const char* kOverSource = R"(
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) };
}
)";

// a triangle at one depth, w = 1
template <class Shader>
static void draw(TGAImage& fb, const Shader& s, double x0, double y0, double x1, double y1, double x2, double y2, double z) {
    Triangle t;
    t[0] = make_vec4(x0, y0, z, 1.0);
    t[1] = make_vec4(x1, y1, z, 1.0);
    t[2] = make_vec4(x2, y2, z, 1.0);
    rasterize(t, s, fb);
}

int main(int argc, char** argv) {
    if (argc != 2 && argc != 4) { std::fprintf(stderr, "usage: demo_blend <out.tga> [width height]\n"); return 1; }
    const int W = argc == 4 ? std::atoi(argv[2]) : 320, H = argc == 4 ? std::atoi(argv[3]) : 240;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_blend: bad size\n"); return 1; }
    const int glass = gl_register_shader_flags(kOverSource, 0, TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE);
    if (glass < 0) { std::fprintf(stderr, "gl_register_shader_flags: %s\n", gl_last_error_message()); return 2; }

    TGAImage fb(W, H, TGAImage::RGB, TGAColor(24, 32, 48));
    init_zbuffer(W, H);
    init_viewport(0, 0, W, H);
    // 1. opaque: six upright wedges at depth 0, left to right
    for (int i = 0; i < 6; ++i) {
        FlatShader s;
        s.color = TGAColor(std::uint8_t(40 * i), 200, std::uint8_t(255 - 40 * i));
        const double x = -0.875 + 0.3125 * i;
        draw(fb, s, x, -0.75, x + 0.25, -0.75, x + 0.125, 0.75, 0.0);
    }
    // 2. the far translucent layer: two wide panes, one behind the wedges (depth 0.5: seen between them only) and one in front (-0.25)
    UserShader pane(glass);
    pane.color = TGAColor(255, 64, 64, 128);
    draw(fb, pane, -1.0, -0.5, 1.0, -0.5, 0.0, 0.25, 0.5);
    pane.color = TGAColor(64, 255, 64, 96);
    draw(fb, pane, -0.75, 0.5, 0.0, -0.625, 0.75, 0.5, -0.25);
    // 3. the near translucent layer, over both: depth -0.5
    pane.color = TGAColor(64, 64, 255, 160);
    draw(fb, pane, -0.5, -0.25, 0.5, -0.25, 0.0, 0.625, -0.5);
    pane.color = TGAColor(255, 255, 255, 48);
    draw(fb, pane, -0.25, -0.875, 0.875, 0.0, -0.25, 0.875, -0.5);

    if (!gl_flush(fb)) { std::fprintf(stderr, "demo_blend: %s\n", gl_last_error_message()); return 3; }
    print_render_stats();
    gl_shutdown();
    return fb.write_tga_file(argv[1]) ? 0 : 4;
}
