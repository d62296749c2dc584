// demo_occlusion.cpp — occlusion culling of model boxes over the shim, the test a scene makes where main.cpp:647,680,706 ask
// frustum.intersects: the large model (a wall) is drawn first, the boxes of the other models are asked against the depths it left in
// HBM, and only the models whose code has bit 0 set are drawn.
//   demo_occlusion [width height] [all]
// prints one line per model - name, TRGL_OCCL_* code, drawn or not - and the FNV-1a digest of the frame.  With `all` every model is
// drawn whatever its code says: the digest must be the same, since a model that was skipped had no fragment to give.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../tinyrenderder_amd/shim/trgl_shaders.h"

namespace {

// stands in for the reference's Model: one quad facing the camera, and the box Model::load would leave in localAABB (model.cpp:15-40:
// the extent with a margin; a flat quad gets a slab in z)
struct QuadModel {
    const char* name; vec3 p[4]; TGAColor color;
    AABB worldAABB() const {
        AABB b;
        for (int a = 0; a < 3; ++a) {
            double lo = p[0][a], hi = p[0][a];
            for (int v = 1; v < 4; ++v) { lo = std::min(lo, p[v][a]); hi = std::max(hi, p[v][a]); }
            const double margin = a == 2 ? 0.1 : (hi - lo) * 0.01;
            b.min[a] = lo - margin; b.max[a] = hi + margin;
        }
        return b;
    }
};

QuadModel quad(const char* name, double x0, double x1, double y0, double y1, double z, TGAColor color) {
    // counter-clockwise seen from +z, where the camera is
    return { name, { make_vec3(x0, y0, z), make_vec3(x1, y0, z), make_vec3(x1, y1, z), make_vec3(x0, y1, z) }, color };
}

void draw_model(const QuadModel& m, TGAImage& fb) {                        // the face loop of main.cpp:660-666 for two faces
    static const int corner[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
    FlatShader shader;
    shader.color = m.color;
    for (const auto& tri : corner) {
        Triangle clip;
        for (int v = 0; v < 3; ++v) clip[v] = Perspective * (ModelView * make_vec4(m.p[tri[v]][0], m.p[tri[v]][1], m.p[tri[v]][2], 1.0));
        rasterize(clip, shader, fb);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool all = argc > 1 && std::strcmp(argv[argc - 1], "all") == 0;
    const int nsize = argc - 1 - (all ? 1 : 0);
    if (nsize != 0 && nsize != 2) { std::fprintf(stderr, "usage: demo_occlusion [width height] [all]\n"); return 1; }
    const int W = nsize ? std::atoi(argv[1]) : 640, H = nsize ? std::atoi(argv[2]) : 480;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "demo_occlusion: bad size\n"); return 1; }

    const QuadModel wall = quad("wall", -2.0, 2.0, -1.5, 1.5, 0.0, TGAColor(200, 190, 170));
    const std::vector<QuadModel> models = {
        quad("behind_centre", -0.5, 0.5, -0.5, 0.5, -2.0, TGAColor(220, 60, 60)),      // hidden by the wall
        quad("behind_edge", 1.0, 1.3, 0.9, 1.2, -1.0, TGAColor(60, 220, 60)),         // hidden too, close to the wall's corner
        quad("in_front", -1.2, -0.6, -0.4, 0.2, 2.0, TGAColor(60, 110, 220)),         // nearer than the wall
        quad("sticks_out", 1.5, 4.0, -0.3, 0.3, -2.0, TGAColor(220, 220, 60)),        // behind the wall, but wider than it
        quad("far_right", 30.0, 31.0, 0.0, 1.0, -2.0, TGAColor(220, 60, 220)),        // off the screen: its rectangle is empty
        quad("behind_camera", -0.5, 0.5, -0.5, 0.5, 8.0, TGAColor(60, 220, 220)),     // w <= 0: the box bounds nothing, rasterize() rejects the faces
    };

    TGAImage framebuffer(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    lookat(make_vec3(0.0, 0.0, 5.0), make_vec3(0.0, 0.0, 0.0), make_vec3(0.0, 1.0, 0.0));
    init_perspective(60.0, double(W) / H, 1.0, 20.0);
    init_viewport(0, 0, W, H);
    const mat<4, 4> viewProjection = Perspective * ModelView;                  // main.cpp:623

    draw_model(wall, framebuffer);                                             // the large model first: its depths are what hides the others

    std::vector<AABB> boxes;
    for (const QuadModel& m : models) boxes.push_back(m.worldAABB());
    const std::vector<std::uint8_t> codes = gl_occlusion_test(boxes, viewProjection);     // one call for all boxes, against the z-buffer in HBM
    if (gl_last_error() != TRGL_OK) { std::fprintf(stderr, "demo_occlusion: %s (code %d)\n", gl_last_error_message(), gl_last_error()); return 2; }

    int drawn = 0;
    for (size_t i = 0; i < models.size(); ++i) {
        const bool draw = all || gl_occlusion_draw(codes[i]);                  // (a scene asks frustum.intersects(boxes[i]) && ... here, main.cpp:647)
        if (draw) { draw_model(models[i], framebuffer); ++drawn; }
        std::printf("%-14s code=%d %s\n", models[i].name, int(codes[i]), draw ? "drawn" : "skipped");
    }
    if (!gl_flush(framebuffer)) { std::fprintf(stderr, "demo_occlusion: %s (code %d)\n", gl_last_error_message(), gl_last_error()); return 2; }

    std::uint64_t digest = 1469598103934665603ull;                             // FNV-1a over the frame's bytes
    const std::uint8_t* px = framebuffer.buffer();
    for (size_t i = 0; i < size_t(W) * H * 3; ++i) { digest ^= px[i]; digest *= 1099511628211ull; }
    std::printf("models drawn: %d of %zu\nframe digest: %016llx\n", drawn, models.size(), (unsigned long long)digest);
    gl_shutdown();
    return 0;
}
