// demo_image_ops.cpp — TGAImage::gaussian_blur / TGAImage::scale as a caller of the reference's image class uses them, over the shim.
//   demo_image_ops host   <in.bin> <out.bin>     the TGAImage members of shim/trgl_image.h: host loops, no GPU is touched
//   demo_image_ops device <in.bin> <out.bin>     the blur through gl_gaussian_blur(): the image is the framebuffer, blurred in HBM
// in.bin : "TRGIMG01", int32 w, h, bpp, radius, w2, h2, then w * h * bpp bytes
// out.bin: the blurred bytes (w * h * bpp); host mode then appends int32 ok, w, h of `image.scale(w2, h2)` and the bytes it left
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../tinyrenderder_amd/shim/trgl_gl.h"

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: demo_image_ops host|device in.bin out.bin\n"); return 1; }
    const std::string mode = argv[1];
    std::ifstream in(argv[2], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    int hd[6];
    if (raw.size() < 8 + sizeof hd || std::memcmp(raw.data(), "TRGIMG01", 8) != 0) { std::fprintf(stderr, "demo_image_ops: bad input\n"); return 1; }
    std::memcpy(hd, raw.data() + 8, sizeof hd);
    const int w = hd[0], h = hd[1], bpp = hd[2], radius = hd[3], w2 = hd[4], h2 = hd[5];
    const size_t n = size_t(w) * h * bpp;
    if (raw.size() != 8 + sizeof hd + n) { std::fprintf(stderr, "demo_image_ops: short input\n"); return 1; }
    TGAImage image(w, h, bpp);
    if (n) std::memcpy(image.buffer(), raw.data() + 8 + sizeof hd, n);
    std::ofstream out(argv[3], std::ios::binary);

    TGAImage blurred = image;
    if (mode == "device") {
        if (!gl_gaussian_blur(blurred, radius) || !gl_flush(blurred)) { std::fprintf(stderr, "demo_image_ops: %s\n", gl_last_error_message()); return 2; }
        out.write(reinterpret_cast<const char*>(blurred.buffer()), std::streamsize(n));
        gl_shutdown();
        return out ? 0 : 3;
    }
    blurred.gaussian_blur(radius);
    if (n) out.write(reinterpret_cast<const char*>(blurred.buffer()), std::streamsize(n));
    TGAImage scaled = image;
    const int res[3] = { scaled.scale(w2, h2) ? 1 : 0, scaled.width(), scaled.height() };
    out.write(reinterpret_cast<const char*>(res), sizeof res);
    const size_t n2 = size_t(res[1]) * res[2] * bpp;
    if (n2) out.write(reinterpret_cast<const char*>(scaled.buffer()), std::streamsize(n2));
    return out ? 0 : 3;
}
