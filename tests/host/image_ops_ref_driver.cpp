// image_ops_ref_driver.cpp — TEST INFRASTRUCTURE.  Calls the reference's own compiled TGAImage::gaussian_blur and TGAImage::scale
// (linked from oracle/_ref/tgaimage.o) for tests/golden/make_image_ops_golden.py.  Nothing of the reference is copied here; the binary
// is built into a temporary directory and never kept.
//   image_ops_ref_driver <cases.txt> <results.txt>
// Bytes travel as hex digits ("-" for none).  One case per line:
//   blur    w h bpp radius bytes        -> w h bytes                 (w * h == 0: a default-constructed, empty TGAImage)
//   scale   w h bpp w2 h2 bytes         -> ok w h bytes              (ok: what scale() returned)
#include "tgaimage.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static std::vector<std::uint8_t> unhex(const std::string& t) {
    std::vector<std::uint8_t> out;
    if (t == "-") return out;
    for (size_t k = 0; k + 1 < t.size(); k += 2) out.push_back((std::uint8_t)std::stoi(t.substr(k, 2), nullptr, 16));
    return out;
}
static void put(std::ostream& out, TGAImage& img, int bpp) {
    const size_t n = (size_t)img.width() * img.height() * bpp;
    out << img.width() << " " << img.height() << " ";
    if (!n) { out << "-"; return; }
    const std::uint8_t* p = img.buffer();
    char b[4];
    for (size_t k = 0; k < n; ++k) { std::snprintf(b, sizeof b, "%02x", p[k]); out << b; }
}
static bool fill(TGAImage& img, int w, int h, int bpp, const std::vector<std::uint8_t>& bytes) {
    if (w * h == 0) return bytes.empty();
    img = TGAImage(w, h, bpp);
    if (bytes.size() != (size_t)w * h * bpp) return false;
    std::memcpy(img.buffer(), bytes.data(), bytes.size());
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string what; ls >> what;
        if (what.empty()) continue;
        if (what != "blur" && what != "scale") { std::fprintf(stderr, "image_ops_ref_driver: unknown case '%s'\n", what.c_str()); return 2; }
        int w, h, bpp, radius = 0, w2 = 0, h2 = 0; std::string hex;
        ls >> w >> h >> bpp;
        if (what == "blur") ls >> radius; else ls >> w2 >> h2;
        ls >> hex;
        TGAImage img;
        if (!ls || !fill(img, w, h, bpp, unhex(hex))) { std::fprintf(stderr, "image_ops_ref_driver: bad case\n"); return 2; }
        if (what == "blur") img.gaussian_blur(radius);
        else out << (img.scale(w2, h2) ? 1 : 0) << " ";
        put(out, img, bpp);
        out << "\n";
    }
    return out ? 0 : 3;
}
