// The host paths of the shadow post-pass (trgl_image::shadow_mask_bytes / modulate_bytes, the loops behind the C ABI's TRGL_MEM_HOST
// calls) on the cases of a file written by tests/shadow_cases.py, for a build under AddressSanitizer + UndefinedBehaviorSanitizer:
//     shadow_host_asan <cases file> <output file>
// Every array lives in a heap block of exactly its size, so a tap or a pixel one element outside is caught.  The output is, per case,
// the w * h mask bytes followed by the images of synthetic_image() (bpp 1, 3, 4) multiplied by that mask; tests/test_shadow.py
// compares it with the numpy model.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tinyrenderder_amd/shim/trgl_image.h"

static bool read_exact(std::FILE* f, void* dst, std::size_t n) { return n == 0 || std::fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <cases> <out>\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    char magic[8]; std::int32_t count = 0;
    if (!read_exact(in, magic, 8) || std::memcmp(magic, "TRSHDW01", 8) != 0 || !read_exact(in, &count, 4)) { std::fprintf(stderr, "bad header\n"); return 2; }
    for (std::int32_t k = 0; k < count; ++k) {
        std::int32_t dims[6]; double bd[2], M[16];
        if (!read_exact(in, dims, sizeof dims) || !read_exact(in, bd, sizeof bd) || !read_exact(in, M, sizeof M)) { std::fprintf(stderr, "case %d: short file\n", k); return 2; }
        const int w = dims[0], h = dims[1], map_w = dims[2], map_h = dims[3], radius = dims[4];
        const std::size_t n = std::size_t(w) * h, nmap = std::size_t(map_w) * map_h;
        std::vector<double> depth(n), map(nmap);
        if (!read_exact(in, depth.data(), n * sizeof(double)) || !read_exact(in, map.data(), nmap * sizeof(double))) { std::fprintf(stderr, "case %d: short file\n", k); return 2; }
        std::vector<std::uint8_t> mask(n);
        trgl_image::shadow_mask_bytes(depth.data(), w, h, M, map.data(), map_w, map_h, bd[0], bd[1], radius, mask.data());
        std::fwrite(mask.data(), 1, n, out);
        for (int bpp : { 1, 3, 4 }) {
            std::vector<std::uint8_t> img(n * bpp);
            for (std::size_t i = 0; i < img.size(); ++i) img[i] = std::uint8_t((i * 7 + i / 251) & 255);      // synthetic_image()
            trgl_image::modulate_bytes(img.data(), n, bpp, mask.data());
            std::fwrite(img.data(), 1, img.size(), out);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%d cases\n", count);
    return 0;
}
