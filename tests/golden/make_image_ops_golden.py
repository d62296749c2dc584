"""Generate tests/golden/image_ops_golden.npz: the reference's own compiled TGAImage::gaussian_blur and TGAImage::scale (tgaimage.cpp:246-324)
on the small images built below.  tests/host/image_ops_ref_driver.cpp is compiled against the reference's tgaimage.h where it lies and
linked with oracle/_ref/tgaimage.o (left there by `make -C oracle ref`), into a temporary directory; only inputs and results are kept.
Build container only; needs the built library (for trgl_gaussian_kernel).

    python tests/golden/make_image_ops_golden.py [reference tree, default /root/reference]

Contents (np.load, no pickle):
    meta                  JSON: {"images": [names], "radii": [...], "switch_radius": r, "scale": [[image, w2, h2, ok], ...]}
    img/<name>            [h, w, bpp] uint8 inputs ("empty" is [0, 0, 3])
    weights/<radius>      the 2 * radius + 1 weights as uint32 bit patterns
    blur/<name>/<radius>  gaussian_blur(radius) of the image
    scale/<k>             the image after scale case k (unchanged where ok = 0)
The reference keeps its weight vector to itself, so the weights stored are trgl_gaussian_kernel's, computed here - and pinned to the
reference by its results: the numpy model (tests/image_ops_model.py), fed these weights, must reproduce every blurred byte of the
reference's compiled code at every radius, which the maker asserts.  Two more assertions: the all-255 image never produces a wrapped
byte (no sum truncates past 255), and a blur at radius 0 / -1 leaves the reference's image alone.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import image_ops_model  # noqa: E402
from tinyrenderder_amd import api  # noqa: E402


def switch_radius():
    text = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()
    return int(re.search(r"constexpr int BLUR_LDS_RADIUS = (\d+);", text).group(1))


def images(rng):
    out = {}
    for bpp in (1, 3, 4):
        out["random_bpp%d" % bpp] = rng.integers(0, 256, (41, 67, bpp), dtype=np.uint8)
    out["all_255"] = np.full((41, 67, 4), 255, np.uint8)
    out["all_0"] = np.zeros((41, 67, 3), np.uint8)
    yy, xx = np.mgrid[0:41, 0:67]
    out["checker"] = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    out["one_pixel"] = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)
    out["one_column"] = rng.integers(0, 256, (23, 1, 3), dtype=np.uint8)         # 1 x 23
    out["one_row"] = rng.integers(0, 256, (1, 23, 4), dtype=np.uint8)            # 23 x 1
    return out


SCALE_CASES = [("random_bpp3", 134, 82), ("random_bpp3", 100, 60), ("random_bpp3", 40, 30), ("random_bpp3", 33, 7), ("random_bpp3", 1, 1),
               ("random_bpp3", 67, 1), ("random_bpp3", 1, 41), ("random_bpp3", 67, 41), ("random_bpp3", 300, 2),
               ("random_bpp1", 101, 67), ("random_bpp1", 13, 50), ("random_bpp4", 90, 31), ("random_bpp4", 20, 80),
               ("one_pixel", 5, 4), ("one_column", 3, 9), ("one_row", 50, 3),
               ("random_bpp3", 0, 10), ("random_bpp3", 10, -1), ("random_bpp1", -3, -3), ("empty", 4, 4)]


def hexbytes(a):
    return a.tobytes().hex() if a.size else "-"


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    obj = os.path.join(ROOT, "oracle", "_ref", "tgaimage.o")
    assert os.path.exists(obj), "oracle/_ref/tgaimage.o missing: run `make -C oracle ref REF=<reference tree>`"
    rng = np.random.default_rng(20262)
    imgs = images(rng)
    imgs["empty"] = np.zeros((0, 0, 3), np.uint8)
    sw = switch_radius()
    radii = sorted({1, 2, 3, 5, 9, 40, 70, sw, sw + 1})
    blur_names = [n for n in imgs if n != "empty"]
    lines, kinds = [], []
    for name in blur_names:
        a = imgs[name]
        for r in radii + [0, -1]:
            lines.append("blur %d %d %d %d %s" % (a.shape[1], a.shape[0], a.shape[2], r, hexbytes(a)))
            kinds.append(("blur", name, r))
    lines.append("blur 0 0 3 2 -"); kinds.append(("blur", "empty", 2))
    for k, (name, w2, h2) in enumerate(SCALE_CASES):
        a = imgs[name]
        lines.append("scale %d %d %d %d %d %s" % (a.shape[1], a.shape[0], a.shape[2], w2, h2, hexbytes(a)))
        kinds.append(("scale", k, None))
    with tempfile.TemporaryDirectory() as d:
        driver = os.path.join(d, "image_ops_ref_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I" + ref,
                        os.path.join(ROOT, "tests", "host", "image_ops_ref_driver.cpp"), obj, "-o", driver, "-lm"], check=True)
        p_in, p_out = os.path.join(d, "cases.txt"), os.path.join(d, "results.txt")
        with open(p_in, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run([driver, p_in, p_out], check=True)
        res = open(p_out).read().splitlines()
    assert len(res) == len(lines)

    def image_of(tok, bpp):
        w, h = int(tok[0]), int(tok[1])
        return np.frombuffer(bytes.fromhex("" if tok[2] == "-" else tok[2]), np.uint8).reshape(h, w, bpp).copy()

    weights = {r: api.gaussian_kernel(r) for r in radii}
    store = {"img/" + n: a for n, a in imgs.items()}
    for r in radii:
        store["weights/%d" % r] = weights[r].view(np.uint32)
    scale_meta = []
    for (kind, key, r), line in zip(kinds, res):
        tok = line.split()
        if kind == "blur":
            a = imgs[key]
            got = image_of(tok, a.shape[2])
            if r <= 0 or key == "empty":
                assert np.array_equal(got, a), (key, r, "the reference touched the image")
                continue
            assert np.array_equal(image_ops_model.gaussian_blur(a, weights[r]), got), (key, r, "model (trgl_gaussian_kernel's weights) != reference")
            if key == "all_255":
                # the weights sum to 1 within a few ulps: a pass turns 255 into 254 or 255 and 254 into 253 or 254 - unless a sum reaches
                # 256 and (uint8_t) wraps it to 0
                assert got.min() >= 253, (r, int(got.min()), "a sum truncated past 255 and wrapped")
            store["blur/%s/%d" % (key, r)] = got
        else:
            name, w2, h2 = SCALE_CASES[key]
            a = imgs[name]
            ok, got = int(tok[0]), image_of(tok[1:], a.shape[2])
            want = image_ops_model.scale(a, w2, h2)
            assert (want is not None) == bool(ok), (name, w2, h2)
            assert np.array_equal(got, want if ok else a), (name, w2, h2, "model != reference")
            store["scale/%d" % key] = got
            scale_meta.append([name, w2, h2, ok])
            print("scale %-12s -> %4d x %-4d ok=%d" % (name, w2, h2, ok))
    assert any(not c[3] for c in scale_meta) and any(c[3] for c in scale_meta)
    store["meta"] = np.array(json.dumps(dict(images=blur_names, radii=radii, switch_radius=sw, scale=scale_meta)))
    path = os.path.join(HERE, "image_ops_golden.npz")
    np.savez_compressed(path, **store)
    print(len(blur_names), "images x", radii, "+", len(scale_meta), "scale cases,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
