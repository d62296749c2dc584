"""Generate tests/golden/tga_random_golden.npz by running the REFERENCE's TGAImage::write_tga_file and read_tga_file
(oracle/_ref/ref_harness modes tga / tgaread = the reference's own tgaimage.cpp compiled in place) on seeded few-colour
images of 1, 3 and 4 bytes per pixel:
  w{bpp}_img, w{bpp}_file            an image and the file the reference writes for it (vflip, RLE: the defaults)
  r{bpp}_v{vflip}_img, _file         an image and the file the reference writes for it (RLE)
  r{bpp}_v{vflip}_cut{n}             what the reference reads from the first n bytes of that file
Build container only; the committed outputs are data.

    python tests/golden/make_tga_random_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import orc  # noqa: E402

READ_CUTS = lambda n: (n, n - 7, 60)                 # whole file, truncated mid-stream, truncated near the header


def main():
    assert orc.ref_available(), "oracle/_ref/ref_harness missing: run `make -C oracle ref REF=<reference tree>`"
    out = {}
    rng = np.random.default_rng(5)
    for bpp in (1, 3, 4):
        img = (rng.integers(0, 3, size=(37, 53, bpp)) * 120).astype(np.uint8)     # few colours: lots of runs
        out[f"w{bpp}_img"] = img
        out[f"w{bpp}_file"] = np.frombuffer(orc.run_reference_tga(img), np.uint8)
    rng = np.random.default_rng(9)
    for bpp in (1, 3, 4):
        img = (rng.integers(0, 3, size=(23, 31, bpp)) * 120).astype(np.uint8)
        for vflip in (0, 1):
            f = orc.run_reference_tga(img, bool(vflip), True)
            key = f"r{bpp}_v{vflip}"
            out[key + "_img"], out[key + "_file"] = img, np.frombuffer(f, np.uint8)
            for cut in READ_CUTS(len(f)):
                got = orc.run_reference_tga_read(f[:cut])
                assert got is not None, (key, cut)          # truncated data is not an error in the reference
                out[f"{key}_cut{cut}"] = got
    np.savez_compressed(os.path.join(HERE, "tga_random_golden.npz"), **out)
    print(len(out), "arrays")


if __name__ == "__main__":
    main()
