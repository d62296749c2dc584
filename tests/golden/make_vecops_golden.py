"""Generate tests/golden/vecops_golden.npz by running the REFERENCE's own geometry.h / tgaimage.h value ops (normalized(),
mat<4,4> * vec4, the varying interpolation v0*b0 + v1*b1 + v2*b2, TGAColor * float) through oracle/_ref/ref_harness, mode vecops,
on the seeded rows of tests/cases.py vecops_inputs().  Build container only; the committed outputs are data.

    python tests/golden/make_vecops_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
from oracle import orc  # noqa: E402
from tinyrenderder_amd import scenes  # noqa: E402


def main():
    assert orc.ref_available(), "oracle/_ref/ref_harness missing: run `make -C oracle ref REF=<reference tree>`"
    data, packed = cases.vecops_inputs()
    n = data.shape[0]
    with tempfile.TemporaryDirectory() as d:
        p_in, p_out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(p_in, "wb") as f:
            f.write(struct.pack("<ii", n, 0))
            for i in range(n):
                f.write(data[i].tobytes()); f.write(struct.pack("<II", int(packed[i]), 0))
        subprocess.run([orc.REF_HARNESS, "vecops", p_in, p_out], check=True)
        raw = np.frombuffer(open(p_out, "rb").read(), np.uint8).reshape(n, 80)
    np.savez_compressed(os.path.join(HERE, "vecops_golden.npz"),
                        inputs=np.array(scenes.digest(data) + scenes.digest(packed)),
                        d=raw[:, :72].copy().view(np.uint64),          # normalized, M*dir, interp: 9 doubles as bits
                        c=raw[:, 72:76].copy())                        # TGAColor * float
    print(n, "rows")


if __name__ == "__main__":
    main()
