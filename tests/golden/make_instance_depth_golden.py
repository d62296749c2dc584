"""Generate tests/golden/instance_depth_golden.npz: element 2 of (A * B) * (p, 1) computed by the REFERENCE's own geometry.h (operator* of
two mat<4,4>, geometry.h:196-205, then operator* of a matrix and a vec<4>, :187-192, which is dot<4>, :123-127) in a stand-alone program
compiled here with -ffp-contract=off - the expression trgl_instance_depths is defined by.  The fixture holds ordinary values, signed
zeros, infinities, denormals and values near 1e308.  Build container only (it needs the reference tree); the committed inputs and
outputs are data.

    python tests/golden/make_instance_depth_golden.py [reference tree]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tinyrenderder_amd import scenes  # noqa: E402

DRIVER = r"""
#include <cstdio>
#include "geometry.h"
int main(int argc, char** argv) {
    FILE* in = std::fopen(argv[1], "rb"); FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    double abp[35];
    while (std::fread(abp, sizeof(double), 35, in) == 35) {
        mat<4, 4> A, B;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { A[i][j] = abp[4 * i + j]; B[i][j] = abp[16 + 4 * i + j]; }
        vec<4> v;
        v[0] = abp[32]; v[1] = abp[33]; v[2] = abp[34]; v[3] = 1.0;
        const vec<4> e = (A * B) * v;
        const double d = e[2];
        std::fwrite(&d, sizeof(double), 1, out);
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
"""

N_ORDINARY = 8          # the first cases hold ordinary values only (a contracted multiply-add shows there)


def fixture(n=96, seed=0x0DE97):
    """[n, 35] float64: A (16), B (16) and the point (3), with special values sprinkled in."""
    rng = scenes.SplitMix64(seed)
    m = rng.uniform(n * 35, -4.0, 4.0).reshape(n, 35)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 1e308, -1e308, 1.0, -1.0])
    pick = rng.u64(n * 35).reshape(n, 35)
    where = (pick % np.uint64(4)) == 0                      # a quarter of the entries
    where[:N_ORDINARY] = False
    m[where] = special[((pick >> np.uint64(8)) % np.uint64(len(special))).astype(np.int64)][where]
    m[8, 8:12] = np.array([-0.0, 0.0, -0.0, 0.0])           # row 2 of A: every product of the first stage is a zero
    m[9, 32:35] = 0.0                                       # the point at the origin: the depth is the translation's
    m[10, :] = 5e-324                                       # denormal products underflow
    m[11, 8:12] = 1e308; m[11, 16:32] = 1.0; m[11, 32:35] = 1.0      # sums that overflow on the way
    m[12, :32] = np.concatenate([np.eye(4).reshape(16), np.eye(4).reshape(16)]); m[12, 32:35] = [0.25, -0.5, -3.0]     # identity: d = p.z
    return np.ascontiguousarray(m)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    assert os.path.exists(os.path.join(ref, "geometry.h")), "the reference tree is needed"
    abp = fixture()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        p_in, p_out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        open(src, "w").write(DRIVER)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", ref, "-o", exe, src], check=True)
        abp.tofile(p_in)
        subprocess.run([exe, p_in, p_out], check=True)
        z = np.fromfile(p_out, np.float64)
    assert z.shape[0] == abp.shape[0]
    np.savez_compressed(os.path.join(HERE, "instance_depth_golden.npz"), abp=abp.view(np.uint64), z=z.view(np.uint64))
    print(z.shape[0], "depths;", int(np.isnan(z).sum()), "NaN,", int(np.isinf(z).sum()), "inf,", int((z == 0).sum()), "zeros")


if __name__ == "__main__":
    main()
