"""Generate tests/golden/scene_golden.json: the reference's own compiled Frustum::createFromMatrix / intersects (our_gl.cpp:212-280),
AABB::transform (geometry.h:297-327), Camera (camera.h, with main.cpp:585-594's settings) and Model::computeAABB (model.cpp:15-40) on
the cases built below.  tests/host/scene_ref_driver.cpp is compiled against the reference's headers where they lie and linked with
the objects `make -C oracle ref` left in oracle/_ref/, into a temporary directory; only inputs and results (doubles as C hex floats)
are kept.  Build container only.

    python tests/golden/make_scene_golden.py [reference tree, default /root/reference]
"""
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")


def hx(a):
    return [float(x).hex() for x in np.asarray(a, np.float64).reshape(-1)]


def line(what, *arrays):
    return what + " " + " ".join(" ".join(hx(a)) for a in arrays)


def unhex(text):
    return [float.fromhex(t) for t in text.split()]


def run(driver, lines):
    with tempfile.TemporaryDirectory() as d:
        p_in, p_out = os.path.join(d, "cases.txt"), os.path.join(d, "results.txt")
        with open(p_in, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run([driver, p_in, p_out], check=True)
        out = open(p_out).read().splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def frustum_matrices(rng, viewproj):
    ms = [viewproj, np.eye(4)]
    for k in range(32):                                        # seeded random matrices, a few scales
        ms.append(rng.standard_normal((4, 4)) * 10.0 ** rng.integers(-3, 4))
    ms.append(np.zeros((4, 4)))                                # every normal has length 0: the `length > 0.0` guard keeps d as it is
    z = rng.standard_normal((4, 4)); z[:3, :] = 0.0            # rows 0..2 zero, row 3 not: normal 0, d != 0
    ms.append(z)
    z = rng.standard_normal((4, 4)); z[1, :] = 0.0             # one zero row
    ms.append(z)
    z = np.eye(4); z[0, 0] = -0.0; z[2, 3] = -0.0              # signed zeros in the sums
    ms.append(z)
    return ms


def boxes_for(planes, rng):
    """Boxes inside, outside and straddling each plane of the cube frustum |x|,|y|,|z| <= 1 (planes of the identity matrix), with
    the positive corner exactly on a plane and one ulp beyond it; degenerate and inverted boxes; NaN and infinite ones."""
    out = [([-0.5] * 3, [0.5] * 3), ([-3.0] * 3, [3.0] * 3), ([0.0] * 3, [0.0] * 3), ([0.5] * 3, [-0.5] * 3)]
    for axis in range(3):
        for sign in (1.0, -1.0):
            lo, hi = [-0.25] * 3, [0.25] * 3
            a, b = sorted((sign * 2.0, sign * 3.0))
            o_lo, o_hi = list(lo), list(hi); o_lo[axis], o_hi[axis] = a, b                       # outside
            out.append((o_lo, o_hi))
            a, b = sorted((sign * 0.5, sign * 1.5))
            s_lo, s_hi = list(lo), list(hi); s_lo[axis], s_hi[axis] = a, b                       # straddling
            out.append((s_lo, s_hi))
            # the corner the test picks lies exactly on the plane: distance == 0 intersects; one ulp further out does not
            e_lo, e_hi = list(lo), list(hi)
            if sign > 0:
                e_lo[axis], e_hi[axis] = 1.0, 2.0
                out.append((e_lo, e_hi)); f = list(e_lo); f[axis] = math.nextafter(1.0, 2.0); out.append((f, list(e_hi)))
            else:
                e_lo[axis], e_hi[axis] = -2.0, -1.0
                out.append((e_lo, e_hi)); f = list(e_hi); f[axis] = math.nextafter(-1.0, -2.0); out.append((list(e_lo), f))
    out.append(([math.nan, 0, 0], [1, 1, 1])); out.append(([0, 0, 0], [math.nan, math.nan, math.nan]))
    out.append(([-math.inf] * 3, [math.inf] * 3)); out.append(([math.inf] * 3, [math.inf] * 3))
    for _ in range(12):
        c, h = rng.uniform(-2, 2, 3), rng.uniform(0, 1.5, 3)
        out.append((c - h, c + h))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    objs = [os.path.join(REF_OBJ, o) for o in ("our_gl.o", "tgaimage.o", "model.o", "model_manager.o")]
    assert all(os.path.exists(o) for o in objs), "oracle/_ref objects missing: run `make -C oracle ref REF=<reference tree>`"
    rng = np.random.default_rng(20260)
    with tempfile.TemporaryDirectory() as d:
        driver = os.path.join(d, "scene_ref_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I" + ref,
                        "-I" + os.path.join(ROOT, "oracle", "assimp_standin"), os.path.join(ROOT, "tests", "host", "scene_ref_driver.cpp")]
                       + objs + ["-o", driver, "-lm"], check=True)

        cam = unhex(run(driver, ["camera"])[0])
        names = ("view", "projection", "view_projection", "sponza_model", "head_model")
        camera = {n: cam[16 * i:16 * i + 16] for i, n in enumerate(names)}
        viewproj = np.array(camera["view_projection"]).reshape(4, 4)
        model_ms = [np.array(camera["sponza_model"]).reshape(4, 4), np.array(camera["head_model"]).reshape(4, 4)]

        ms = frustum_matrices(rng, viewproj)
        res = run(driver, [line("frustum", m) for m in ms])
        frustum = [dict(m=hx(m), planes=hx(unhex(r))) for m, r in zip(ms, res)]

        icases = []
        cube = np.array(unhex(res[1])).reshape(6, 4)                                    # planes of the identity matrix
        for lo, hi in boxes_for(cube, rng):
            icases.append((cube, lo, hi))
        vp_planes = np.array(unhex(res[0])).reshape(6, 4)                               # main.cpp's camera
        for _ in range(40):
            c, h = rng.uniform(-8, 8, 3), rng.uniform(0, 3, 3)
            icases.append((vp_planes, c - h, c + h))
        for k in (2, 5, 9, 34, 35, 36, 37):                                             # random and degenerate frustums
            pl = np.array(unhex(res[k])).reshape(6, 4)
            for _ in range(6):
                c, h = rng.uniform(-3, 3, 3), rng.uniform(0, 2, 3)
                icases.append((pl, c - h, c + h))
        ires = run(driver, [line("intersect", *c) for c in icases])
        intersect = [dict(planes=hx(c[0]), min=hx(c[1]), max=hx(c[2]), result=int(r)) for c, r in zip(icases, ires)]
        assert {x["result"] for x in intersect} == {0, 1}

        tcases = []
        for m in model_ms + [np.eye(4), viewproj]:
            for lo, hi in (([-1.0, -2.0, -3.0], [1.5, 2.5, 3.5]), ([0.0] * 3, [0.0] * 3), ([2.0] * 3, [-2.0] * 3), ([-50.0, 0.0, -70.0], [60.0, 40.0, 30.0])):
                tcases.append((m, lo, hi))
        for _ in range(24):                                                             # general matrices: some corners get w <= 0
            m = rng.standard_normal((4, 4))
            c, h = rng.uniform(-2, 2, 3), rng.uniform(0, 2, 3)
            tcases.append((m, c - h, c + h))
        w0 = np.eye(4); w0[3] = [1.0, 0.0, 0.0, 0.0]                                    # w = x: exactly 0 on the box's min.x face
        tcases.append((w0, [0.0, -1.0, -1.0], [1.0, 1.0, 1.0]))
        tcases.append((w0, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]))                        # w < 0 on one side
        tcases.append((np.zeros((4, 4)), [-1.0] * 3, [1.0] * 3))                        # 0 / 0 everywhere: the sentinels stay
        tcases.append((np.eye(4) * 1e12, [-1.0] * 3, [1.0] * 3))
        tres = [unhex(r) for r in run(driver, [line("transform", *c) for c in tcases])]
        transform = [dict(m=hx(c[0]), min=hx(c[1]), max=hx(c[2]), out_min=hx(r[:3]), out_max=hx(r[3:])) for c, r in zip(tcases, tres)]

        meshes = [np.zeros((0, 3)), rng.standard_normal((1, 3)), rng.standard_normal((2, 14)), rng.standard_normal((1000, 3)) * 3.0]
        m = rng.standard_normal((40, 8)); m[3, 0] = math.nan; m[7, 1] = math.inf; m[9, 2] = -math.inf; m[11, :3] = math.nan
        meshes.append(m)
        meshes.append(np.full((5, 3), 2e9)); meshes.append(np.full((5, 3), -2e9))       # beyond the start values: they stay
        flat = rng.standard_normal((6, 3)); flat[:, 1] = [0.0, -0.0, 0.0, -0.0, 0.0, 0.0]
        meshes.append(flat.copy())
        flat[:, 1] = [-0.0, 0.0, 0.0, -0.0, 0.0, 0.0]
        meshes.append(flat.copy())
        bres = [unhex(r) for r in run(driver, ["bounds %d %d %s" % (v.shape[0], v.shape[1], " ".join(hx(v))) for v in meshes])]
        bounds = [dict(n=int(v.shape[0]), stride=int(v.shape[1]), v=hx(v), out_min=hx(r[:3]), out_max=hx(r[3:])) for v, r in zip(meshes, bres)]

    with open(os.path.join(HERE, "scene_golden.json"), "w") as f:
        json.dump(dict(camera={k: hx(v) for k, v in camera.items()}, frustum=frustum, intersect=intersect, transform=transform, bounds=bounds),
                  f, separators=(",", ":"))
    print(len(frustum), "frustums,", len(intersect), "intersections,", len(transform), "transforms,", len(bounds), "meshes")


if __name__ == "__main__":
    main()
