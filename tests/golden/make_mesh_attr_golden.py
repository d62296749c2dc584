"""Generate tests/golden/mesh_attr_golden.json: the reference's own compiled Model::generateNormalsIfNeeded (model.cpp:269-316) and
Model::computeTangentsIfNeeded (model.cpp:318-388) on the small meshes built below.  tests/host/mesh_attr_ref_driver.cpp is compiled
against the reference's headers where they lie and linked with oracle/_ref/model.o (left there by `make -C oracle ref`), into a temporary
directory; only inputs and results (doubles as C hex floats) are kept.  Build container only.

    python tests/golden/make_mesh_attr_golden.py [reference tree, default /root/reference]

A case is {name, kind, stride, v [nv * stride], i [nf * 3] or {fan: arguments of mesh_attr_model.fan_indices}, generated, out}: `out` holds
the columns the function may write (normal; tangent and bitangent), and the maker asserts that the reference left every other one alone.
The reference's record has 14 doubles; a case of another stride hands it the first min(stride, 14) columns (zeros behind them); columns
past 14 are the caller's own and must come back untouched.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_attr_model  # noqa: E402


def hx(a):
    return [float(x).hex() for x in np.asarray(a, np.float64).reshape(-1)]


def fan(rng, nfaces, rim=40):
    """`nfaces` faces around vertex 0 over `rim` rim vertices whose distances spread over 8 decades: face areas (products of two) spread
    over 16, with both windings.  Every rim vertex is in many faces too.  The faces come from mesh_attr_model.fan_indices."""
    v = np.zeros((rim + 1, 14))
    d = rng.standard_normal((rim, 3))
    v[1:, 0:3] = d / np.linalg.norm(d, axis=1)[:, None] * 10.0 ** rng.uniform(-4, 4, (rim, 1))
    v[1:, 6:8] = rng.uniform(-1, 1, (rim, 2)) * 10.0 ** rng.uniform(-2, 2, (rim, 1))
    v[0, 6:8] = [0.25, 0.5]
    return v, FanFaces(nfaces, rim, 1000 + nfaces)


class FanFaces:
    def __init__(self, nfaces, rim, seed):
        self.key = [nfaces, rim, seed]
        self.i = mesh_attr_model.fan_indices(nfaces, rim, seed)
        assert (self.i[:, 1] != self.i[:, 2]).all() and self.i[:, 1:].min() >= 1 and self.i.max() <= rim


def normal_cases(rng):
    z14 = lambda n: np.zeros((n, 14))
    out = []
    out.append(("one_face_on_one_vertex", z14(1), [[0, 0, 0]], 6))
    tri = z14(3); tri[:, 0:3] = [[0, 0, 0], [1, 0.25, 0], [0.5, 2, -0.125]]
    out.append(("proper_triangle", tri, [[0, 1, 2]], 14))
    v = z14(6); v[:, 0:3] = rng.standard_normal((6, 3)); v[:, 6:] = rng.standard_normal((6, 8))
    out.append(("vertices_in_no_face", v, [[4, 1, 2]], 14))
    v = z14(5); v[:, 0:3] = rng.standard_normal((5, 3))
    out.append(("vertex_named_twice", v, [[0, 1, 1], [1, 2, 3], [3, 3, 1], [1, 3, 4], [2, 2, 2], [4, 1, 0]], 6))
    v = z14(3); v[:, 0:3] = rng.standard_normal((3, 3))
    out.append(("cancel_exactly", v, [[0, 1, 2], [0, 2, 1]], 6))
    # one face in the y/z plane: its vector is (s, 0, 0), so a sum that passes `norm > 0.001` ends as (1, 0, 0) and one that does not
    # as the fallback (0, 0, 1) - the two branches cannot be mistaken for one another (main() asserts that they differ)
    for name, s in (("sum_below_threshold", 0.0009), ("sum_just_below_threshold", math.nextafter(0.001, 0.0)), ("sum_at_threshold", 0.001),
                    ("sum_just_above_threshold", math.nextafter(0.001, 1.0)), ("sum_above_threshold", 0.0011)):
        v = z14(3); v[1, 1] = s; v[2, 2] = 1.0
        out.append((name, v, [[0, 1, 2]], 9))
    v = z14(4); v[:, 0:3] = rng.standard_normal((4, 3)); v[:, 3:6] = [[0.001, 0, 0], [0, -2, 0], [0.0006, 0.0006, 0.0006], [1e-3, 1e-9, 0]]
    out.append(("not_needed_all_long_enough", v, [[0, 1, 2], [1, 2, 3]], 9))
    v = z14(4); v[:, 0:3] = rng.standard_normal((4, 3)); v[:, 3:6] = [[1, 0, 0], [math.nan, 0, 0], [0, 1, 0], [0, 0, -1]]
    out.append(("not_needed_nan_normal", v, [[0, 1, 2], [1, 2, 3]], 6))
    v = z14(5); v[:, 0:3] = rng.standard_normal((5, 3)); v[:, 3:6] = [0, 0.5, 0]; v[4, 3:6] = [0.000999, 0, 0]
    out.append(("needed_by_the_last_vertex_only", v, rng.integers(0, 5, (4, 3)), 6))
    v = z14(1); v[0, 3:6] = [0.0, 0.0, 0.0]
    out.append(("no_faces", np.concatenate([v, tri]), np.zeros((0, 3), np.int64), 6))
    for n in (300, 5000):
        v, i = fan(rng, n)
        out.append(("fan_%d" % n, v, i, 6))
    # cross = (-0.0, +0.0, 1): the sum starts at +0.0, and +0.0 + -0.0 is +0.0 - starting from the first face vector would keep -0.0
    v = z14(3); v[:, 0:3] = [[0, 0, 0], [1, -1, 0], [0, 1, 0]]
    out.append(("negative_zero_component", v, [[0, 1, 2]], 6))
    v = z14(12); v[:, 0:3] = rng.standard_normal((12, 3)); v[:, 6:] = rng.standard_normal((12, 8))
    out.append(("stride_17", np.concatenate([v, rng.standard_normal((12, 3))], axis=1), rng.integers(0, 12, (30, 3)), 17))
    return out


def tangent_cases(rng):
    out = []
    # one triangle per value of r: uv (0,0), (1,0), (0,r) give r = 1 * r - 0 * 0 exactly
    rs = [1e-8, -1e-8, math.nextafter(1e-8, 0.0), math.nextafter(-1e-8, 0.0), math.nextafter(1e-8, 1.0), 0.0, -0.0, math.nan, 0.5]
    v = np.zeros((3 * len(rs), 14)); i = []
    for k, r in enumerate(rs):
        p = rng.standard_normal((3, 3))
        v[3 * k:3 * k + 3, 0:3] = p; v[3 * k:3 * k + 3, 3:6] = rng.standard_normal((3, 3))
        v[3 * k + 1, 6:8] = [1.0, 0.0]; v[3 * k + 2, 6:8] = [0.0, r]
        i.append([3 * k, 3 * k + 1, 3 * k + 2])
    out.append(("r_at_the_threshold", v, i, 14))
    v = np.zeros((3, 14)); v[:, 0:3] = [[0, 0, 0], [2, 0, 0], [0, 3, 0]]; v[:, 3:6] = [[1, 0, 0], [0, 0, 1], [0.5, 0, 0]]
    v[1, 6:8] = [1.0, 0.0]; v[2, 6:8] = [0.0, 1.0]
    out.append(("tangent_parallel_to_normal", v, [[0, 1, 2]], 14))
    v = rng.standard_normal((6, 14)); v[:, 8:] = 0.0; v[2, 3:6] = [0.0005, 0.0005, 0.0005]; v[4, 3:6] = 0.0
    out.append(("normal_shorter_than_threshold", v, [[0, 1, 2], [2, 3, 4], [4, 5, 0]], 14))
    v = rng.standard_normal((8, 14)); v[:, 8:11] = rng.standard_normal((8, 3)) + 2.0
    out.append(("not_needed", v, rng.integers(0, 8, (10, 3)), 14))
    v = rng.standard_normal((8, 14)); v[:, 8:11] = 1.0; v[3, 8] = math.nan
    out.append(("not_needed_nan_tangent", v, rng.integers(0, 8, (10, 3)), 14))
    v = rng.standard_normal((5, 14)); v[:, 8:11] = [0, 0, 2]; v[4, 8:11] = [0, 0.000999, 0]
    out.append(("needed_by_the_last_vertex_only", v, rng.integers(0, 5, (4, 3)), 14))
    v = rng.standard_normal((7, 14)); v[:, 8:] = 0.0
    out.append(("vertices_in_no_face_and_named_twice", v, [[0, 1, 2], [2, 2, 1], [1, 2, 3], [3, 0, 3]], 14))
    for n in (300, 5000):
        v, i = fan(rng, n)
        v[:, 3:6] = rng.standard_normal((v.shape[0], 3))
        out.append(("fan_%d" % n, v, i, 14))
    # the face's tangent is (-0.0, 2, 0) and the normal (0, 0, 1): a sum that starts at +0.0 ends in tangent.x = +0.0
    v = np.zeros((3, 14)); v[:, 0:3] = [[0, 0, 0], [-0.0, 2, 0], [0, 0, 3]]; v[:, 3:6] = [0, 0, 1]; v[1, 6:8] = [1.0, 0.0]; v[2, 6:8] = [0.0, 1.0]
    out.append(("negative_zero_component", v, [[0, 1, 2]], 14))
    v = rng.standard_normal((12, 17)); v[:, 8:14] = 0.0
    out.append(("stride_17", v, rng.integers(0, 12, (30, 3)), 17))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    objs = [os.path.join(ROOT, "oracle", "_ref", o) for o in ("our_gl.o", "tgaimage.o", "model.o", "model_manager.o")]
    assert all(os.path.exists(o) for o in objs), "oracle/_ref objects missing: run `make -C oracle ref REF=<reference tree>`"
    rng = np.random.default_rng(20261)
    cases = [("normals",) + c for c in normal_cases(rng)] + [("tangents",) + c for c in tangent_cases(rng)]
    lines, kept = [], []
    for kind, name, v, i, stride in cases:
        fan_key = i.key if isinstance(i, FanFaces) else None
        v = np.asarray(v, np.float64); i = np.asarray(i.i if fan_key else i, np.int64).reshape(-1, 3)
        if v.shape[1] < stride:
            v = np.concatenate([v, np.zeros((v.shape[0], stride - v.shape[1]))], axis=1)
        v = np.ascontiguousarray(v[:, :stride])
        w = min(stride, 14)
        rec = np.zeros((v.shape[0], 14)); rec[:, :w] = v[:, :w]
        lines.append("%s %d %d %s %s" % (kind, v.shape[0], i.shape[0], " ".join(hx(rec)), " ".join(str(int(x)) for x in i.reshape(-1))))
        kept.append((kind, name, v, i, stride, w, fan_key))
    with tempfile.TemporaryDirectory() as d:
        driver = os.path.join(d, "mesh_attr_ref_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I" + ref,
                        "-I" + os.path.join(ROOT, "oracle", "assimp_standin"), os.path.join(ROOT, "tests", "host", "mesh_attr_ref_driver.cpp")]
                       + objs + ["-o", driver, "-lm"], check=True)
        p_in, p_out = os.path.join(d, "cases.txt"), os.path.join(d, "results.txt")
        with open(p_in, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run([driver, p_in, p_out], check=True)
        res = open(p_out).read().splitlines()
    assert len(res) == len(lines)
    golden, thresholds = [], {}
    for (kind, name, v, i, stride, w, fan_key), r in zip(kept, res):
        tok = r.split()
        generated = int(tok[0])
        got = np.array([float.fromhex(t) for t in tok[1:]]).reshape(-1, 14)
        out = v.copy(); out[:, :w] = got[:, :w]
        model = mesh_attr_model.generate_normals if kind == "normals" else mesh_attr_model.compute_tangents
        m_out, m_gen = model(v, i)
        assert m_gen == bool(generated) and np.array_equal(m_out.view(np.uint64), out.view(np.uint64)), (kind, name)
        if generated:
            assert not np.isnan(out[:, 3:6] if kind == "normals" else out[:, 8:14]).any(), (kind, name)      # NaN bits differ between machines
        if name.startswith("fan_"):
            # the ordering tests rest on this: the same face vectors summed in reverse order give other bits at the centre.  The reversed
            # sum comes from the Python model, not from the reference: that is sound only because the model has just been asserted equal
            # to the reference, bit for bit, on this very mesh in forward order - keep that assertion in front of this one
            r_out, _ = model(v, i[::-1])
            cols = slice(3, 6) if kind == "normals" else slice(8, 14)
            assert not np.array_equal(r_out[0, cols].view(np.uint64), out[0, cols].view(np.uint64)), (kind, name, "order does not show: replace this fan")
        if kind == "normals" and name.startswith("sum_"):
            thresholds[name] = out[:, 3:6].copy()
        lo, hi = (3, 6) if kind == "normals" else (8, 14)
        rest = [c for c in range(stride) if not lo <= c < hi]
        assert np.array_equal(out[:, rest].view(np.uint64), v[:, rest].view(np.uint64)), (kind, name, "the reference wrote another field")
        golden.append(dict(name=name, kind=kind, stride=stride, v=hx(v), i=dict(fan=fan_key) if fan_key else [int(x) for x in i.reshape(-1)],
                           generated=generated, out=hx(out[:, lo:hi])))
        print("%-8s %-36s nv=%-4d nf=%-5d stride=%-2d generated=%d" % (kind, name, v.shape[0], i.shape[0], stride, generated))
    # the cases around `norm(sum) > 0.001` show which branch was taken: normalised (1, 0, 0) above, the fallback (0, 0, 1) below
    assert (thresholds["sum_above_threshold"] == [1.0, 0.0, 0.0]).all() and (thresholds["sum_just_above_threshold"] == [1.0, 0.0, 0.0]).all()
    assert (thresholds["sum_below_threshold"] == [0.0, 0.0, 1.0]).all() and (thresholds["sum_just_below_threshold"] == [0.0, 0.0, 1.0]).all()
    path = os.path.join(HERE, "mesh_attr_golden.json")
    with open(path, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
    print(len(golden), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
