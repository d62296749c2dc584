"""Instanced draws without a GPU (include/trgl.h: trgl_draw_instanced): the numpy model's matrix product against the reference's own
geometry.h, the vertex-shader prelude with its three new members, the exported symbols, the mirrored kernel sizes, and a self-check
that the shapes of tests/test_instanced_gpu.py reach the branches they are meant for."""
import os
import re

import numpy as np

import instance_model as M
import instanced_cases as IC
import vertex_shader_sources as V
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_model_matrix_product_equals_the_reference_operator():
    """tests/golden/instance_matmul_golden.npz (make_instance_golden.py): A * B by geometry.h:196-205, on matrices with signed zeros,
    infinities and denormals.  Bit for bit where the product is a number; NaN where it is NaN."""
    g = np.load(os.path.join(HERE, "golden", "instance_matmul_golden.npz"))
    ab, want = g["ab"].view(np.float64), g["c"]
    assert ab.shape[0] >= 64 and want.shape == (ab.shape[0], 16)
    f = ab.reshape(-1)
    assert (np.signbit(f) & (f == 0)).any() and np.isinf(f).any() and ((f != 0) & (np.abs(f) < 2.3e-308)).any()
    w = want.view(np.float64)
    # (a sum that starts from +0.0 is never -0.0 under round-to-nearest: zeros of products with negative-zero terms come out positive)
    assert (w == 0).sum() >= 16 and not (np.signbit(w) & (w == 0)).any()
    for k in range(ab.shape[0]):
        got = M.mat_product(ab[k, 0], ab[k, 1]).reshape(16)
        nan = np.isnan(got)
        assert np.array_equal(nan, np.isnan(w[k])), k
        assert np.array_equal(got.view(np.uint64)[~nan], want[k][~nan]), k


def test_product_starts_from_positive_zero():
    """0.0 + (-0.0) is +0.0: a sum of four negative zeros is +0.0, as `result[i][j] = 0; result[i][j] += ...` leaves it."""
    a = np.zeros((4, 4)); a[0, :] = -0.0
    b = np.ones((4, 4)); b[:, 0] = 0.0
    assert not np.signbit(M.mat_product(a, b)[0, 0])


def test_vertex_shader_sees_the_instance_members():
    """A source that reads in.instance, in.inst and in.inst_stride compiles (the same source compiles for both kernels of the code
    object); without the members it would not."""
    for name, (src, K) in IC.STAGES.items():
        ok, log = api.vertex_shader_compile(src, K)
        assert ok, f"{name}: {log}"
    ok, log = api.vertex_shader_compile(V.RESTATED, 24)          # a source from before the members still does
    assert ok, log
    ok, log = api.vertex_shader_compile(IC.MOVE.replace("in.inst_stride", "in.no_such_member"), 0)
    assert not ok and "no_such_member" in log


def test_symbols_and_mirrored_sizes():
    L = api.load_library()
    for name in ("trgl_draw_instanced", "trgl_instance_stage"):
        assert name in api.SYMBOLS and hasattr(L, name)
    text = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()
    for name, value in (("INST_BLOCK", api.INST_BLOCK), ("INST_SCAN_CHUNK", api.INST_SCAN_CHUNK), ("INST_VS_FACES", api.INST_VS_FACES)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    dev = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "trgl_device.h")).read()
    assert int(re.search(r"#define TRGL_VERTEX_USER_FACES (\d+)", dev).group(1)) == api.INST_VS_FACES


def _drawn(s):
    return len(M.compact(IC.visible(s.pattern, s.n), s.n))


def test_gpu_shapes_reach_their_branches():
    S = IC.SHAPES
    B = IC.BLOCK_FACES
    assert {s.nf for s in S.values()} >= {1, 2, 12, 37, 64, 65}
    assert {s.n for s in S.values()} >= {0, 1, 3, 64, 257, IC.BIG}
    assert {s.pattern for s in S.values()} == set(IC.PATTERNS)
    assert {s.stride for s in S.values()} >= {16, 19}
    for stage in ("builtin", "k0", "k5", "k64"):
        mine = [s for s in S.values() if s.stage == stage]
        assert {s.inst_device for s in mine} == {False, True}, stage
        # a partial last block, and more than one block
        assert any(_drawn(s) * s.nf % B not in (0,) and _drawn(s) * s.nf > B for s in mine), stage
    # a block of 64 output faces spanning at least 3 instances, in the built-in and in a user stage
    assert any(s.stage == "builtin" and s.nf * 3 <= B - 2 and _drawn(s) >= 6 for s in S.values())
    assert any(s.stage != "builtin" and s.nf * 3 <= B - 2 and _drawn(s) >= 6 for s in S.values())
    # an odd number of varying doubles in the last block (the 8-byte tail store of the user kernel)
    assert any(s.stage == "k5" and (_drawn(s) * s.nf % B) * 5 % 2 == 1 for s in S.values())
    # more instances than one scan block, and than one block of block sums - in device memory, where the scan runs
    assert any(s.inst_device and s.pattern not in ("absent",) and IC.SCAN_BLOCK < s.n <= IC.TWO_LEVEL for s in S.values())
    big = [s for s in S.values() if s.inst_device and s.pattern != "absent" and s.n > IC.TWO_LEVEL]
    assert big and all(s.n % IC.SCAN_BLOCK != 0 for s in big)
    assert {s.stage for s in big} >= {"builtin", "k0"}
    # bytes whose bit 0 disagrees with "non-zero"
    v = IC.visible("random", 257)
    assert v[0] == 0xFE and v[1] == 0xFF and len(set(v.tolist())) > 100
    # nothing to draw: all0 and n = 0
    assert any(s.n and _drawn(s) == 0 for s in S.values()) and any(s.n == 0 for s in S.values())
    # a call without an instance array
    assert any(s.stride == 0 for s in S.values())


def test_model_rows_of_one_instance_are_the_vertex_stage():
    """With M = identity the model's rows are orc.vertex_stage's; with visible bytes they follow the drawn instances in order."""
    from oracle import orc
    from tinyrenderder_amd import scenes
    hd = scenes.head_standin(1, 64, 64)
    verts, idx = IC.cube(8, 0.5)
    inst = IC.instances(5, 19)
    inst[2, :16] = np.eye(4).reshape(16)
    vis = np.array([0, 2, 0xFF, 1, 0xFE], np.uint8)
    clip, vary, drawn = M.builtin_rows(hd["model_view"], hd["projection"], verts, idx, inst, vis)
    assert drawn.tolist() == [2, 3] and clip.shape == (24, 12) and vary.shape == (24, 24)
    c0, v0 = orc.vertex_stage(hd["model_view"], hd["projection"], verts, idx)
    assert np.array_equal(clip[:12].view(np.uint64), c0.view(np.uint64)) and np.array_equal(vary[:12].view(np.uint64), v0.view(np.uint64))
    assert not np.array_equal(clip[12:], c0)
    assert M.colors(drawn, 12, instance_colors=np.arange(5, dtype=np.uint32)).tolist() == [2] * 12 + [3] * 12
    assert M.colors(drawn, 12, face_colors=np.arange(12, dtype=np.uint32)).tolist() == list(range(12)) * 2
    assert M.colors(drawn, 12) is None
