"""trgl_instance_boxes and trgl_frustum_boxes in host memory (include/trgl.h), their Python wrappers and the shim functions, without a GPU.

The yardstick is the reference's own compiled code: tests/golden/scene_golden.json holds results of AABB::transform (geometry.h:297-327)
and Frustum::intersects (our_gl.cpp:264-280), and the array calls must reproduce them bit for bit - all cases in one call, and one by
one.  tests/scene_model.py is pinned to the same goldens by tests/test_scene_cpu.py; the seeded cases of tests/instance_cull_cases.py are
proved on that model alone to reach what they are meant for (a zero w, a negative w, NaN positions, a tie of zeros, a box at distance
exactly 0, a zero normal, each plane alone), then the host paths are held to the model on them.  The scene of the end-to-end GPU test is
checked here too: it has an instance the frustum rejects that occlusion would have drawn, one that occlusion hides, and one that is drawn."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import instance_cull_cases as CC
import occlusion_model as om
import scene_model
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_INVALID, E_UNSUPPORTED = -1, -5
POISON = 0x10                       # a pointer that faults when it is read or written


def same_bits(a, b):
    a, b = CC.bits(a), CC.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ---- against the reference's compiled code ----------------------------------------------------------------------------------------
def test_all_golden_transforms_in_one_call():
    local, mats, want = CC.golden_transform()
    assert len(local) >= 30
    got = api.instance_boxes(local, mats)                      # local_stride 6, instance_stride 16
    assert got.shape == want.shape and same_bits(got, want), np.argwhere(CC.bits(got) != CC.bits(want))[:5]


def test_golden_transforms_one_by_one_with_one_local_box():
    local, mats, want = CC.golden_transform()
    for i in range(len(local)):
        got = api.instance_boxes(local[i], mats[i:i + 1])      # local_stride 0
        assert same_bits(got, want[i]), (i, got, want[i])


def test_golden_intersects_set_and_merge():
    groups = CC.golden_intersect_groups()
    seen = set()
    for planes, boxes, result in groups:
        got = api.frustum_boxes(planes, boxes)
        assert np.array_equal(got, np.where(result == 1, api.OCCL_VISIBLE, api.OCCL_OUTSIDE)), (planes, got, result)
        seen |= set(result.tolist())
        for prior in CC.PRIOR_BYTES:
            codes = np.full(len(boxes), prior, np.uint8)
            back = api.frustum_boxes(planes, boxes, codes, merge=True)
            assert back is codes
            assert np.array_equal(codes, np.where(result == 1, prior, api.OCCL_OUTSIDE)), (prior, codes, result)
    assert seen == {0, 1} and sum(len(g[1]) for g in groups) == len(CC.GOLDEN["intersect"])


# ---- the seeded cases reach what they are meant for (on the model alone) -------------------------------------------------------
def test_special_transform_cases_reach_their_corners():
    sp = CC.special_transform_cases()
    box = {k: CC.model_boxes(l, m[None])[0] for k, (l, m) in sp.items()}

    def w_of(name):                                            # the eight w of the case, in corner order
        l, m = sp[name]
        return [m[12] * (l[3] if k & 1 else l[0]) + m[13] * (l[4] if k & 2 else l[1]) + m[14] * (l[5] if k & 4 else l[2]) + m[15] for k in range(8)]

    assert 0.0 in w_of("w_zero") and np.isinf(box["w_zero"]).any() and not np.isnan(box["w_zero"]).any()
    assert all(w < 0 for w in w_of("w_negative")) and np.isfinite(box["w_negative"]).all()
    assert np.array_equal(box["all_nan"], [1e9] * 3 + [-1e9] * 3)
    assert box["nan_row"][1] == 1e9 and box["nan_row"][4] == -1e9 and box["nan_row"][0] == -1.0 and box["nan_row"][3] == 1.0
    neg, pos = box["zero_tie_neg_first"], box["zero_tie_pos_first"]
    assert neg[0] == 0.0 and pos[0] == 0.0 and neg[3] == 0.0 and pos[3] == 0.0
    assert math.copysign(1.0, neg[0]) == -1.0 and math.copysign(1.0, neg[3]) == -1.0, "the earlier zero (-0.0) must stay"
    assert math.copysign(1.0, pos[0]) == 1.0 and math.copysign(1.0, pos[3]) == 1.0, "the earlier zero (+0.0) must stay"
    far = box["beyond_start_values"]
    assert far[0] == 1e9 and far[3] > 1e9 and far[4] == -1e9 and far[1] < -1e9
    for b in box.values():
        assert not np.isnan(b).any(), "an output is never NaN"


def test_seeded_transform_cases_hold_every_special_case_and_w_crossing_zero():
    local, inst = CC.seeded_transform_cases(256, 17, 7)
    boxes = CC.model_boxes(local, inst)
    assert np.isinf(boxes).any() and (boxes == 1e9).any() and (boxes == -1e9).any() and not np.isnan(boxes).any()
    n_golden = len(CC.GOLDEN["transform"])
    assert same_bits(boxes[:n_golden], CC.golden_transform()[2])
    signs = np.sign(inst[:, 12:16] @ np.ones(4))               # rough: random projective rows exist on both sides
    assert (signs > 0).any() and (signs < 0).any()


def test_frustum_cases_reach_their_corners():
    on, off = CC.touching_boxes()
    assert scene_model.frustum_intersects(CC.CUBE_PLANES, on[:3], on[3:]) and not scene_model.frustum_intersects(CC.CUBE_PLANES, off[:3], off[3:])
    pl = CC.CUBE_PLANES[api.FRUSTUM_RIGHT]
    assert (pl[0] * on[0] + pl[1] * on[4]) + pl[2] * on[5] + pl[3] == 0.0, "the touching box is at distance exactly 0"
    for i, b in enumerate(CC.only_plane_boxes()):
        assert CC.rejecting_planes(CC.CUBE_PLANES, b) == [i], (i, b)
    zn_all, zn_none = CC.zero_normal_planes()
    assert not zn_all[api.FRUSTUM_TOP, :3].any() and not zn_none[api.FRUSTUM_TOP, :3].any()
    inside = np.array([-0.25] * 3 + [0.25] * 3)
    assert CC.rejecting_planes(zn_all, inside) == [api.FRUSTUM_TOP] and CC.rejecting_planes(zn_none, inside) == []
    for planes, boxes in CC.seeded_frustum_cases(257):
        hit = CC.model_hits(planes, boxes)
        if planes is not zn_all:
            assert hit.any() and not hit.all(), "a seeded frustum case needs both answers"
        else:
            assert not hit.any()


# ---- the host paths against the model on the seeded cases -----------------------------------------------------------------------
@pytest.mark.parametrize("stride,local_stride", [(16, 6), (17, 7), (24, 0)])
def test_host_boxes_equal_the_model_on_the_seeded_cases(stride, local_stride):
    local, inst = CC.seeded_transform_cases(300, stride, max(local_stride, 6))
    if local_stride == 0:
        for name, (l, m) in CC.special_transform_cases().items():
            one = inst.copy()
            one[:, :16] = m
            one[::2, :16] = inst[::2, :16]
            assert same_bits(api.instance_boxes(l, one), CC.model_boxes(l, one)), name
    else:
        assert same_bits(api.instance_boxes(local, inst), CC.model_boxes(local, inst))


def test_host_codes_equal_the_model_on_the_seeded_cases():
    rng = np.random.default_rng(5)
    for planes, boxes in CC.seeded_frustum_cases(257):
        assert np.array_equal(api.frustum_boxes(planes, boxes), CC.model_codes(planes, boxes))
        prior = rng.integers(0, 256, len(boxes)).astype(np.uint8)
        prior[: len(CC.PRIOR_BYTES)] = CC.PRIOR_BYTES
        codes = prior.copy()
        api.frustum_boxes(planes, boxes, codes, merge=True)
        assert np.array_equal(codes, CC.model_codes(planes, boxes, prior))


def test_host_calls_write_exactly_n_rows():
    local, inst = CC.seeded_transform_cases(65, 17, 7)
    out = np.full((70, 6), -7.25)
    api.instance_boxes(local, inst, out=out[:65])
    assert same_bits(out[:65], CC.model_boxes(local, inst)) and (out[65:] == -7.25).all()
    planes, boxes = CC.seeded_frustum_cases(65)[0]
    codes = np.full(70, 0xA5, np.uint8)
    api.frustum_boxes(planes, boxes, codes[:65])
    assert np.array_equal(codes[:65], CC.model_codes(planes, boxes)) and (codes[65:] == 0xA5).all()


def test_the_single_box_calls_and_the_array_calls_agree():
    """trgl_aabb_transform / trgl_frustum_intersects and the array calls share scene_core.h: equal bits on the seeded cases."""
    local, inst = CC.seeded_transform_cases(120)
    boxes = api.instance_boxes(local, inst)
    for i in range(len(inst)):
        lo, hi = api.aabb_transform(local[i, :3], local[i, 3:6], inst[i, :16])
        assert same_bits(np.concatenate([lo, hi]), boxes[i]), i
    planes, fb = CC.seeded_frustum_cases(120)[0]
    codes = api.frustum_boxes(planes, fb)
    for i in range(len(fb)):
        assert api.frustum_intersects(planes, fb[i, :3], fb[i, 3:]) == (codes[i] == api.OCCL_VISIBLE), i


# ---- the scene of the end-to-end GPU test -----------------------------------------------------------------------------------------
def test_cull_scene_holds_every_kind_of_instance():
    sc = CC.cull_scene()
    lo, hi = scene_model.compute_aabb(sc["verts"])
    boxes = CC.model_boxes(np.concatenate([lo, hi]), sc["inst"])
    planes = sc["planes"]
    hit = CC.model_hits(planes, boxes)
    # the wall's depths without a GPU: the wall is the plane z = 0 over the left half of the view, so a depth image that holds its
    # NDC depth over columns 0 .. w/2 - 1 is what the rasterizer leaves up to the pixels of its edge column
    clip = sc["wall"].reshape(-1, 4)
    zw = clip[0, 2] / clip[0, 3]
    assert np.allclose(clip[:, 2] / clip[:, 3], zw)
    depth = np.full((sc["h"], sc["w"]), np.inf)
    depth[:, : sc["w"] // 2 - 1] = zw
    occl = om.codes(depth, sc["viewport"], sc["view_proj"], boxes)
    merged = np.where(hit, occl, om.OUTSIDE)
    assert ((~hit) & ((occl & 1) == 1)).any(), "no instance that the frustum rejects and occlusion would have drawn"
    assert (hit & (occl == om.HIDDEN)).any(), "no instance that occlusion hides"
    assert (hit & ((occl & 1) == 1)).sum() >= 4, "too few instances are drawn"
    assert (~hit).sum() >= 8 and 0 < (merged & 1).sum() < len(hit)
    assert CC.rejecting_planes(planes, boxes[0]) == [api.FRUSTUM_LEFT] and CC.rejecting_planes(planes, boxes[12]) == [api.FRUSTUM_RIGHT]
    assert api.FRUSTUM_NEAR in CC.rejecting_planes(planes, boxes[-1]) and occl[-1] == om.UNDECIDED      # behind the eye


# ---- errors and the n == 0 rule --------------------------------------------------------------------------------------------------
def test_error_codes_of_both_calls():
    L = api.load_library()
    local, inst = CC.seeded_transform_cases(4)
    out = np.zeros((4, 6))
    planes = np.ascontiguousarray(CC.CUBE_PLANES)
    codes = np.zeros(4, np.uint8)
    pl = planes.ctypes.data_as(C.POINTER(C.c_double))
    H, D = api.MEM_HOST, api.MEM_DEVICE

    def boxes(ls=6, st=16, n=4, mk=H, l=local.ctypes.data, i=inst.ctypes.data, o=out.ctypes.data):
        return L.trgl_instance_boxes(None, l, ls, i, st, n, mk, o)

    def frustum(n=4, mode=api.FRUSTUM_SET, mk=H, p=pl, b=out.ctypes.data, c=codes.ctypes.data):
        return L.trgl_frustum_boxes(None, p, b, n, mode, mk, c)

    assert boxes() == 0 and frustum() == 0
    assert boxes(mk=2) == E_INVALID and boxes(mk=-1) == E_INVALID and frustum(mk=2) == E_INVALID
    assert boxes(mk=D) == E_INVALID and frustum(mk=D) == E_INVALID                     # device memory needs a context
    for ls in (-1, 1, 5):
        assert boxes(ls=ls) == E_INVALID
    assert boxes(st=15) == E_INVALID and boxes(st=0) == E_INVALID and boxes(st=-16) == E_INVALID
    assert frustum(mode=2) == E_INVALID and frustum(mode=-1) == E_INVALID
    assert frustum(p=None) == E_INVALID and frustum(p=None, n=0) == E_INVALID          # planes is a scalar argument: checked before n
    assert boxes(l=None) == E_INVALID and boxes(i=None) == E_INVALID and boxes(o=None) == E_INVALID
    assert boxes(ls=0, l=None) == E_INVALID
    assert frustum(b=None) == E_INVALID and frustum(c=None) == E_INVALID
    assert boxes(n=1 << 31) == E_UNSUPPORTED and frustum(n=1 << 31) == E_UNSUPPORTED
    assert b"trgl_frustum_boxes" in L.trgl_last_error(None)


def test_n_zero_touches_no_array():
    L = api.load_library()
    pl = np.ascontiguousarray(CC.CUBE_PLANES).ctypes.data_as(C.POINTER(C.c_double))
    for ls in (0, 6, 9):
        assert L.trgl_instance_boxes(None, POISON, ls, POISON, 16, 0, api.MEM_HOST, POISON) == 0
        assert L.trgl_instance_boxes(None, None, ls, None, 16, 0, api.MEM_HOST, None) == 0
    for mode in (api.FRUSTUM_SET, api.FRUSTUM_MERGE):
        assert L.trgl_frustum_boxes(None, pl, POISON, 0, mode, api.MEM_HOST, POISON) == 0
        assert L.trgl_frustum_boxes(None, pl, None, 0, mode, api.MEM_HOST, None) == 0
    # the scalar arguments are still checked
    assert L.trgl_instance_boxes(None, POISON, 3, POISON, 16, 0, api.MEM_HOST, POISON) == E_INVALID
    assert L.trgl_instance_boxes(None, POISON, 0, POISON, 8, 0, api.MEM_HOST, POISON) == E_INVALID
    assert L.trgl_frustum_boxes(None, pl, POISON, 0, 7, api.MEM_HOST, POISON) == E_INVALID
    assert api.instance_boxes(CC.UNIT, np.zeros((0, 16))).shape == (0, 6)
    assert api.frustum_boxes(CC.CUBE_PLANES, np.zeros((0, 6))).shape == (0,)


def test_python_wrappers_refuse_what_they_cannot_pass_on():
    local, inst = CC.seeded_transform_cases(4)
    with pytest.raises(ValueError):
        api.instance_boxes(local[:3], inst)                                            # one local box per instance
    with pytest.raises(ValueError):
        api.instance_boxes(local, inst, out=np.zeros((3, 6)))
    with pytest.raises(ValueError):
        api.frustum_boxes(CC.CUBE_PLANES, np.zeros((4, 6)), merge=True)                # nothing to merge into
    with pytest.raises(ValueError):
        api.frustum_boxes(CC.CUBE_PLANES, np.zeros((4, 6)), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        api.frustum_boxes(CC.CUBE_PLANES[:5], np.zeros((4, 6)))
    with pytest.raises(api.TrglError):
        api.instance_boxes(CC.UNIT, np.zeros((4, 15)))


# ---- the shim ---------------------------------------------------------------------------------------------------------------------
def test_shim_functions_equal_the_model(tmp_path):
    """tests/host/shim_instance_cull.cpp runs gl_instance_boxes and gl_frustum_test (both forms) over the matrices and planes it reads
    and prints the results in hex; they must equal the model's."""
    exe = str(tmp_path / "shim_instance_cull")
    lib = os.path.join(ROOT, "tinyrenderder_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(HERE, "host", "shim_instance_cull.cpp"), "-o", exe,
                    "-L" + lib, "-ltrgl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    local, inst = CC.seeded_transform_cases(40)
    planes = CC.CUBE_PLANES
    prior = (np.arange(40) * 37 % 256).astype(np.uint8)
    text = " ".join(float(x).hex() for x in np.concatenate([local[0, :6], planes.reshape(-1)])) + "\n"
    text += "\n".join(" ".join(float(x).hex() for x in row[:16]) + f" {int(p)}" for row, p in zip(inst, prior)) + "\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    rows = [ln.split() for ln in res.stdout.strip().splitlines()]
    assert len(rows) == 40
    boxes = np.array([[float.fromhex(x) for x in r[:6]] for r in rows])
    want = CC.model_boxes(local[0, :6], inst)
    assert same_bits(boxes, want)
    assert np.array_equal(np.array([int(r[6]) for r in rows], np.uint8), CC.model_codes(planes, want))
    assert np.array_equal(np.array([int(r[7]) for r in rows], np.uint8), CC.model_codes(planes, want, prior))


def test_host_loops_under_the_sanitizers():
    """tests/host/instance_cull_host.cpp: the host loops of both calls over heap blocks of exactly the promised sizes, compiled with
    AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, against the single-box calls."""
    subprocess.run(["make", "-C", os.path.join(HERE, "host"), "-f", "instance_cull.mk", "instance_cull"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(HERE, "host", "instance_cull_host_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
