"""Occlusion culling of boxes on the host: trgl_occlusion_boxes_image with TRGL_MEM_HOST (plain C++, no GPU) against
tests/occlusion_model.py on random scenes and on inputs that sit on every comparison of the seven steps include/trgl.h writes down;
what a code promises, checked by pushing a box's own faces through the reference-pinned oracle; the error contract."""
import ctypes as C

import numpy as np
import pytest

import occlusion_cases as oc
import occlusion_model as om
from oracle import orc
from tinyrenderder_amd import api

E_INVALID, E_UNSUPPORTED = -1, -5
SCENES = [(200, 136, 3), (200, 136, 5), (70, 45, 3), (70, 45, 5)]
_cache = {}


def scene(w, h, seed):
    """The scene, the oracle's frame and depths of its quads, and the model's result - computed once, never modified."""
    key = (w, h, seed)
    if key not in _cache:
        sc = oc.random_scene(w, h, seed)
        o = orc.Oracle(w, h, 3, viewport=sc["viewport"])
        o.draw(orc.FLAT, sc["clip"], colors=sc["colors"])
        fb, z = o.fb.copy(), o.z.copy()
        fb.setflags(write=False); z.setflags(write=False)
        _cache[key] = (sc, fb, z, om.classify(z, sc["viewport"], sc["view_proj"], sc["boxes"]))
    return _cache[key]


def assert_code_shares(codes):
    share = np.bincount(codes, minlength=4) / len(codes)
    print("shares of HIDDEN, VISIBLE, OUTSIDE, UNDECIDED:", share)
    assert len(codes) == oc.N_BOXES and (share >= 0.10).all(), share


@pytest.mark.parametrize("case", SCENES, ids=lambda s: "%dx%d_seed%d" % s)
def test_host_codes_equal_the_model_on_random_scenes(case):
    sc, _, z, res = scene(*case)
    assert_code_shares(res.codes)                                         # asserted on the model alone
    got = api.occlusion_boxes_image(z, sc["viewport"], sc["view_proj"], sc["boxes"])
    assert got.dtype == np.uint8 and np.array_equal(got, res.codes), np.nonzero(got != res.codes)[0][:10]


@pytest.mark.parametrize("case", SCENES, ids=lambda s: "%dx%d_seed%d" % s)
def test_a_box_not_to_be_drawn_draws_nothing_through_the_oracle(case):
    """For every box whose code has bit 0 clear, the 24 proxy triangles built from the model's clip corners leave z-buffer, frame and
    fragments_drawn as they were; at least half of the VISIBLE boxes do draw (so the proxies are not simply inert)."""
    sc, fb, z, res = scene(*case)
    w, h = case[0], case[1]
    o = orc.Oracle(w, h, 3, viewport=sc["viewport"])

    def draws(i):
        o.fb[...] = fb; o.z[...] = z
        before = o.stats[1]
        o.draw(orc.FLAT, om.proxy_triangles(res.clip[i]), colors=np.full(24, 0xff00ff00, np.uint32))
        changed = o.stats[1] != before or not np.array_equal(o.z.view(np.uint64), z.view(np.uint64)) or not np.array_equal(o.fb, fb)
        assert changed == (o.stats[1] != before)                          # a fragment drawn is the only way anything changes
        return changed

    skipped = np.nonzero((res.codes & 1) == 0)[0]
    assert len(skipped) >= 0.2 * oc.N_BOXES
    wrong = [int(i) for i in skipped if draws(i)]
    assert not wrong, (len(wrong), wrong[:10], res.codes[wrong[:10]])
    visible = np.nonzero(res.codes == om.VISIBLE)[0]
    drawn = sum(draws(i) for i in visible)
    print("%d boxes with bit 0 clear drew nothing; %d of %d VISIBLE boxes draw" % (len(skipped), drawn, len(visible)))
    assert 2 * drawn >= len(visible)


THRESHOLD = oc.threshold_cases()


@pytest.mark.parametrize("case", THRESHOLD, ids=lambda c: c[0])
def test_thresholds_model_host_and_by_hand(case):
    """The model and the code could share a misreading: `want` is worked out from the header's text alone (occlusion_cases.py)."""
    name, depth, V, M, boxes, want = case
    model = om.codes(depth, V, M, boxes).tolist()
    host = api.occlusion_boxes_image(depth, V, M, boxes).tolist()
    assert model == want and host == want, (name, model, host, want)


def test_every_threshold_the_header_names_has_a_case():
    names = " ".join(c[0] for c in THRESHOLD)
    for part in ("pixel_holds_zq", "pixel_above_zq", "w_at_guard", "w_above_guard", "z_range_limits", "all_nan", "nan_with_inf_at", "zero_plus_against_minus",
                 "zero_minus_against_plus", "screen_1e300", "integer_bounds_witness_2_1", "empty_on_each_side", "w_is_zero"):
        assert part in names, part


def _call(depth, w, h, V, M, boxes, n, codes, kind=api.MEM_HOST):
    L = api.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    return L.trgl_occlusion_boxes_image(None, ptr(depth), w, h, dp(V), dp(M), ptr(boxes), n, ptr(codes), kind)


def test_error_contract():
    depth, boxes, codes = np.zeros((3, 4)), np.array([oc.box(0, 1, 0, 1)]), np.full(3, 77, np.uint8)
    I = np.eye(4)
    assert _call(depth, 4, 3, I, I, boxes, 1, codes) == 0 and codes.tolist() == [oc.VISIBLE, 77, 77]     # zq < 0.0; exactly n bytes are written
    for d, b, c in ((None, boxes, codes), (depth, None, codes), (depth, boxes, None)):
        assert _call(d, 4, 3, I, I, b, 1, c) == E_INVALID
    assert _call(depth, 4, 3, None, I, boxes, 1, codes) == E_INVALID and _call(depth, 4, 3, I, None, boxes, 1, codes) == E_INVALID
    assert _call(depth, -4, 3, I, I, boxes, 1, codes) == E_INVALID and _call(depth, 4, -3, I, I, boxes, 1, codes) == E_INVALID
    assert _call(depth, 4, 3, I, I, boxes, 1, codes, kind=2) == E_INVALID
    assert _call(depth, 4, 3, I, I, boxes, 1, codes, kind=api.MEM_DEVICE) == E_INVALID                    # no context
    assert _call(depth, 65536, 32768, I, I, boxes, 1, codes) == E_UNSUPPORTED                             # 2^31 pixels
    assert _call(depth, 4, 3, I, I, boxes, 2 ** 31, codes) == E_UNSUPPORTED
    assert api.load_library().trgl_last_error(None)


def test_nothing_to_do_touches_nothing():
    I = np.eye(4)
    assert _call(None, 4, 3, I, I, None, 0, None) == 0                                                    # n == 0: no array is looked at
    codes = np.full(2, 77, np.uint8)
    boxes = np.array([oc.box(0, 1, 0, 1), oc.box(0, 1, 0, 1)])
    assert _call(None, 0, 3, I, I, boxes, 2, codes) == 0 and codes.tolist() == [oc.OUTSIDE] * 2           # an empty image: depth is not read
    assert api.occlusion_boxes_image(np.zeros((3, 4)), I, I, np.zeros((0, 6))).shape == (0,)
    with pytest.raises(ValueError):
        api.occlusion_boxes_image(np.zeros((3, 4)), I, I, np.zeros((2, 5)))


def test_symbols_and_constants():
    assert {"trgl_occlusion_boxes_image", "trgl_occlusion_boxes"} <= set(api.SYMBOLS)
    assert (api.OCCL_HIDDEN, api.OCCL_VISIBLE, api.OCCL_OUTSIDE, api.OCCL_UNDECIDED) == (om.HIDDEN, om.VISIBLE, om.OUTSIDE, om.UNDECIDED) == (0, 1, 2, 3)
