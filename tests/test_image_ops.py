"""trgl_gaussian_kernel / trgl_image_blur / trgl_image_scale in host memory, the numpy model and the shim's TGAImage::gaussian_blur /
scale against tests/golden/image_ops_golden.npz: the reference's own compiled tgaimage.cpp:246-324 (tests/golden/make_image_ops_golden.py).
No GPU here."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import image_ops_model
from tinyrenderder_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_image_ops")
G = np.load(os.path.join(ROOT, "tests", "golden", "image_ops_golden.npz"))
META = json.loads(str(G["meta"]))
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5


def golden_weights(radius):
    return G["weights/%d" % radius].view(np.float32)


def test_gaussian_kernel_gives_the_golden_bits():
    """First, and with its own message: a libm whose expf differs on this machine shows up here, not as a wrong blur further down."""
    for r in META["radii"]:
        got = api.gaussian_kernel(r)
        assert got.dtype == np.float32 and got.shape == (2 * r + 1,)
        assert np.array_equal(got.view(np.uint32), G["weights/%d" % r]), \
            "trgl_gaussian_kernel(%d) differs from the bits the golden was made with: this machine's std::exp(float) is another one" % r


def test_golden_holds_what_the_issue_lists():
    assert {1, 2, 3, 5, 9, 40, 70, META["switch_radius"], META["switch_radius"] + 1} == set(META["radii"])
    shapes = {n: G["img/" + n].shape for n in META["images"]}
    assert {shapes["random_bpp%d" % b] for b in (1, 3, 4)} == {(41, 67, 1), (41, 67, 3), (41, 67, 4)}
    assert shapes["one_pixel"][:2] == (1, 1) and shapes["one_column"][:2] == (23, 1) and shapes["one_row"][:2] == (1, 23)
    assert (G["img/all_255"] == 255).all() and not G["img/all_0"].any() and set(np.unique(G["img/checker"])) == {0, 255}
    assert max(shapes["random_bpp3"][:2]) < 70                                   # radius 70 exceeds both dimensions


@pytest.mark.parametrize("name", META["images"])
def test_host_blur_equals_the_reference(name):
    img = G["img/" + name]
    for r in META["radii"]:
        want = G["blur/%s/%d" % (name, r)]
        assert np.array_equal(api.image_blur(img, r), want), (name, r)
        assert np.array_equal(image_ops_model.gaussian_blur(img, golden_weights(r)), want), (name, r, "numpy model")


def test_blur_is_not_the_identity_on_the_golden():
    assert not np.array_equal(G["blur/random_bpp3/1"], G["img/random_bpp3"])
    assert not np.array_equal(G["blur/random_bpp3/32"], G["blur/random_bpp3/33"])


@pytest.mark.parametrize("k", range(len(META["scale"])))
def test_host_scale_equals_the_reference(k):
    name, w2, h2, ok = META["scale"][k]
    img, want = G["img/" + name], G["scale/%d" % k]
    if not ok:                                                                  # the reference returned false and left the image alone
        assert np.array_equal(want, img)
        assert image_ops_model.scale(img, w2, h2) is None
        with pytest.raises(api.TrglError, match=r"\(-1\)"):
            api.image_scale(img, w2, h2)
        return
    assert want.shape == (h2, w2, img.shape[2])
    assert np.array_equal(api.image_scale(img, w2, h2), want)
    assert np.array_equal(image_ops_model.scale(img, w2, h2), want)


def test_radius_not_positive_leaves_the_bytes_alone():
    L = api.load_library()
    img = G["img/random_bpp4"].copy()
    for r in (0, -1, -46341):
        assert L.trgl_image_blur(None, img.ctypes.data, 67, 41, 4, r, api.MEM_HOST) == 0
        assert np.array_equal(img, G["img/random_bpp4"])
    # an empty image: nothing is read, a null pointer is fine (tgaimage.cpp:272)
    assert L.trgl_image_blur(None, None, 0, 5, 3, 2, api.MEM_HOST) == 0
    assert L.trgl_image_blur(None, None, 5, 0, 3, 2, api.MEM_HOST) == 0
    assert L.trgl_image_blur(None, None, 5, 5, 3, 0, api.MEM_HOST) == 0


def test_return_codes():
    L = api.load_library()
    img = np.zeros((4, 5, 3), np.uint8)
    out = np.zeros((8, 10, 3), np.uint8)
    p, q = img.ctypes.data, out.ctypes.data
    w = np.zeros(3, np.float32)
    assert L.trgl_gaussian_kernel(1, w.ctypes.data) == 0
    assert L.trgl_gaussian_kernel(0, w.ctypes.data) == E_INVALID and L.trgl_gaussian_kernel(1, None) == E_INVALID
    assert L.trgl_gaussian_kernel(46341, w.ctypes.data) == E_UNSUPPORTED
    big = np.zeros(2 * 46340 + 1, np.float32)
    assert L.trgl_gaussian_kernel(46340, big.ctypes.data) == 0 and np.isfinite(big).all() and big[46340] > 0
    # blur
    for bpp in (0, 2, 5):
        assert L.trgl_image_blur(None, p, 5, 4, bpp, 1, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_blur(None, None, 5, 4, 3, 1, api.MEM_HOST) == E_INVALID            # null with a non-empty image
    assert L.trgl_image_blur(None, p, 5, 4, 3, 1, 2) == E_INVALID                          # bad mem_kind
    assert L.trgl_image_blur(None, p, -5, 4, 3, 1, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_blur(None, p, 5, 4, 3, 1, api.MEM_DEVICE) == E_INVALID             # device memory needs a context
    assert L.trgl_image_blur(None, p, 5, 4, 3, 46341, api.MEM_HOST) == E_UNSUPPORTED
    assert L.trgl_image_blur(None, p, 1 << 15, 1 << 15, 3, 1, api.MEM_HOST) == E_UNSUPPORTED   # w * h * bpp > INT_MAX; refused before anything is read
    assert not img.any()
    # scale
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, 10, 8, api.MEM_HOST) == 0
    for w2, h2 in ((0, 8), (10, 0), (-1, 8), (10, -1)):
        assert L.trgl_image_scale(None, p, 5, 4, 3, q, w2, h2, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_scale(None, p, 0, 4, 3, q, 10, 8, api.MEM_HOST) == E_INVALID       # empty source
    assert L.trgl_image_scale(None, p, 5, 0, 3, q, 10, 8, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_scale(None, p, 5, 4, 2, q, 10, 8, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_scale(None, None, 5, 4, 3, q, 10, 8, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_scale(None, p, 5, 4, 3, None, 10, 8, api.MEM_HOST) == E_INVALID
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, 10, 8, 7) == E_INVALID
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, 10, 8, api.MEM_DEVICE) == E_INVALID
    assert L.trgl_image_scale(None, p, 5, 4, 3, p + 3, 2, 2, api.MEM_HOST) == E_INVALID    # overlap
    # the reference's int arithmetic would overflow; refused before anything is touched
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, (1 << 29) + 1, 1, api.MEM_HOST) == E_UNSUPPORTED   # (w2 - 1) * w
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, 1, (1 << 29) + 1, api.MEM_HOST) == E_UNSUPPORTED   # (h2 - 1) * h
    assert L.trgl_image_scale(None, p, 5, 4, 3, q, 1 << 15, 1 << 15, api.MEM_HOST) == E_UNSUPPORTED   # w2 * h2 * bpp
    assert L.trgl_framebuffer_blur(None, 1) == E_INVALID                                   # no context


def test_shim_image_members_match_the_reference(tmp_path):
    """examples/demo_image_ops.cpp in host mode: TGAImage::gaussian_blur and TGAImage::scale of shim/trgl_image.h, as a caller of the
    reference's class would use them."""
    assert os.path.exists(DEMO), "examples/demo_image_ops not built: run __graft_entry__.build()"
    img = G["img/random_bpp3"]
    k = next(i for i, c in enumerate(META["scale"]) if c[0] == "random_bpp3" and c[3] and (c[1], c[2]) == (40, 30))
    cases = [(9, 40, 30, G["blur/random_bpp3/9"], 1, G["scale/%d" % k]), (0, 0, 10, img, 0, img)]
    for radius, w2, h2, want_blur, want_ok, want_scaled in cases:
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(src, "wb") as f:
            f.write(b"TRGIMG01" + struct.pack("<6i", 67, 41, 3, radius, w2, h2) + img.tobytes())
        r = subprocess.run([DEMO, "host", str(src), str(dst)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        raw = open(dst, "rb").read()
        assert np.array_equal(np.frombuffer(raw, np.uint8, img.size).reshape(img.shape), want_blur)
        ok, sw, sh = struct.unpack_from("<3i", raw, img.size)
        assert (ok, sh, sw) == (want_ok,) + want_scaled.shape[:2]
        assert np.array_equal(np.frombuffer(raw, np.uint8, sw * sh * 3, img.size + 12).reshape(sh, sw, 3), want_scaled)
