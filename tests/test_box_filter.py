"""The host path of trgl_image_downsample (the exact integer box filter of include/trgl.h, "box-filter resolve and frames as textures")
against tests/box_model.py, byte for byte: every bpp and factor, sizes with and without a remainder, the largest sum, exact ties and
their neighbours, the remainder columns and rows, the error cases.  Needs no GPU."""
import numpy as np
import pytest

import box_model
from tinyrenderder_amd import api

BPPS = (1, 3, 4)
FACTORS = (1, 2, 3, 4, 7, 16)
E_INVALID, E_UNSUPPORTED = -1, -5
MEM_HOST, MEM_DEVICE = 0, 1


def sizes(f):
    """(w, h): multiples of f, remainders in w, in h and in both, one block in either direction, one output column, one output row."""
    return [(5 * f, 3 * f), (5 * f + f - 1, 3 * f), (4 * f, 2 * f + f - 1 + (f == 1)), (6 * f + 1, 4 * f + f - 1),
            (f, 3 * f + 1), (5 * f, f), (f, f), (2 * f - 1 + (f == 1), 37), (41, 2 * f - 1 + (f == 1))]


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("bpp", BPPS)
def test_random_images_equal_the_model(bpp, f):
    rng = np.random.default_rng(1000 * bpp + f)
    for w, h in sizes(f):
        img = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
        got, want = api.image_downsample(img, f), box_model.box_filter(img, f)
        assert got.shape == (h // f, w // f, bpp) and np.array_equal(got, want), (w, h, bpp, f, np.argwhere(got != want)[:5])


def test_the_sizes_cover_what_they_claim():
    for f in FACTORS:
        s = sizes(f)
        assert any(w % f == 0 and h % f == 0 for w, h in s) and any(w == f for w, h in s) and any(h == f for w, h in s)
        assert any(w // f == 1 for w, h in s) and any(h // f == 1 for w, h in s)
        if f > 1:
            assert any(w % f and h % f for w, h in s) and any(w % f and not h % f for w, h in s) and any(h % f and not w % f for w, h in s)


@pytest.mark.parametrize("bpp", BPPS)
def test_factor_one_is_the_input(bpp):
    img = np.random.default_rng(bpp).integers(0, 256, (23, 31, bpp), dtype=np.uint8)
    assert np.array_equal(api.image_downsample(img, 1), img)


@pytest.mark.parametrize("bpp", BPPS)
def test_all_255_at_factor_16_is_the_largest_sum(bpp):
    img = np.full((35, 50, bpp), 255, np.uint8)
    got = api.image_downsample(img, 16)
    assert got.shape == (2, 3, bpp) and (got == 255).all()
    img[5, 7, bpp - 1] = 254                                 # 65279 + 128 still rounds to 255 ...
    assert (api.image_downsample(img, 16) == 255).all()
    img[0:8, 0:16, 0] = 254                                  # ... 65280 - 128 is the tie and rounds up, one less does not
    assert api.image_downsample(img, 16)[0, 0, 0] == 255
    img[8, 0, 0] = 254
    want = box_model.box_filter(img, 16)
    assert want[0, 0, 0] == 254 and np.array_equal(api.image_downsample(img, 16), want)


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("bpp", BPPS)
def test_ties_and_their_neighbours(bpp, f):
    """Every output of the first image sits one below the rounding threshold, of the second on it (for an even f that is an exact tie:
    it rounds up), of the third one above."""
    rng = np.random.default_rng(77 * bpp + f)
    shape = (5, 9, bpp)
    n = f * f
    for offset in (-1, 0, 1):
        sums = box_model.tie_sums(shape, f, rng, offset) if f > 1 else rng.integers(0, 256, shape)
        img = box_model.image_with_sums(sums, f, rng)
        assert np.array_equal(img.astype(np.int64).reshape(5, f, 9, f, bpp).sum(axis=(1, 3)), sums)
        want = (sums + n // 2) // n
        if f % 2 == 0:
            assert np.array_equal(want, sums // n + (offset >= 0))        # even f: exactly half rounds up, one less rounds down
        got = api.image_downsample(img, f)
        assert np.array_equal(got, want) and np.array_equal(got, box_model.box_filter(img, f)), (bpp, f, offset)


@pytest.mark.parametrize("f", [2, 3, 7, 16])
@pytest.mark.parametrize("bpp", BPPS)
def test_remainder_columns_and_rows_have_no_influence(bpp, f):
    rng = np.random.default_rng(5 * bpp + f)
    w, h = 4 * f + f - 1, 3 * f + f - 1
    img = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    a = api.image_downsample(img, f)
    scribbled = img.copy()
    scribbled[:, 4 * f:] = rng.integers(0, 256, (h, f - 1, bpp), dtype=np.uint8)
    scribbled[3 * f:, :] = rng.integers(0, 256, (f - 1, w, bpp), dtype=np.uint8)
    assert not np.array_equal(scribbled, img)
    assert np.array_equal(api.image_downsample(scribbled, f), a)
    assert np.array_equal(a, api.image_downsample(np.ascontiguousarray(img[:3 * f, :4 * f]), f))


def call(src, w, h, bpp, f, dst, mem_kind=MEM_HOST, ctx=None):
    L = api.load_library()
    sp = src.ctypes.data if isinstance(src, np.ndarray) else src
    dp = dst.ctypes.data if isinstance(dst, np.ndarray) else dst
    return L.trgl_image_downsample(ctx, sp, w, h, bpp, f, dp, mem_kind)


def test_error_cases():
    src = np.zeros((40, 48, 3), np.uint8)
    dst = np.full((40, 48, 3), 9, np.uint8)
    assert call(src, 48, 40, 3, 2, dst) == 0
    for f in (0, -1, 17, 1 << 20):                                             # factor outside 1..16
        assert call(src, 48, 40, 3, f, dst) == E_INVALID
    assert b"factor" in api.load_library().trgl_last_error(None)
    assert call(src, 15, 40, 3, 16, dst) == E_INVALID                          # w2 == 0
    assert call(src, 48, 6, 3, 7, dst) == E_INVALID                            # h2 == 0
    assert call(src, 0, 40, 3, 1, dst) == E_INVALID and call(src, 48, -4, 3, 2, dst) == E_INVALID
    for bpp in (0, 2, 5, -3):
        assert call(src, 48, 40, bpp, 2, dst) == E_INVALID
    assert call(None, 48, 40, 3, 2, dst) == E_INVALID and call(src, 48, 40, 3, 2, None) == E_INVALID
    for mk in (-1, 2, 7):
        assert call(src, 48, 40, 3, 2, dst, mem_kind=mk) == E_INVALID
    assert call(src, 48, 40, 3, 2, dst, mem_kind=MEM_DEVICE, ctx=None) == E_INVALID       # device memory without a context
    # overlap: dst inside src, dst == src, dst ending one byte into src; touching ranges are fine
    flat = np.zeros(48 * 40 * 3 + 24 * 20 * 3, np.uint8)
    base = flat.ctypes.data
    n2 = 24 * 20 * 3
    assert call(base, 48, 40, 3, 2, base) == E_INVALID
    assert call(base, 48, 40, 3, 2, base + 100) == E_INVALID
    assert call(base + n2 - 1, 48, 40, 3, 2, base) == E_INVALID
    assert b"overlap" in api.load_library().trgl_last_error(None)
    assert call(base + n2, 48, 40, 3, 2, base) == 0
    assert call(base, 48, 40, 3, 2, base + 48 * 40 * 3) == 0
    # w * h * bpp above INT_MAX: refused before a byte is read
    assert call(src, 65535, 65535, 1, 2, dst) == E_UNSUPPORTED
    assert call(src, 30000, 30000, 3, 16, dst) == E_UNSUPPORTED
    assert (dst[20:] == 9).all()                                               # no refused call wrote


def test_python_wrappers_refuse_what_the_library_refuses():
    img = np.zeros((8, 8, 3), np.uint8)
    for f in (0, 17, 9):
        with pytest.raises(api.TrglError, match=r"\(-1\)"):
            api.image_downsample(img, f)
    with pytest.raises(ValueError):
        api.image_downsample(np.zeros((8, 8), np.uint8), 2)
