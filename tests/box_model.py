"""The box filter of include/trgl.h (trgl_image_downsample) in plain numpy: the yardstick of test_box_filter.py and test_resolve_gpu.py.

    w2 = w // f, h2 = h // f
    dst(x, y, c) = (sum over j < f, i < f of src(x * f + i, y * f + j, c) + (f * f) // 2) // (f * f)

Exact integer arithmetic, so every comparison against it is byte for byte.  Nothing here is shared with the library's code.
"""
import numpy as np

MAX_FACTOR = 16


def box_filter(img, f):
    """img [h, w, bpp] uint8 -> [h // f, w // f, bpp] uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and 1 <= f <= MAX_FACTOR
    h, w, bpp = img.shape
    h2, w2 = h // f, w // f
    assert h2 >= 1 and w2 >= 1
    blocks = img[:h2 * f, :w2 * f].astype(np.uint64).reshape(h2, f, w2, f, bpp)
    sums = blocks.sum(axis=(1, 3))
    return ((sums + (f * f) // 2) // (f * f)).astype(np.uint8)


def image_with_sums(sums, f, rng):
    """An image [h2 * f, w2 * f, bpp] whose f x f blocks add up to `sums` [h2, w2, bpp] (each 0 .. 255 * f * f), the bytes of a block
    spread at random: fill every byte with sum // (f * f), then add 1 to (sum % (f * f)) randomly chosen bytes of the block."""
    sums = np.asarray(sums, np.int64)
    h2, w2, bpp = sums.shape
    n = f * f
    assert sums.min() >= 0 and sums.max() <= 255 * n
    base, extra = sums // n, sums % n
    order = rng.permuted(np.tile(np.arange(n), (h2, w2, bpp, 1)), axis=-1)        # a random rank for each byte of each block
    blocks = base[..., None] + (order < extra[..., None])                          # [h2, w2, bpp, f * f]
    img = blocks.reshape(h2, w2, bpp, f, f).transpose(0, 3, 1, 4, 2).reshape(h2 * f, w2 * f, bpp)
    return img.astype(np.uint8)


def tie_sums(shape, f, rng, offset=0):
    """Block sums q * f * f + (f * f) // 2 + offset with q random in 0..254: offset 0 is the exact tie of an even f (the result is q + 1),
    -1 is one below it (q), +1 one above (q + 1)."""
    q = rng.integers(0, 255, shape)
    return q * (f * f) + (f * f) // 2 + offset
