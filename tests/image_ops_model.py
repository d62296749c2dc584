"""TGAImage::gaussian_blur and TGAImage::scale (tgaimage.cpp:246-324) restated in numpy, for images [h, w, bpp] uint8.

Every float32 operation is its own numpy call, so each rounds separately (no fused multiply-add), and the taps are added in the
reference's order k = -radius..radius from 0.0f; the arrays only run the independent pixels side by side.  The weights are an argument:
tests pass the golden's or trgl_gaussian_kernel's (the same bits), so the model never depends on numpy's exp.
tests/golden/make_image_ops_golden.py asserts this model equal to the reference's compiled code on every golden case."""
import numpy as np


def _pass(img, weights, axis):
    n = img.shape[axis]
    radius = (len(weights) - 1) // 2
    src = img.astype(np.int32).astype(np.float32)              # uint8 -> int -> float (tgaimage.cpp:298)
    acc = np.zeros(img.shape, np.float32)
    pos = np.arange(n)
    for k in range(-radius, radius + 1):
        taps = np.take(src, np.clip(pos + k, 0, n - 1), axis=axis)                        # :294 / :313
        acc = np.add(acc, np.multiply(taps, np.float32(weights[k + radius]), dtype=np.float32), dtype=np.float32)
    return acc.astype(np.int32).astype(np.uint8)               # (uint8_t)accum: a truncation; the golden's maker shows it never exceeds 255


def gaussian_blur(img, weights):
    """img [h, w, bpp] uint8, weights the 2 * radius + 1 float32 of the radius (None or empty: radius <= 0, the image comes back as it is)."""
    img = np.ascontiguousarray(img, np.uint8)
    if weights is None or len(weights) == 0 or img.size == 0:
        return img.copy()
    weights = np.asarray(weights, np.float32)
    return _pass(_pass(img, weights, 1), weights, 0)           # horizontal, then vertical over the horizontal pass's bytes (:306)


def scale(img, w2, h2):
    """img [h, w, bpp] -> [h2, w2, bpp], or None where the reference returns false (:247)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    if w2 <= 0 or h2 <= 0 or img.size == 0:
        return None
    sx = np.arange(w2, dtype=np.int64) * w // w2               # :253 (non-negative: // is C's /)
    sy = np.arange(h2, dtype=np.int64) * h // h2               # :254
    return np.ascontiguousarray(img[sy][:, sx])
