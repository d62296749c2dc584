"""A numpy model of trgl_triangle_depths and trgl_order_stage, written from include/trgl.h alone.

depths: a fold over the clip w of a group's 3 g vertices in memory order - a sum started from 0.0 (CENTROID), a running minimum
(NEAREST) or maximum (FARTHEST) that a later value replaces only when a strict < says so - then bit 63 flipped as an integer.  Which
NaN an addition returns is decided here in integers, as the header writes it down, not by this machine's adder.
gather: output group p = input group order[p]; an entry that names no group gives all-zero rows (a device list) or is an error (a
host list)."""
import numpy as np

CENTROID, NEAREST, FARTHEST = 0, 1, 2
MODES = (CENTROID, NEAREST, FARTHEST)
_QUIET = np.uint64(1) << np.uint64(51)
_SIGN = np.uint64(1) << np.uint64(63)
_INDEFINITE = np.uint64(0xFFF8000000000000)


def _add(acc, w):
    """acc + w; a NaN result: acc quieted when acc is a NaN, else w quieted when w is one, else 0xFFF8000000000000."""
    with np.errstate(all="ignore"):
        r = acc + w
    rb = r.view(np.uint64).copy()
    bad = np.isnan(r)
    a_nan, w_nan = np.isnan(acc), np.isnan(w)
    rb[bad] = _INDEFINITE
    m = bad & w_nan
    rb[m] = w.view(np.uint64)[m] | _QUIET
    m = bad & a_nan
    rb[m] = acc.view(np.uint64)[m] | _QUIET
    return rb.view(np.float64)


def depths(clip, group=1, mode=CENTROID):
    """[n / group] float64 from clip [n, 12]."""
    clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
    assert group >= 1 and clip.shape[0] % group == 0
    w = np.ascontiguousarray(clip.reshape(-1, 4)[:, 3].reshape(-1, 3 * group))          # [G, 3 g], memory order
    G = w.shape[0]
    if mode == CENTROID:
        acc = _add(np.zeros(G, np.float64), np.ascontiguousarray(w[:, 0]))
    else:
        acc = w[:, 0].copy()
    for v in range(1, 3 * group):
        wv = np.ascontiguousarray(w[:, v])
        if mode == CENTROID:
            acc = _add(acc, wv)
        else:
            with np.errstate(invalid="ignore"):
                take = (wv < acc) if mode == NEAREST else (acc < wv)                   # false for every NaN; -0.0 < +0.0 is false
            acc = np.where(take, wv, acc)
    return (np.ascontiguousarray(acc).view(np.uint64) ^ _SIGN).view(np.float64)


def gather(clip, vary, colors, order, group=1, zero_out_of_range=False):
    """(clip_out, vary_out, colors_out) with len(order) * group rows; vary / colors None stay None."""
    clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
    n = clip.shape[0]
    assert group >= 1 and n % group == 0
    G = n // group
    o = np.asarray(order, np.uint32).astype(np.int64)
    bad = o >= G
    assert zero_out_of_range or not bad.any(), "a host list with an entry out of range is TRGL_E_INVALID"
    rows = (np.where(bad, 0, o)[:, None] * group + np.arange(group)[None, :]).reshape(-1)
    bad_rows = np.repeat(bad, group)

    def take(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if n == 0:
            return np.zeros((rows.size,) + a.shape[1:], a.dtype)
        out = a[rows].copy()
        out[bad_rows] = 0
        return out
    return take(clip), take(vary), take(colors)
