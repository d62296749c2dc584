"""A numpy model of trgl_instance_depths, trgl_depth_order and the ordered instanced calls, written from include/trgl.h alone.

depths: element 2 of (model_view * M_i) * (point, 1) - row 2 of the matrix product summed from 0.0 with k ascending, then dot<4> summed
from 0.0, one rounding per product and per sum.  order: the unsigned key of a double's bits (sign set: all bits flipped, clear: sign bit
set), complemented for front to back, argsorted stably.  visit: the instances an ordered call draws, in the order it draws them."""
import numpy as np

BACK_TO_FRONT, FRONT_TO_BACK = 0, 1


def depths(model_view, point, instances):
    """[n] float64; instances [n, stride >= 16]."""
    mv = np.asarray(model_view, np.float64).reshape(4, 4)
    p = np.asarray(point, np.float64).reshape(3)
    m = np.asarray(instances, np.float64)[:, :16].reshape(-1, 4, 4)
    with np.errstate(all="ignore"):
        r = []
        for c in range(4):
            s = np.zeros(m.shape[0], np.float64)
            for k in range(4):
                s = s + mv[2, k] * m[:, k, c]
            r.append(s)
        d = np.zeros(m.shape[0], np.float64)
        for c, x in enumerate((p[0], p[1], p[2], np.float64(1.0))):
            d = d + r[c] * x
    return d


def keys(d, direction=BACK_TO_FRONT):
    """[n] uint64: what the order sorts."""
    b = np.ascontiguousarray(d, np.float64).view(np.uint64)
    k = b ^ np.where(b >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63))
    return ~k if direction == FRONT_TO_BACK else k


def order(d, direction=BACK_TO_FRONT):
    """[n] uint32: the permutation that sorts the keys, ties in ascending number."""
    return np.argsort(keys(d, direction), kind="stable").astype(np.uint32)


def visit(order_list, n_instances, visible=None, skip_out_of_range=False):
    """The original numbers of the instances an ordered call draws, in its order.  An entry >= n_instances: skipped (a device list), or
    an error (a host list)."""
    o = np.asarray(order_list, np.uint32).astype(np.int64)
    bad = o >= n_instances
    if bad.any():
        assert skip_out_of_range, "a host list with an entry out of range is TRGL_E_INVALID"
        o = o[~bad]
    if visible is not None:
        o = o[(np.asarray(visible, np.uint8)[o] & 1) != 0]
    return o
