"""The contract of trgl_mesh_weld (include/trgl.h, "mesh welding") restated in plain Python, the yardstick of tests/test_weld.py and
tests/test_weld_gpu.py: a dict from key tuples to the first vertex that had the key, a NaN check, numbers by first occurrence.  No hash
of its own and no sort: it shares no mechanism with the library's host loop (a probed table) or its kernels (a radix sort of hashes)."""
import math

import numpy as np

NONE = 0xFFFFFFFF


def q_value(x, cell):
    """the compared value of a key component: x, or the number of its grid cell - an IEEE division, one rounded sum, an exact floor"""
    x = float(x)
    if cell == 0.0:
        return x
    s = np.float64(x) / np.float64(cell) + np.float64(0.5)     # numpy scalars: fp64, each operation rounded
    return float(np.floor(s))


def key_of(record, key_offset, key_count, cell):
    """The key as a tuple a dict may hold, or None when it holds a NaN.  Python's float == is IEEE's: -0.0 == 0.0, inf == inf; equal
    floats hash alike, so the dict groups exactly the identical keys."""
    key = tuple(q_value(record[key_offset + a], cell) for a in range(key_count))
    return None if any(math.isnan(q) for q in key) else key


def representatives(vertices, key_offset, key_count, cell=0.0):
    """rep[v]: the lowest-numbered vertex identical to v, v itself when there is none"""
    first, rep = {}, []
    for v, record in enumerate(np.asarray(vertices, np.float64)):
        key = key_of(record, key_offset, key_count, cell)
        rep.append(v if key is None else first.setdefault(key, v))
    return rep


def weld(vertices, key_offset, key_count, cell=0.0, indices=None, device=False):
    """(remap [n], firsts [n], vertices_out [n, stride], indices_out [F, 3] or None, n_unique).  device: an index >= n becomes NONE (in
    host memory the library refuses it, and so does this model)."""
    vertices = np.ascontiguousarray(vertices, np.float64)
    n = vertices.shape[0]
    rep = representatives(vertices, key_offset, key_count, cell)
    number, firsts = {}, []
    for v in range(n):
        if rep[v] == v:
            number[v] = len(firsts)
            firsts.append(v)
    remap = np.array([number[rep[v]] for v in range(n)], np.uint32).reshape(n)
    U = len(firsts)
    firsts_out = np.full(n, NONE, np.uint32)
    firsts_out[:U] = firsts
    out = np.zeros_like(vertices)
    out.view(np.uint64)[:U] = vertices.view(np.uint64)[firsts] if U else 0
    indices_out = None
    if indices is not None:
        indices = np.asarray(indices, np.uint32)
        flat = indices.reshape(-1).astype(np.int64)
        bad = flat >= n
        assert device or not bad.any(), "host memory: an index out of range is refused"
        indices_out = np.where(bad, NONE, remap[np.where(bad, 0, flat)] if n else NONE).astype(np.uint32).reshape(indices.shape)
    return remap, firsts_out, out, indices_out, U


def runs_by_low_bits(hashes, bits):
    """vertex numbers grouped by the low `bits` bits of their hashes: the runs the device path walks"""
    mask = (1 << bits) - 1 if bits < 64 else (1 << 64) - 1
    runs = {}
    for v, h in enumerate(hashes):
        runs.setdefault(int(h) & mask, []).append(v)
    return runs
