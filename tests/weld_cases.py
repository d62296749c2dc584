"""Vertex arrays for the welding tests (tests/test_weld.py, tests/test_weld_gpu.py): a hand-made case, seeded arrays at every duplicate
rate, the special values of IEEE ==, grid-cell borders, the cube as an OBJ reader delivers it and the head stand-in as a soup."""
import numpy as np

import weld_model as M
from tinyrenderder_amd import api, scenes

SENTINEL_U32 = 0xA5A5A5A5
SENTINEL_F64 = np.frombuffer(np.uint64(0xA5A5A5A5A5A5A5A5).tobytes(), np.float64)[0]
NONE = 0xFFFFFFFF

# (vertex_stride, key_offset, key_count): a position key in front, the whole record, a key in the middle, a single double
LAYOUTS = [(3, 0, 3), (5, 0, 5), (8, 3, 3), (14, 2, 1), (14, 0, 3), (5, 2, 1), (8, 0, 8), (3, 2, 1)]


def seeded(n, stride, key_offset, key_count, dup, seed):
    """n records of noise whose keys repeat at the rate `dup`: 0 - every key distinct; 1 - one key; else about n * (1 - dup) distinct keys
    drawn at random, so that some are never drawn and the first of a key may come late.  The doubles outside the key differ from vertex
    to vertex: a record copied from the wrong vertex shows."""
    rng = scenes.SplitMix64(seed)
    v = rng.uniform(n * stride, -9.0, 9.0).reshape(n, stride)
    pool_n = n if dup == 0 else 1 if dup >= 1 else max(1, int(round(n * (1.0 - dup))))
    pool = rng.uniform(pool_n * key_count, -1.0, 1.0).reshape(pool_n, key_count)
    pool[:, 0] = np.arange(pool_n) + 0.25 * pool[:, 0]                 # distinct for certain
    src = np.arange(n) if dup == 0 else (rng.u64(n) % np.uint64(pool_n)).astype(np.int64)
    v[:, key_offset:key_offset + key_count] = pool[src]
    return np.ascontiguousarray(v)


def hand_made():
    """8 vertices of stride 4, key = doubles 1 and 2.  Returns (vertices, remap, firsts, n_unique) with the expected arrays written out."""
    nan = float("nan")
    v = np.array([[10.0, 1.0, 2.0, 0.5],      # 0: new 0
                  [11.0, 3.0, 4.0, 0.5],      # 1: new 1
                  [12.0, 1.0, 2.0, 0.7],      # 2: = 0
                  [13.0, 0.0, -0.0, 0.5],     # 3: new 2
                  [14.0, -0.0, 0.0, 0.5],     # 4: = 3 (signed zeros are equal)
                  [15.0, nan, 2.0, 0.5],      # 5: new 3 (a NaN joins nothing)
                  [16.0, nan, 2.0, 0.5],      # 6: new 4 (not even its twin)
                  [17.0, 3.0, 4.0, 0.9]],     # 7: = 1
                 np.float64)
    return v, [0, 1, 0, 2, 2, 3, 4, 1], [0, 1, 3, 5, 6, NONE, NONE, NONE], 5


def special_values(stride=5, key_offset=1, key_count=3):
    """signed zeros, infinities of both signs, NaNs with different payloads, bit-identical NaN vertices, denormals, values one ulp apart"""
    nan2 = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), np.float64)[0]
    inf, nan, tiny = float("inf"), float("nan"), 5e-324
    one_up = np.nextafter(1.0, 2.0)
    keys = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, 0.0), (inf, 1.0, -inf), (inf, 1.0, -inf), (-inf, 1.0, -inf), (inf, 1.0, inf),
            (nan, 1.0, 2.0), (nan, 1.0, 2.0), (1.0, nan2, 2.0), (1.0, 1.0, 2.0), (1.0, 1.0, nan), (tiny, 0.0, 0.0), (-tiny, 0.0, 0.0), (tiny, 0.0, 0.0),
            (1.0, 1.0, 2.0), (one_up, 1.0, 2.0), (1.0, one_up, 2.0), (one_up, 1.0, 2.0), (-0.0, -0.0, -0.0), (nan, nan, nan), (nan, nan, nan)]
    rng = scenes.SplitMix64(77)
    v = rng.uniform(len(keys) * stride, -9.0, 9.0).reshape(-1, stride)
    v[:, key_offset:key_offset + key_count] = np.array(keys, np.float64)[:, :key_count]
    return np.ascontiguousarray(v), key_offset, key_count


CELL = 0.25


def cell_values():
    """One key double per vertex around the borders of the grid of CELL = 0.25 (cells are centred on multiples of 0.25: borders at odd
    multiples of 0.125), negative values, x / cell == -0.5 exactly, values whose quotient is huge or overflows, zeros and non-finite values.  (The
    double just below 0.125 lands in cell 1: 4 x + 0.5 rounds up to 1.0 - the sum is rounded once, as the contract says.)
    Returns (vertices [n, 2] - the key is double 1 -, the q the contract gives each, written out)."""
    up, down = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    inf, nan = float("inf"), float("nan")
    rows = [(0.0, 0.0), (-0.0, 0.0), (0.1, 0.0), (down(0.125), 1.0), (0.125, 1.0), (up(0.125), 1.0), (0.25, 1.0), (0.3, 1.0), (down(0.375), 1.0), (0.375, 2.0),
            (-0.1, -0.0), (-0.125, 0.0), (down(-0.125), -1.0), (-0.25, -1.0), (up(-0.375), -1.0), (-0.375, -1.0), (down(-0.375), -2.0),
            (1e308, inf), (-1e308, -inf), (1e300, 4e300), (2.0 ** 60, 2.0 ** 62), (2.0 ** 60 + 256.0, 2.0 ** 62 + 1024.0), (-(2.0 ** 60), -(2.0 ** 62)),
            (1e15 + 0.125, 4e15 + 1.0), (inf, inf), (-inf, -inf), (nan, nan), (0.12, 0.0), (-0.3, -1.0)]
    v = np.array([[float(i), x] for i, (x, _) in enumerate(rows)], np.float64)
    return v, [q for _, q in rows]


def split_cube():
    """The cube of 8 corners as an OBJ reader delivers it: one vertex per (position, face normal) pair - 24 records of 6 doubles, position
    at +0 and normal at +3 - and 12 faces.  Returns (vertices, indices)."""
    corner = lambda c: [2.0 * (c & 1) - 1, 2.0 * ((c >> 1) & 1) - 1, 2.0 * ((c >> 2) & 1) - 1]
    quads = [((0, 2, 3, 1), (0, 0, -1)), ((4, 5, 7, 6), (0, 0, 1)), ((0, 1, 5, 4), (0, -1, 0)), ((2, 6, 7, 3), (0, 1, 0)), ((0, 4, 6, 2), (-1, 0, 0)),
             ((1, 3, 7, 5), (1, 0, 0))]
    v, idx = [], []
    for q, n in quads:
        base = len(v)
        v += [corner(c) + [float(x) for x in n] for c in q]
        idx += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.array(v, np.float64), np.array(idx, np.uint32)


def head_soup(level=2, w=64, h=64):
    """The head stand-in unwelded: three 14-double records per face (position, normal, uv, six doubles of noise) and indices 0 .. 3 F - 1.
    Returns (the scene dict, vertices, indices)."""
    hd = scenes.head_standin(level, w, h)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    rng = scenes.SplitMix64(23)
    verts = np.ascontiguousarray(np.concatenate([pos, nrm, uv, rng.uniform(pos.shape[0] * 6, -1.0, 1.0).reshape(-1, 6)], 1))
    return hd, verts, np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)


# (n, stride, key_offset, key_count, dup, seed) that tests/test_weld_gpu.py runs with few hash bits
COLLISION_CASES = [(257, 5, 1, 3, 0.5, 31), (4096, 3, 0, 3, 0.5, 32), (1000, 8, 3, 3, 0.0, 33), (300, 14, 2, 1, 0.83, 34)]


def collision_proof(v, ko, kc, bits, cell=0.0):
    """Through the model: (runs of the low `bits` hash bits that hold several distinct keys, vertices whose representative is neither
    themselves nor the head of their run - found only by walking the run)."""
    hashes = api.weld_hashes(api.make_weld_params(v.shape[1], ko, kc, cell), v)
    rep = M.representatives(v, ko, kc, cell)
    mixed, walked = 0, 0
    for run in M.runs_by_low_bits(hashes, bits).values():
        mixed += len({rep[u] for u in run}) > 1
        walked += sum(1 for u in run if rep[u] != u and rep[u] != run[0])
    return mixed, walked
