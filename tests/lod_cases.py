"""Meshes for the level-of-detail tests (tests/test_lod.py, tests/test_lod_gpu.py): a hand-made face list with its classes written out,
seeded face lists at every duplicate and degenerate rate, unreferenced vertices at the front, in the middle and at the end, a closed
sphere, positions with the special values of IEEE ==, and the proof that few hash bits put different triples into one run."""
import numpy as np

import lod_model as M
from tinyrenderder_amd import api, scenes

SENTINEL_U32 = 0xA5A5A5A5
SENTINEL_F64 = np.frombuffer(np.uint64(0xA5A5A5A5A5A5A5A5).tobytes(), np.float64)[0]
NONE = 0xFFFFFFFF


def hand_made():
    """14 faces over 12 vertices.  Returns (indices, n_vertices, the class of every face with TRGL_CLEAN_DUPLICATES, written out).
    Vertices 0, 6 and 11 are named by no kept face: the front, the middle and the end."""
    c, g, d = M.CANDIDATE, M.DEGENERATE, M.DUPLICATE
    rows = [((1, 2, 3), c),        # 0
            ((2, 3, 1), d),        # 1: a rotation of 0
            ((3, 1, 2), d),        # 2: the other rotation
            ((3, 2, 1), c),        # 3: 0 mirrored - the other side of a sheet stays
            ((1, 3, 2), d),        # 4: a rotation of 3
            ((4, 4, 5), g),        # 5: a == b
            ((4, 5, 5), g),        # 6: b == c
            ((5, 4, 5), g),        # 7: c == a
            ((7, 7, 7), g),        # 8: all three
            ((5, 4, 4), g),        # 9: dropped, and so ...
            ((4, 4, 5), g),        # 10: ... this is no duplicate of 5: both are degenerate
            ((8, 9, 10), c),       # 11
            ((1, 2, 3), d),        # 12: face 0 itself again
            ((10, 8, 9), d)]       # 13: a rotation of 11 that starts with the largest index
    return np.array([r for r, _ in rows], np.uint32), 12, [k for _, k in rows]


def records(n, stride, seed):
    """n records of noise: a record copied from the wrong vertex shows"""
    return np.ascontiguousarray(scenes.SplitMix64(seed).uniform(n * stride, -9.0, 9.0).reshape(n, stride))


def seeded_faces(F, V, dup, degen, seed):
    """F faces over V >= 3 vertices: about F * degen of them degenerate (all three shapes), about F * dup of the rest a rotation of an
    earlier face (dup >= 1: every face after the first candidate), the others fresh triples.  Some vertices are named by nobody."""
    rng = scenes.SplitMix64(seed)
    r = rng.u64(6 * F).reshape(F, 6)
    out, candidates = np.zeros((F, 3), np.uint32), []
    for f in range(F):
        a, b, c = (int(x % np.uint64(V)) for x in r[f, :3])
        roll = int(r[f, 3] % np.uint64(1000)) / 1000.0
        if roll < degen:
            shape = int(r[f, 4] % np.uint64(4))
            t = [(a, a, c), (a, c, c), (c, b, c), (a, a, a)][shape]
        elif candidates and (dup >= 1.0 or int(r[f, 4] % np.uint64(1000)) / 1000.0 < dup):
            g = out[candidates[int(r[f, 5] % np.uint64(len(candidates)))]].tolist()
            k = int(r[f, 4] % np.uint64(3))
            t = tuple(g[k:] + g[:k])
        else:
            if b == a:
                b = (a + 1) % V
            while c == a or c == b:
                c = (c + 1) % V
            t = (a, b, c)
            candidates.append(f)
        out[f] = t
    return out


def octa_sphere(level, stride=3, seed=5):
    """A closed sphere: the octahedron subdivided `level` times, every new vertex on the unit sphere, vertices shared - a clean closed
    mesh of 8 * 4^level faces and 4^(level+1) + 2 vertices.  Doubles behind the position are noise.  Returns (vertices, indices)."""
    pos = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(level):
        mid, finer = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.array(pos[key[0]]) + np.array(pos[key[1]])
                pos.append(tuple((p / np.sqrt((p * p).sum())).tolist()))
                mid[key] = len(pos) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            finer += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = finer
    v = records(len(pos), stride, seed)
    v[:, :3] = np.array(pos, np.float64)
    return np.ascontiguousarray(v), np.array(faces, np.uint32)


def special_positions(stride=5):
    """Vertices whose positions hold signed zeros, infinities, NaNs and ordinary values, and faces that name most of them; vertex 9 shares
    vertex 8's cell and is named by nobody.  Returns (vertices, indices)."""
    inf, nan = float("inf"), float("nan")
    pos = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (1.0, 1.0, 1.0), (1.0, 2.0, 1.0), (inf, 1.0, -inf), (inf, 1.0, -inf), (nan, 1.0, 2.0), (nan, 1.0, 2.0),
           (3.0, 3.0, 3.0), (3.0, 3.0, 3.0), (-0.0, -0.0, -0.0), (2.0, 0.5, 0.25), (-inf, 0.0, 0.0), (2.0, 0.5, 0.25)]
    v = records(len(pos), stride, 19)
    v[:, :3] = np.array(pos, np.float64)
    idx = np.array([[0, 2, 3], [1, 2, 3], [10, 3, 2], [4, 2, 3], [5, 2, 3], [6, 2, 3], [7, 2, 3], [8, 11, 12], [8, 13, 12], [2, 3, 11], [6, 7, 2], [1, 0, 2]],
                   np.uint32)
    return np.ascontiguousarray(v), idx


def collision_proof(indices, n_vertices, bits):
    """Through the model: (runs of the low `bits` bits that hold candidates with several distinct canonical triples, duplicates whose
    earlier twin is not the head of their run - found only by walking the run)."""
    indices = np.asarray(indices, np.uint32).reshape(-1, 3)
    hashes = api.lod_face_hashes(indices, n_vertices)
    cls = M.classes(indices, n_vertices)
    mixed = walked = 0
    for run in M.runs_by_low_bits(hashes, bits).values():
        triples = {f: M.canonical(*indices[f].tolist()) for f in run if cls[f] != M.DEGENERATE and cls[f] != M.INVALID}
        mixed += len(set(triples.values())) > 1
        walked += sum(1 for f in run if cls[f] == M.DUPLICATE and (run[0] not in triples or triples[run[0]] != triples[f]))
    return mixed, walked


# (F, V, dup, degen, seed) that tests/test_lod_gpu.py runs with few hash bits
COLLISION_CASES = [(257, 40, 0.5, 0.2, 51), (3000, 900, 0.5, 0.1, 52), (1000, 2000, 0.0, 0.0, 53), (300, 30, 0.8, 0.3, 54)]
