"""The contracts of trgl_mesh_clean and trgl_mesh_simplify (include/trgl.h, "mesh levels of detail") restated in plain Python, the
yardstick of tests/test_lod.py and tests/test_lod_gpu.py: a class per face, canonical triples as tuples, first occurrences through a dict,
numbers by ascending old number, the mean as an explicit left-to-right loop in np.float64.  The weld of a simplification is
tests/weld_model.py's.  No hash and no sort: it shares no mechanism with the library's host loops or its kernels."""
import numpy as np

import weld_model

NONE = 0xFFFFFFFF
DUPLICATES, VERTICES = 1, 2
FILL_NONE, FILL_ZERO = 0, 1
CANDIDATE, INVALID, DEGENERATE, DUPLICATE = "candidate", "invalid", "degenerate", "duplicate"


def canonical(a, b, c):
    """the rotation that puts the smallest index first, orientation kept"""
    rotations = [(a, b, c), (b, c, a), (c, a, b)]
    return min(rotations, key=lambda t: t[0])


def classes(indices, n_vertices, duplicates=True):
    """the class of every face: INVALID, DEGENERATE, DUPLICATE (of an earlier face that is neither invalid nor degenerate) or CANDIDATE -
    the kept ones"""
    seen, out = {}, []
    for f, (a, b, c) in enumerate(np.asarray(indices, np.uint32).reshape(-1, 3).tolist()):
        if a >= n_vertices or b >= n_vertices or c >= n_vertices:
            out.append(INVALID)
        elif a == b or b == c or c == a:
            out.append(DEGENERATE)
        elif duplicates and seen.setdefault(canonical(a, b, c), f) != f:
            out.append(DUPLICATE)
        else:
            out.append(CANDIDATE)
    return out


def clean(indices, n_vertices, flags=DUPLICATES | VERTICES, fill=FILL_NONE, vertices=None, device=False):
    """dict(indices [F, 3], face_firsts [F], vremap [V], vfirsts [V], vertices [V, S] - None where the call writes nothing -, counts).
    device: an invalid face is dropped (in host memory the library refuses it, and so does this model)."""
    indices = np.asarray(indices, np.uint32).reshape(-1, 3)
    F, V = indices.shape[0], int(n_vertices)
    cls = classes(indices, V, bool(flags & DUPLICATES))
    assert device or INVALID not in cls, "host memory: an index out of range is refused"
    kept = [f for f in range(F) if cls[f] == CANDIDATE]
    K = len(kept)
    fill_word = 0 if fill == FILL_ZERO else NONE
    res = dict(vremap=None, vfirsts=None, vertices=None)
    number = {}
    U = V
    if flags & VERTICES:
        named = set(int(i) for f in kept for i in indices[f])
        firsts = sorted(named)
        number = {v: j for j, v in enumerate(firsts)}
        U = len(firsts)
        res["vremap"] = np.array([number.get(v, NONE) for v in range(V)], np.uint32).reshape(V)
        res["vfirsts"] = np.full(V, NONE, np.uint32)
        res["vfirsts"][:U] = firsts
        if vertices is not None:
            vertices = np.ascontiguousarray(vertices, np.float64)
            res["vertices"] = np.zeros_like(vertices)
            if U:
                res["vertices"].view(np.uint64)[:U] = vertices.view(np.uint64)[firsts]
    out = np.full((F, 3), fill_word, np.uint32)
    for j, f in enumerate(kept):
        out[j] = [number[int(i)] for i in indices[f]] if flags & VERTICES else indices[f]
    face_firsts = np.full(F, NONE, np.uint32)
    face_firsts[:K] = kept
    res.update(indices=out, face_firsts=face_firsts, counts=(K, U))
    check_clean_properties(res, bool(flags & DUPLICATES), bool(flags & VERTICES))
    return res


def check_clean_properties(res, duplicates, with_vertices):
    """What every result of a clean satisfies - the model's own, and the library's: kept faces have three distinct indices below the vertex
    count, no two share a canonical triple, every new vertex is named, the first occurrences ascend."""
    K, U = res["counts"]
    faces = np.asarray(res["indices"]).reshape(-1, 3)[:K].astype(np.int64)
    assert ((faces >= 0) & (faces < U)).all(), "a kept face names no vertex"
    assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])).all(), "a kept face is degenerate"
    if duplicates:
        assert len({canonical(*f) for f in faces.tolist()}) == K, "two kept faces share a canonical triple"
    assert (np.diff(np.asarray(res["face_firsts"])[:K].astype(np.int64)) > 0).all(), "face_firsts do not ascend"
    if with_vertices:
        assert set(faces.reshape(-1).tolist()) == set(range(U)), "a new vertex that no kept face names"
        assert (np.diff(np.asarray(res["vfirsts"])[:U].astype(np.int64)) > 0).all(), "vfirsts do not ascend"


def cell_means(vertices, indices, remap, n_clusters, records, mean_count):
    """(b) of trgl_mesh_simplify over the weld's records (changed in place): the first mean_count doubles of record j become the mean of
    the referenced members of cluster j, summed in ascending old number, one rounded sum at a time, one IEEE division"""
    n = vertices.shape[0]
    referenced = np.zeros(n, bool)
    flat = np.asarray(indices, np.uint32).reshape(-1)
    referenced[flat[flat < n]] = True
    members = [[] for _ in range(n_clusters)]
    for v in range(n):                                       # ascending old number
        if referenced[v]:
            members[int(remap[v])].append(v)
    for j, m in enumerate(members):
        if len(m) == 1:
            records.view(np.uint64)[j, :mean_count] = vertices.view(np.uint64)[m[0], :mean_count]
        elif len(m) > 1:
            for a in range(mean_count):
                s = np.float64(vertices[m[0], a])
                for v in m[1:]:
                    s = np.float64(s + np.float64(vertices[v, a]))
                records[j, a] = np.float64(s / np.float64(len(m)))


def simplify(vertices, indices, cell, mean_count=3, fill=FILL_NONE, device=False):
    """dict(remap [n], firsts [n], vertices [n, S], indices [F, 3], face_firsts [F], counts): the composition the header writes down"""
    vertices = np.ascontiguousarray(vertices, np.float64)
    indices = np.asarray(indices, np.uint32).reshape(-1, 3)
    n = vertices.shape[0]
    with np.errstate(all="ignore"):
        remap, firsts, records, welded, U = weld_model.weld(vertices, 0, 3, cell, indices, device=device)
        if mean_count:
            cell_means(vertices, indices, remap, U, records, mean_count)
    c = clean(welded, n, DUPLICATES | VERTICES, fill, records, device=device)
    K, Vk = c["counts"]
    out_remap = c["vremap"][remap] if n else np.zeros(0, np.uint32)
    out_firsts = np.full(n, NONE, np.uint32)
    out_firsts[:Vk] = firsts[c["vfirsts"][:Vk]]
    assert (np.diff(out_firsts[:Vk].astype(np.int64)) > 0).all(), "firsts do not ascend"
    return dict(remap=out_remap.astype(np.uint32), firsts=out_firsts, vertices=c["vertices"], indices=c["indices"], face_firsts=c["face_firsts"],
                counts=c["counts"])


def runs_by_low_bits(hashes, bits):
    """face numbers grouped by the low `bits` bits of what the device path sorts them by: the runs it walks"""
    return weld_model.runs_by_low_bits(hashes, bits)
