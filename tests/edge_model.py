"""A numpy restatement of trgl_mesh_edges and trgl_edge_select (include/trgl.h, "mesh edges"): np.lexsort over (lo, hi, half-edge) for
the edges, plain Python floats - IEEE doubles, one rounding per operation - for the arithmetic.  It shares no code with the library;
the tests hold the host twin and the kernels to it bit for bit."""
import math

import numpy as np

NONE = 0xFFFFFFFF
ANY, BOUNDARY, SILHOUETTE, CREASE = 1, 2, 4, 8


class OutOfRange(Exception):
    """what the host path answers with TRGL_E_INVALID"""


def edges(indices, n_vertices, device=False):
    """(records [3 F, 4] uint32, number of edges).  device: an index >= n_vertices makes no edge; else it raises OutOfRange."""
    idx = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.uint64)
    F = idx.shape[0]
    a, b = idx.reshape(-1), idx[:, [1, 2, 0]].reshape(-1)
    inside = (a < n_vertices) & (b < n_vertices)
    if not device and not inside.all():
        raise OutOfRange
    ok = inside & (a != b)
    lo, hi, h = np.minimum(a, b)[ok], np.maximum(a, b)[ok], np.arange(3 * F, dtype=np.uint64)[ok]
    order = np.lexsort((h, hi, lo))
    lo, hi, h = lo[order], hi[order], h[order]
    rec = np.full((3 * F, 4), NONE, np.uint32)
    if lo.size == 0:
        return rec, 0
    head = np.ones(lo.size, bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    first = np.flatnonzero(head)
    E = first.size
    second = np.minimum(first + 1, lo.size - 1)
    has_second = (first + 1 < lo.size) & ~head[second]
    rec[:E, 0], rec[:E, 1], rec[:E, 2] = lo[first], hi[first], h[first] // 3
    rec[:E, 3] = np.where(has_second, h[second] // 3, NONE)
    return rec, E


def face(vertices, tri, eye):
    """(front, unit normal) of the face with the vertex numbers tri under eye (x, y, z, w)"""
    p0, p1, p2 = ([float(x) for x in vertices[int(i), :3]] for i in tri)
    e1 = [p1[a] - p0[a] for a in range(3)]
    e2 = [p2[a] - p0[a] for a in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    d = [eye[a] - eye[3] * p0[a] for a in range(3)]
    s = 0.0
    for a in range(3):
        s = s + n[a] * d[a]
    ss = 0.0
    for a in range(3):
        ss = ss + n[a] * n[a]
    length = math.sqrt(ss)
    u = n if length == 0.0 else [x / length for x in n]
    return s > 0.0, u


def select(records, vertices, indices, eye, crease_cos, select_mask, class_color=(0, 0, 0, 0), compact=False, device=False):
    """(codes [n] uint8, segments [n, 2] uint32, colors [n] uint32, n_selected) over the n given records.  device: a record out of range
    gets code 0; else it raises OutOfRange."""
    rec = np.asarray(records, np.uint32).reshape(-1, 4)
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    vertices = np.asarray(vertices, np.float64)
    eye = [float(x) for x in eye]
    crease_cos = float(crease_cos)
    n, F, nv = rec.shape[0], idx.shape[0], vertices.shape[0]
    cache = {}

    def get(f):
        if f not in cache:
            cache[f] = None if f >= F or (idx[f] >= nv).any() else face(vertices, idx[f], eye)
        return cache[f]

    codes = np.zeros(n, np.uint8)
    for i in range(n):
        f0, f1 = int(rec[i, 2]), int(rec[i, 3])
        if f0 == NONE:
            continue
        A, B = get(f0), (get(f1) if f1 != NONE else None)
        if A is None or (f1 != NONE and B is None):
            if device:
                continue
            raise OutOfRange
        code = ANY
        if f1 == NONE:
            code |= BOUNDARY
        else:
            if A[0] != B[0]:
                code |= SILHOUETTE
            dot = 0.0
            for a in range(3):
                dot = dot + A[1][a] * B[1][a]
            if dot < crease_cos:
                code |= CREASE
        codes[i] = code
    sel = codes & np.uint8(select_mask)
    chosen = sel != 0
    lowest = np.where(sel & 1, 0, np.where(sel & 2, 1, np.where(sel & 4, 2, 3)))
    segments = np.where(chosen[:, None], rec[:, :2], np.uint32(NONE)).astype(np.uint32)
    colors = np.where(chosen, np.asarray(class_color, np.uint32)[lowest], 0).astype(np.uint32)
    if compact:
        k = int(chosen.sum())
        segments = np.concatenate([segments[chosen], np.full((n - k, 2), NONE, np.uint32)])
        colors = np.concatenate([colors[chosen], np.zeros(n - k, np.uint32)])
    return codes, segments, colors, int(chosen.sum())
