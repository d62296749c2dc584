"""A numpy and plain-Python restatement of trgl_subdiv_topology and trgl_subdiv_vertices (include/trgl.h, "mesh subdivision"): numpy
for the table, Python floats - IEEE doubles, one rounding per operation - for the arithmetic.  The edge records come from
tests/edge_model.py.  It shares no code with the library; the tests hold the host twin and the kernels to it bit for bit."""
import numpy as np

from edge_model import NONE, OutOfRange

LINEAR, LOOP = 0, 1
CANONICAL_NAN = 0x7FF8000000000000


def stencil_words(n_vertices, n_edges):
    return 6 * n_edges + 4 * n_vertices


def _opposite(idx, f, lo, hi, nv):
    """(corner of face f opposite (lo, hi), whether f holds the pair and names vertices only); f is clipped by the caller's mask"""
    F = idx.shape[0]
    face = idx[np.minimum(f, max(F - 1, 0))]
    corner = np.full(f.shape, NONE, np.uint64)
    found = np.zeros(f.shape, bool)
    for k in (2, 1, 0):                                                  # the lowest k wins: assigned last
        a, b = face[:, k], face[:, (k + 1) % 3]
        hit = ((a == lo) & (b == hi)) | ((a == hi) & (b == lo))
        corner = np.where(hit, face[:, (k + 2) % 3], corner)
        found |= hit
    return corner, found & (face < nv).all(axis=1)


def _find(keys, want):
    """the header's halving, for every entry of `want` at once: the first record whose key is not below it, or len(keys)"""
    first = np.zeros(want.shape, np.int64)
    last = np.full(want.shape, keys.size, np.int64)
    while True:
        live = first < last
        if not live.any():
            return first
        mid = (first + last) // 2
        below = live & (keys[np.minimum(mid, keys.size - 1)] < want)
        first = np.where(below, mid + 1, first)
        last = np.where(live & ~below, mid, last)


def topology(indices, n_vertices, records, device=False):
    """(refined indices [4 F, 3] uint32, stencils [6 E + 4 V] uint32) for the E = len(records) records given.  device: entries out of
    range give the header's harmless output; else they raise OutOfRange."""
    idx = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.uint64)
    rec = np.asarray(records, np.uint32).reshape(-1, 4).astype(np.uint64)
    F, E, V = idx.shape[0], rec.shape[0], int(n_vertices)
    if not device and (idx >= V).any():
        raise OutOfRange
    lo, hi, f0, f1 = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    no_edge = f0 == NONE
    has1 = f1 != NONE
    ok = ~no_edge & (lo < hi) & (hi < V) & (f0 < F) & (~has1 | (f1 < F))
    o0, ok0 = _opposite(idx, f0, lo, hi, V)
    o1, ok1 = _opposite(idx, f1, lo, hi, V)
    edge = ok & ok0 & (~has1 | ok1)
    if not device and (~no_edge & ~edge).any():
        raise OutOfRange
    boundary = ~has1 | (f1 == f0)
    odd = np.full((E, 4), NONE, np.uint64)
    odd[edge, 0], odd[edge, 1] = lo[edge], hi[edge]
    inner = edge & ~boundary
    odd[inner, 2], odd[inner, 3] = o0[inner], o1[inner]

    # the ring: (vertex, edge number, other endpoint) of both ends of every edge, by vertex, then by edge number
    e = np.flatnonzero(edge).astype(np.uint64)
    vert = np.concatenate([lo[edge], hi[edge]])
    other = np.concatenate([hi[edge], lo[edge]])
    num = np.concatenate([e, e])
    on_boundary = np.concatenate([boundary[edge], boundary[edge]])
    order = np.lexsort((num, vert))
    vert, other, on_boundary = vert[order], other[order], on_boundary[order]
    ring = np.full(2 * E, NONE, np.uint64)
    ring[:other.size] = other
    count = np.bincount(vert.astype(np.int64), minlength=V).astype(np.uint64)
    begin = np.where(count > 0, np.cumsum(count) - count, 0).astype(np.uint64)
    even = np.zeros((V, 4), np.uint64)
    even[:, 0], even[:, 1] = begin, count
    bv, bo = vert[on_boundary].astype(np.int64), other[on_boundary]          # still by vertex, then by edge number
    nb = np.bincount(bv, minlength=V)
    start = np.cumsum(nb) - nb
    own = np.arange(V, dtype=np.uint64)
    two = nb == 2
    even[:, 2] = np.where(nb == 0, NONE, own)
    even[:, 3] = even[:, 2]
    even[two, 2], even[two, 3] = bo[start[two]], bo[start[two] + 1]

    # the refined faces
    keys = (lo << np.uint64(32)) | hi
    refined = np.zeros((F, 12), np.uint64)
    a, b, c = idx[:, 0], idx[:, 1], idx[:, 2]
    usable = (a != b) & (b != c) & (c != a) & (idx < V).all(axis=1)
    mids = []
    for p, q in ((a, b), (b, c), (c, a)):
        plo, phi = np.minimum(p, q), np.maximum(p, q)
        at = _find(keys, (plo << np.uint64(32)) | phi) if E else np.zeros(F, np.int64)
        safe = np.minimum(at, max(E - 1, 0))
        named = (at < E) & (E > 0)
        if E:
            named &= (lo[safe] == plo) & (hi[safe] == phi) & edge[safe]
        usable_pair = named | ~usable
        if not device and not usable_pair.all():
            raise OutOfRange
        usable = usable & named
        mids.append(np.uint64(V) + safe.astype(np.uint64))
    m_ab, m_bc, m_ca = mids
    four = np.stack([a, m_ab, m_ca, b, m_bc, m_ab, c, m_ca, m_bc, m_ab, m_bc, m_ca], axis=1)
    refined[usable] = four[usable]
    stencils = np.concatenate([odd.reshape(-1), even.reshape(-1), ring]).astype(np.uint32)
    return refined.reshape(4 * F, 3).astype(np.uint32), stencils


def beta(count):
    return 0.1875 if count <= 3 else 3.0 / (8.0 * float(count))


def vertices(verts, stencils, n_edges, mode=LOOP, smooth=3, device=False):
    """refined vertices [V + E, stride] float64.  device: a stencil word that names no vertex gives a zero record (odd) or a copy
    (even); else it raises OutOfRange."""
    verts = np.ascontiguousarray(verts, np.float64)
    V, S = verts.shape
    E = int(n_edges)
    st = np.asarray(stencils, np.uint32).astype(np.int64)
    odd, even, ring = st[:4 * E].reshape(E, 4), st[4 * E:4 * E + 4 * V].reshape(V, 4), st[4 * E + 4 * V:]
    assert ring.size == 2 * E
    x = verts.tolist()
    bits = verts.view(np.uint64)
    out = np.zeros((V + E, S), np.float64)
    out_bits = out.view(np.uint64)
    sm = int(smooth) if mode == LOOP else 0

    def put(r, d, value):
        if value != value:
            out_bits[r, d] = CANONICAL_NAN
        else:
            out[r, d] = value

    def refuse():
        if not device:
            raise OutOfRange

    jobs = []                                                            # computed after every word is checked: a refusal writes nothing
    for v in range(V):
        out_bits[v] = bits[v]                                            # a copy keeps its 64 bits
        begin, count, b0, b1 = (int(w) for w in even[v])
        if begin + count > 2 * E:
            refuse()
            continue
        if b0 == NONE and b1 == NONE:
            if count == 0:
                continue
            entries = [int(w) for w in ring[begin:begin + count]]
            if any(n >= V for n in entries):
                refuse()
                continue
            jobs.append(("ring", v, entries))
        elif b0 >= V or b1 >= V:
            refuse()
        elif not (b0 == v and b1 == v):
            jobs.append(("edge", v, (b0, b1)))
    for e in range(E):
        lo, hi, o0, o1 = (int(w) for w in odd[e])
        if lo == NONE and hi == NONE and o0 == NONE and o1 == NONE:
            continue                                                     # all +0.0
        if lo >= V or hi >= V:
            refuse()
            continue
        if o0 == NONE and o1 == NONE:
            jobs.append(("mid", e, (lo, hi)))
        elif o0 >= V or o1 >= V:
            refuse()
        else:
            jobs.append(("full", e, (lo, hi, o0, o1)))
    for what, n, w in jobs:
        if what == "ring":
            count = len(w)
            bt = beta(count)
            a = 1.0 - float(count) * bt
            for d in range(sm):
                total = 0.0
                for k in w:
                    total = total + x[k][d]
                p, q = a * x[n][d], bt * total
                put(n, d, p + q)
        elif what == "edge":
            for d in range(sm):
                p, q = 0.75 * x[n][d], 0.125 * (x[w[0]][d] + x[w[1]][d])
                put(n, d, p + q)
        else:
            for d in range(S):
                if what == "full" and d < sm:
                    s, t = x[w[0]][d] + x[w[1]][d], x[w[2]][d] + x[w[3]][d]
                    p, q = 0.375 * s, 0.125 * t
                    put(V + n, d, p + q)
                else:
                    put(V + n, d, 0.5 * (x[w[0]][d] + x[w[1]][d]))
    return out
