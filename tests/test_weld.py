"""Mesh welding in host memory (include/trgl.h: trgl_mesh_weld; csrc/weld_core.h, host_mesh_weld) against tests/weld_model.py, bit for
bit: a hand-made case with its arrays written out, seeded arrays from no duplicate to one key, the special values of IEEE ==, keys
inside a record, grid cells at their borders, every output left out in turn, every refusal, and the cube of an OBJ reader, whose
seams trgl_mesh_edges reports until it is welded.  The model proves itself on the same cases; the hash the device path sorts by is
shown to collide in its low bits on the seeds tests/test_weld_gpu.py uses."""
import ctypes as C

import numpy as np
import pytest

import weld_cases as WC
import weld_model as M
from tinyrenderder_amd import api

NONE = M.NONE
INVALID, UNSUPPORTED = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(v, layout_key, cell=0.0, indices=None, what=""):
    """the host path against the model; returns the model's (remap, firsts, vertices, indices, n_unique)"""
    key_offset, key_count = layout_key
    with np.errstate(all="ignore"):
        want = M.weld(v, key_offset, key_count, cell, indices)
    P = api.make_weld_params(v.shape[1], key_offset, key_count, cell)
    before = v.copy()
    out, n = api.mesh_weld(P, v, indices)
    what = f"{what}: n={v.shape[0]} stride={v.shape[1]} key=({key_offset},{key_count}) cell={cell}"
    assert n == want[4], f"{what}: {n} distinct vertices, the model has {want[4]}"
    assert np.array_equal(out["remap"], want[0]), f"{what}: remap"
    assert np.array_equal(out["firsts"], want[1]), f"{what}: firsts"
    assert np.array_equal(_bits(out["vertices"]), _bits(want[2])), f"{what}: records"
    if indices is None:
        assert out["indices"] is None
    else:
        assert np.array_equal(out["indices"], want[3]), f"{what}: indices"
    assert np.array_equal(_bits(v), _bits(before)), f"{what}: the input was written to"
    return want


def test_the_hand_made_case_gives_the_arrays_written_out():
    v, remap, firsts, U = WC.hand_made()
    out, n = api.mesh_weld(api.make_weld_params(4, 1, 2), v, np.array([[0, 2, 7], [4, 5, 6]], np.uint32))
    assert n == U == 5
    assert out["remap"].tolist() == remap == [0, 1, 0, 2, 2, 3, 4, 1]
    assert out["firsts"].tolist() == firsts == [0, 1, 3, 5, 6, NONE, NONE, NONE]
    assert out["indices"].tolist() == [[0, 0, 1], [2, 3, 4]]
    assert np.array_equal(_bits(out["vertices"][:5]), _bits(v[[0, 1, 3, 5, 6]])) and not _bits(out["vertices"][5:]).any()
    assert np.signbit(out["vertices"][2, 2]) and not np.signbit(out["vertices"][2, 1]), "-0.0 stays -0.0: vertex 3's record, bit for bit"
    # ... and the model agrees with the literals
    want = M.weld(v, 1, 2)
    assert want[0].tolist() == remap and want[1].tolist() == firsts and want[4] == U


@pytest.mark.parametrize("dup", [0.0, 0.1, 0.5, 0.83, 1.0])
def test_seeded_arrays_at_every_duplicate_rate(dup):
    for k, (n, (stride, ko, kc)) in enumerate(zip([1, 2, 7, 64, 257, 1000, 3000, 500], WC.LAYOUTS)):
        v = WC.seeded(n, stride, ko, kc, dup, 100 + k)
        idx = (WC.scenes.SplitMix64(k).u64(3 * (n + 3)) % np.uint64(n)).astype(np.uint32).reshape(-1, 3)
        remap, firsts, out, _, U = _check(v, (ko, kc), indices=idx, what=f"dup {dup}")
        if dup == 0.0:
            assert U == n and np.array_equal(remap, np.arange(n)) and np.array_equal(_bits(out), _bits(v)), "a mesh without duplicates maps to itself"
        elif dup == 1.0:
            assert U == 1 and not remap.any() and firsts[0] == 0 and np.array_equal(_bits(out[0]), _bits(v[0]))
        elif n >= 64:
            assert U < n and (np.diff(firsts[:U].astype(np.int64)) > 0).all(), "representatives are numbered in ascending old number"


def test_signed_zeros_infinities_and_nans():
    v, ko, kc = WC.special_values()
    remap, firsts, out, _, U = _check(v, (ko, kc), what="special values")
    r = remap.tolist()
    assert r[0] == r[1] == r[2] == r[19], "-0.0 equals +0.0 in every component"
    assert r[3] == r[4] and len({r[3], r[5], r[6]}) == 3, "infinities of one sign are equal, of two signs not"
    nan_rows = [7, 8, 9, 11, 20, 21]
    assert len({r[i] for i in nan_rows}) == len(nan_rows) and all(firsts[r[i]] == i for i in nan_rows), "a key with a NaN joins nothing: bit-identical NaN vertices stay two"
    assert r[12] == r[14] != r[13] and r[13] != r[0], "denormals are values like any other"
    assert r[10] == r[15] and r[16] == r[18] and len({r[10], r[16], r[17]}) == 3, "one ulp apart is apart"
    assert np.array_equal(_bits(out[r[1]]), _bits(v[0])) and np.array_equal(_bits(out[r[8]]), _bits(v[8])), "the kept record is the lower-numbered vertex's"
    # the same keys as the whole record and as a single double
    _check(np.ascontiguousarray(v[:, ko:ko + kc]), (0, kc), what="special values, whole record")
    _check(v, (ko, 1), what="special values, one double")


def test_a_key_inside_the_record_ignores_the_rest():
    for stride, ko, kc in WC.LAYOUTS:
        v = WC.seeded(40, stride, ko, kc, 0.0, 5)
        v[13, ko:ko + kc] = v[4, ko:ko + kc]
        v[30, ko:ko + kc] = v[4, ko:ko + kc]
        remap, firsts, out, _, U = _check(v, (ko, kc), what="key inside")
        assert U == 38 and remap[13] == remap[30] == remap[4] == 4
        assert np.array_equal(_bits(out[4]), _bits(v[4])), "the record kept is the lower-numbered one's, bit for bit"
        if kc < stride:
            w = v.copy()                                                   # a difference inside the key keeps them apart
            w[13, ko] = np.nextafter(w[13, ko], np.inf)
            assert _check(w, (ko, kc), what="key differs")[4] == 39


def test_grid_cells_at_their_borders():
    v, q = WC.cell_values()
    with np.errstate(all="ignore"):
        got_q = [M.q_value(x, WC.CELL) for x in v[:, 1]]
    for x, g, w in zip(v[:, 1], got_q, q):
        assert g == w or (g != g and w != w), f"the model's q of {x!r} is {g!r}, the contract gives {w!r}"
    remap, firsts, out, _, U = _check(v, (1, 1), cell=WC.CELL, what="cells")
    for i in range(len(q)):
        for j in range(i):
            assert (remap[i] == remap[j]) == (q[i] == q[j]), f"vertices {j} ({v[j, 1]!r}) and {i} ({v[i, 1]!r}): cells {q[j]} and {q[i]}"
    x = v[:, 1].tolist()
    assert remap[x.index(0.1)] != remap[x.index(0.125)], "a grid weld, not a distance weld: 0.1 and 0.125 lie on either side of a border"
    assert remap[x.index(-0.125)] == remap[x.index(0.0)] and remap[x.index(-0.1)] == remap[x.index(0.0)], "x / cell = -0.5 is cell 0, and -0.0 equals 0.0"
    # other widths, over seeded values: a width that is no power of two (the division rounds), a tiny one, the smallest denormal (every quotient overflows: cells -inf and +inf) and a huge one
    rng = WC.scenes.SplitMix64(9)
    w = np.ascontiguousarray(rng.uniform(600 * 4, -2.0, 2.0).reshape(-1, 4))
    for cell, lo, hi in ((0.1, 60, 600), (1.0 / 3.0, 20, 600), (1e-9, 600, 600), (5e-324, 2, 8), (1e300, 1, 1), (3.0, 2, 27)):
        assert lo <= _check(w, (1, 3), cell=cell, what="cell width")[4] <= hi
        _check(w, (0, 1), cell=cell, what="cell width, one double")


def test_indices_are_optional_and_every_output_may_be_left_out():
    v = WC.seeded(300, 5, 1, 2, 0.5, 3)
    idx = (WC.scenes.SplitMix64(4).u64(3 * 90) % np.uint64(300)).astype(np.uint32).reshape(-1, 3)
    want = M.weld(v, 1, 2, 0.0, idx)
    P = api.make_weld_params(5, 1, 2)
    L = api.load_library()
    full = dict(remap=want[0], firsts=want[1], vertices=want[2], indices=want[3])
    for left_out in (None,) + api.WELD_OUTPUTS:
        names = [k for k in api.WELD_OUTPUTS if k != left_out]
        _, out, n = api._mesh_weld(L, None, P, v, idx, False, {k: None for k in names}, True)
        assert n == want[4] and out.get(left_out) is None
        for k in names:
            assert np.array_equal(out[k].view(np.uint32), np.ascontiguousarray(full[k]).view(np.uint32)), f"{k} without {left_out}"
    # no indices: remap is the index array of a soup; no count either
    _, out, n = api._mesh_weld(L, None, P, v, None, False, dict(remap=None), False)
    assert n is None and np.array_equal(out["remap"], want[0])
    # indices without indices_out are still checked in host memory
    bad = idx.copy(); bad[7, 1] = 300
    with pytest.raises(api.TrglError, match="index out of range"):
        api._mesh_weld(L, None, P, v, bad, False, dict(remap=None), True)
    # nothing to weld
    n = C.c_uint64(7)
    assert L.trgl_mesh_weld(None, C.byref(P), None, 0, None, 0, api.MEM_HOST, None, None, None, None, C.byref(n)) == 0 and n.value == 0


def test_every_refusal_and_nothing_written():
    L = api.load_library()
    v = WC.seeded(16, 4, 0, 3, 0.5, 1)
    idx = np.array([[0, 1, 2], [3, 15, 5]], np.uint32)
    S32, S64 = WC.SENTINEL_U32, WC.SENTINEL_F64
    outs = [np.full(16, S32, np.uint32), np.full(16, S32, np.uint32), np.full((16, 4), S64), np.full((2, 3), S32, np.uint32)]
    n = C.c_uint64(99)
    p = api._ptr

    def call(P=None, vertices=v, nv=16, indices=idx, nf=2, mem=api.MEM_HOST, o=outs, ctx=None, count=n):
        P = api.make_weld_params(4, 0, 3) if P is None else P
        return L.trgl_mesh_weld(ctx, None if P == "null" else C.byref(P), p(vertices), nv, p(indices), nf, mem, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                None if count is None else C.byref(count))

    def params(**kw):
        P = api.make_weld_params(4, 0, 3)
        for k, x in kw.items():
            setattr(P, k, x)
        return P

    refusals = {
        "bad mem_kind": dict(mem=7), "device memory without a context": dict(mem=api.MEM_DEVICE), "params NULL": dict(P="null"),
        "reserved32": dict(P=params(reserved32=1)), "reserved": dict(P=params(reserved=1)), "stride 0": dict(P=params(vertex_stride=0)),
        "negative offset": dict(P=params(key_offset=-1)), "count 0": dict(P=params(key_count=0)), "key past the record": dict(P=params(key_offset=2)),
        "key count past the record": dict(P=params(key_count=5)), "offset + count overflows": dict(P=params(key_offset=2 ** 31 - 1, key_count=2 ** 31 - 1)),
        "negative cell": dict(P=params(cell=-0.5)), "NaN cell": dict(P=params(cell=float("nan"))), "infinite cell": dict(P=params(cell=float("inf"))),
        "null vertices": dict(vertices=None), "indices_out without indices": dict(indices=None),
        "misaligned vertices": dict(vertices=v.ctypes.data + 4), "misaligned remap": dict(o=[outs[0].ctypes.data + 2] + outs[1:]),
        "misaligned records out": dict(o=outs[:2] + [outs[2].ctypes.data + 4, outs[3]]),
        "misaligned indices": dict(indices=idx.ctypes.data + 1),
        "records out over the input": dict(o=outs[:2] + [v.ctypes.data + 8 * 4 * 15, outs[3]]),
        "indices out over the indices": dict(o=outs[:3] + [idx]), "remap over the vertices": dict(o=[v.ctypes.data] + outs[1:]),
        "two outputs overlap": dict(o=[outs[0], outs[0].ctypes.data + 4 * 15] + outs[2:]),
        "firsts over records out": dict(o=[outs[0], outs[2].ctypes.data + 8, outs[2], outs[3]]),
        "faces without vertices": dict(nv=0), "index out of range": dict(indices=np.array([[0, 1, 2], [3, 16, 5]], np.uint32)),
    }
    for what, kw in refusals.items():
        assert call(**kw) == INVALID, what
        assert api.load_library().trgl_last_error(None).decode().startswith("trgl_mesh_weld: "), what
    for what, kw in {"too many vertices": dict(nv=2 ** 31), "too many faces": dict(nf=(2 ** 31 - 1) // 3 + 1),
                     "records that do not fit": dict(P=params(vertex_stride=2 ** 31 - 1, key_count=1), nv=2 ** 31 - 1)}.items():
        assert call(**kw) == UNSUPPORTED, what
    assert all((o.view(np.uint32) == S32).all() for o in outs[:2] + outs[3:]) and (_bits(outs[2]) == _bits(np.array([S64]))[0]).all() and n.value == 99, \
        "a refused call wrote something"
    assert call() == 0 and n.value == M.weld(v, 0, 3)[4]
    assert call(count=None) == 0
    # the test hook for the hash checks its scalars the same way
    h = np.zeros(16, np.uint64)
    assert L.trgl_debug_weld_hash(C.byref(params(key_count=9)), p(v), 16, p(h)) == INVALID


def test_the_split_cube_has_seams_until_it_is_welded():
    v, idx = WC.split_cube()
    assert v.shape == (24, 6) and idx.shape == (12, 3)
    rec, E = api.mesh_edges(idx, 24)
    assert E == 30 and (rec[:E, 3] == NONE).sum() == 24, "split along every normal seam: the 24 sides of the six quads are boundaries"
    remap, firsts, out, new_idx, U = _check(v, (0, 3), indices=idx, what="cube by position")
    assert U == 8
    rec, E = api.mesh_edges(new_idx, U)
    assert E == 18 and (rec[:E, 3] != NONE).all(), "the 12 edges of the cube and the 6 diagonals of its quads, no boundary"
    # the diagonals aside, these are the cube's 12 edges
    d = out[rec[:E, 0], :3] - out[rec[:E, 1], :3]
    assert ((d * d).sum(1) == 4.0).sum() == 12
    # welding by the whole record joins nothing; by the normal alone, six vertices remain
    assert _check(v, (0, 6), what="cube by record")[4] == 24 and _check(v, (3, 3), what="cube by normal")[4] == 6
    # the head stand-in as a soup closes: E = 3 F / 2
    _, hv, hidx = WC.head_soup()
    remap, _, _, new_idx, U = _check(hv, (0, 3), indices=hidx, what="head soup")
    assert np.array_equal(new_idx.reshape(-1), remap), "for a soup remap is the index array"
    rec, E = api.mesh_edges(new_idx, U)
    assert 2 * E == 3 * hidx.shape[0] and (rec[:E, 3] != NONE).all() and U == E - hidx.shape[0] + 2


# ---- the hash of the device path ------------------------------------------------------------------------------------------------------
def test_identical_keys_hash_alike_and_low_bits_collide_on_the_gpu_tests_seeds():
    v, ko, kc = WC.special_values()
    h = api.weld_hashes(api.make_weld_params(v.shape[1], ko, kc), v)
    rep = M.representatives(v, ko, kc)
    assert all(h[u] == h[rep[u]] for u in range(len(rep))), "identical keys must hash alike (-0.0 as +0.0)"
    assert h[0] == h[1] == h[19] and h[3] == h[4]
    cv, _ = WC.cell_values()
    with np.errstate(all="ignore"):
        hc = api.weld_hashes(api.make_weld_params(2, 1, 1, WC.CELL), cv)
        repc = M.representatives(cv, 1, 1, WC.CELL)
    assert all(hc[u] == hc[repc[u]] for u in range(len(repc))), "cell mode hashes q"
    for n, stride, ko, kc, dup, seed in WC.COLLISION_CASES:
        w = WC.seeded(n, stride, ko, kc, dup, seed)
        full = api.weld_hashes(api.make_weld_params(stride, ko, kc), w)
        rep = M.representatives(w, ko, kc)
        assert len(set(full.tolist())) == len(set(rep)), "64 bits: no two keys of these cases collide"
        for bits in (3, 1, 0):
            mixed, walked = WC.collision_proof(w, ko, kc, bits)
            assert mixed >= 1 and (dup == 0.0 or walked > 0), f"n={n} bits={bits}: {mixed} mixed runs, {walked} walked vertices - the case forces no collision walk"
