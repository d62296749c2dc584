"""Mesh levels of detail in host memory (include/trgl.h: trgl_mesh_clean, trgl_mesh_simplify; csrc/lod_core.h, host_mesh_clean,
host_mesh_simplify) against tests/lod_model.py, bit for bit: a hand-made face list with its classes written out - every rotation of a
duplicate, a mirrored pair, a duplicate of a dropped face, degenerate faces of all shapes -, seeded face lists from no duplicate to all,
all faces dropped, no face at all, unreferenced vertices, both fills, every output left out in turn, sentinels behind every capacity,
every refusal; simplification as the caller's own weld + clean, as the identity, down to nothing, over special values and with the mean's
rules; and the properties of every result over seeded meshes, which the model asserts of its own output too."""
import ctypes as C

import numpy as np
import pytest

import lod_cases as LC
import lod_model as M
from tinyrenderder_amd import api

NONE = M.NONE
INVALID, UNSUPPORTED = -1, -5
BOTH = api.CLEAN_DUPLICATES | api.CLEAN_VERTICES
S32, S64 = LC.SENTINEL_U32, LC.SENTINEL_F64


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    """the five arrays and the counts of a clean or simplify result against the model's"""
    for k, w in want.items():
        if k == "counts":
            continue
        if w is None:
            assert got.get(k) is None, f"{what}: {k} was written"
        elif k == "vertices":
            assert np.array_equal(_bits(got[k]), _bits(w)), f"{what}: records"
        else:
            assert np.array_equal(got[k], w), f"{what}: {k}"


def _check_clean(idx, V, flags=BOTH, fill=api.CLEAN_FILL_NONE, vertices=None, what=""):
    want = M.clean(idx, V, flags, fill, vertices)
    before = idx.copy()
    stride = 0 if vertices is None else vertices.shape[1]
    got, counts = api.mesh_clean(api.make_clean_params(stride, flags, fill), idx, vertices, V)
    what = f"{what}: F={idx.shape[0]} V={V} flags={flags} fill={fill}"
    assert counts == want["counts"], f"{what}: counts {counts}, the model has {want['counts']}"
    _same(got, want, what)
    got["counts"] = counts
    M.check_clean_properties(got, bool(flags & 1), bool(flags & 2))
    assert np.array_equal(idx, before), f"{what}: the input was written to"
    return want


def _check_simplify(v, idx, cell, mean_count=3, fill=api.CLEAN_FILL_NONE, what=""):
    want = M.simplify(v, idx, cell, mean_count, fill)
    bv, bi = v.copy(), idx.copy()
    got, counts = api.mesh_simplify(api.make_simplify_params(v.shape[1], cell, mean_count, fill), v, idx)
    what = f"{what}: F={idx.shape[0]} n={v.shape[0]} cell={cell} mean_count={mean_count}"
    assert counts == want["counts"], f"{what}: counts {counts}, the model has {want['counts']}"
    _same(got, want, what)
    got["counts"] = counts
    M.check_clean_properties(dict(got, vfirsts=got["firsts"]), True, True)
    assert np.array_equal(_bits(v), _bits(bv)) and np.array_equal(idx, bi), f"{what}: an input was written to"
    return want


# ---- trgl_mesh_clean --------------------------------------------------------------------------------------------------------------------
def test_the_hand_made_faces_get_the_classes_written_out():
    idx, V, cls = LC.hand_made()
    assert M.classes(idx, V) == cls, "the model disagrees with the literals"
    v = LC.records(V, 4, 1)
    want = _check_clean(idx, V, vertices=v, what="hand made")
    assert want["counts"] == (3, 6)
    assert want["face_firsts"].tolist() == [0, 3, 11] + [NONE] * 11
    assert want["indices"][:3].tolist() == [[0, 1, 2], [2, 1, 0], [3, 4, 5]], "kept faces in their order and their original rotation"
    assert (want["indices"][3:] == NONE).all()
    assert want["vremap"].tolist() == [NONE, 0, 1, 2, NONE, NONE, NONE, NONE, 3, 4, 5, NONE], "unreferenced at the front, in the middle, at the end"
    assert want["vfirsts"].tolist() == [1, 2, 3, 8, 9, 10] + [NONE] * 6
    assert np.array_equal(_bits(want["vertices"][:6]), _bits(v[[1, 2, 3, 8, 9, 10]])) and not _bits(want["vertices"][6:]).any()
    # without TRGL_CLEAN_DUPLICATES every rotation and repetition stays; without TRGL_CLEAN_VERTICES the numbers stay
    want = _check_clean(idx, V, flags=api.CLEAN_VERTICES, vertices=v, what="hand made, duplicates kept")
    assert want["face_firsts"][:8].tolist() == [0, 1, 2, 3, 4, 11, 12, 13] and want["counts"] == (8, 6)
    want = _check_clean(idx, V, flags=api.CLEAN_DUPLICATES, fill=api.CLEAN_FILL_ZERO, what="hand made, old numbers")
    assert want["counts"] == (3, 12) and want["indices"][:3].tolist() == [[1, 2, 3], [3, 2, 1], [8, 9, 10]] and not want["indices"][3:].any()
    want = _check_clean(idx, V, flags=0, what="hand made, degenerates only")
    assert want["counts"] == (8, 12)


@pytest.mark.parametrize("dup", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("degen", [0.0, 0.25, 1.0])
def test_seeded_faces_at_every_duplicate_and_degenerate_rate(dup, degen):
    for k, (F, V, stride) in enumerate([(1, 3, 3), (2, 3, 5), (7, 5, 8), (64, 30, 3), (257, 400, 14), (1500, 300, 4)]):
        idx = LC.seeded_faces(F, V, dup, degen, 200 + k)
        v = LC.records(V, stride, k)
        for fill in (api.CLEAN_FILL_NONE, api.CLEAN_FILL_ZERO):
            want = _check_clean(idx, V, fill=fill, vertices=v, what=f"dup {dup} degen {degen}")
        K, U = want["counts"]
        if degen == 1.0:
            assert (K, U) == (0, 0) and (want["vremap"] == NONE).all() and not _bits(want["vertices"]).any(), "all faces dropped: every vertex leaves"
        elif dup == 1.0 and degen == 0.0:
            assert K == 1
        elif dup == 0.0 and degen == 0.0 and F < V:
            assert K >= F - 2
        _check_clean(idx, V, flags=api.CLEAN_DUPLICATES, what="old numbers")
        _check_clean(idx, V, flags=api.CLEAN_VERTICES, vertices=v, what="duplicates kept")


def test_no_faces_and_every_output_left_out_in_turn():
    L = api.load_library()
    v = LC.records(9, 3, 2)
    out, counts = api.mesh_clean(api.make_clean_params(3), np.zeros((0, 3), np.uint32), v)
    assert counts == (0, 0) and (out["vremap"] == NONE).all() and (out["vfirsts"] == NONE).all() and not _bits(out["vertices"]).any()
    out, counts = api.mesh_clean(api.make_clean_params(0, api.CLEAN_DUPLICATES), np.zeros((0, 3), np.uint32), None, 9)
    assert counts == (0, 9)
    n = (C.c_uint64 * 2)(7, 7)
    assert L.trgl_mesh_clean(None, C.byref(api.make_clean_params(3)), None, 0, None, 0, api.MEM_HOST, None, None, None, None, None, n) == 0
    assert (n[0], n[1]) == (0, 0)
    idx = LC.seeded_faces(300, 80, 0.4, 0.2, 9)
    v = LC.records(80, 5, 3)
    want = M.clean(idx, 80, vertices=v)
    P = api.make_clean_params(5)
    for left_out in (None,) + api.CLEAN_OUTPUTS:
        names = [k for k in api.CLEAN_OUTPUTS if k != left_out]
        _, out, counts = api._mesh_clean(L, None, P, idx, v, None, False, {k: None for k in names}, left_out != "indices")
        assert counts == (want["counts"] if left_out != "indices" else None) and out.get(left_out) is None
        _same(out, {k: want[k] for k in names}, f"without {left_out}")
    # vertices may be NULL when no record is written, with the flag and without
    _, out, counts = api._mesh_clean(L, None, api.make_clean_params(0), idx, None, 80, False, None, True)
    assert counts == want["counts"] and out["vertices"] is None and np.array_equal(out["vremap"], want["vremap"])


def test_every_output_of_a_simplification_left_out_in_turn():
    L = api.load_library()
    idx = LC.seeded_faces(300, 80, 0.2, 0.1, 9)
    v = LC.records(80, 5, 3)
    v[:, :3] /= 3.0
    for mean_count in (0, 3):
        P = api.make_simplify_params(5, 1.0, mean_count)
        want = M.simplify(v, idx, 1.0, mean_count)
        assert 0 < want["counts"][0] < 300 and 0 < want["counts"][1] < 80
        for left_out in (None,) + api.SIMPLIFY_OUTPUTS:
            names = [k for k in api.SIMPLIFY_OUTPUTS if k != left_out]
            _, out, counts = api._mesh_simplify(L, None, P, v, idx, False, {k: None for k in names}, left_out != "remap")
            assert counts == (want["counts"] if left_out != "remap" else None) and out.get(left_out) is None
            _same(out, {k: want[k] for k in names}, f"mean_count {mean_count} without {left_out}")
        for only in api.SIMPLIFY_OUTPUTS:                                 # ... and each output alone: without the records no mean is taken
            _, out, counts = api._mesh_simplify(L, None, P, v, idx, False, {only: None}, True)
            assert counts == want["counts"]
            _same(out, {only: want[only]}, f"mean_count {mean_count}, {only} alone")
    _, out, counts = api._mesh_simplify(L, None, api.make_simplify_params(5, 1.0), v, idx, False, {}, True)
    assert counts == M.simplify(v, idx, 1.0)["counts"] and all(x is None for x in out.values())


def test_nothing_behind_a_capacity_is_written():
    idx = LC.seeded_faces(100, 40, 0.3, 0.2, 4)
    v = LC.records(40, 3, 4)
    F, V = 100, 40
    o = [np.full(3 * F + 3, S32, np.uint32), np.full(F + 3, S32, np.uint32), np.full(V + 3, S32, np.uint32), np.full(V + 3, S32, np.uint32), np.full(3 * V + 3, S64)]
    L, p = api.load_library(), api._ptr
    n = (C.c_uint64 * 2)()
    P = api.make_clean_params(3)
    assert L.trgl_mesh_clean(None, C.byref(P), p(idx), F, p(v), V, api.MEM_HOST, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), n) == 0
    want = M.clean(idx, V, vertices=v)
    assert np.array_equal(o[0][:3 * F].reshape(F, 3), want["indices"]) and np.array_equal(o[2][:V], want["vremap"])
    assert all((a[-3:] == S32).all() for a in o[:4]) and (_bits(o[4][-3:]) == _bits(np.array([S64]))[0]).all()
    s = [np.full(V + 3, S32, np.uint32), np.full(V + 3, S32, np.uint32), np.full(3 * V + 3, S64), np.full(3 * F + 3, S32, np.uint32), np.full(F + 3, S32, np.uint32)]
    Q = api.make_simplify_params(3, 4.0)
    assert L.trgl_mesh_simplify(None, C.byref(Q), p(v), V, p(idx), F, api.MEM_HOST, p(s[0]), p(s[1]), p(s[2]), p(s[3]), p(s[4]), n) == 0
    want = M.simplify(v, idx, 4.0)
    assert (n[0], n[1]) == want["counts"] and np.array_equal(s[0][:V], want["remap"]) and np.array_equal(s[3][:3 * F].reshape(F, 3), want["indices"])
    assert all((a[-3:] == S32).all() for a in s[:2] + s[3:]) and (_bits(s[2][-3:]) == _bits(np.array([S64]))[0]).all()


def test_every_refusal_of_a_clean_and_nothing_written():
    L, p = api.load_library(), api._ptr
    idx = np.array([[0, 1, 2], [3, 15, 5]], np.uint32)
    v = LC.records(16, 4, 1)
    outs = [np.full((2, 3), S32, np.uint32), np.full(2, S32, np.uint32), np.full(16, S32, np.uint32), np.full(16, S32, np.uint32), np.full((16, 4), S64)]
    n = (C.c_uint64 * 2)(99, 99)

    def call(P=None, indices=idx, nf=2, vertices=v, nv=16, mem=api.MEM_HOST, o=outs, ctx=None, count=n):
        P = api.make_clean_params(4) if P is None else P
        return L.trgl_mesh_clean(ctx, None if P == "null" else C.byref(P), p(indices), nf, p(vertices), nv, mem, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), count)

    def params(**kw):
        P = api.make_clean_params(4)
        for k, x in kw.items():
            setattr(P, k, x)
        return P

    refusals = {
        "bad mem_kind": dict(mem=7), "device memory without a context": dict(mem=api.MEM_DEVICE), "params NULL": dict(P="null"),
        "reserved32": dict(P=params(reserved32=1)), "reserved": dict(P=params(reserved=1)), "unknown flags": dict(P=params(flags=4 | 3)),
        "unknown fill": dict(P=params(fill=2)), "stride 0 where it is read": dict(P=params(vertex_stride=0)),
        "negative stride": dict(P=params(vertex_stride=-4)),
        "vremap without the flag": dict(P=params(flags=1), o=outs[:2] + [outs[2], None, None]),
        "vfirsts without the flag": dict(P=params(flags=1), o=outs[:2] + [None, outs[3], None]),
        "records without the flag": dict(P=params(flags=0), o=outs[:2] + [None, None, outs[4]]),
        "records without vertices": dict(vertices=None), "null indices": dict(indices=None),
        "misaligned indices": dict(indices=idx.ctypes.data + 2), "misaligned vertices": dict(vertices=v.ctypes.data + 4),
        "misaligned records out": dict(o=outs[:4] + [outs[4].ctypes.data + 4]), "misaligned vremap": dict(o=outs[:2] + [outs[2].ctypes.data + 1] + outs[3:]),
        "misaligned face_firsts": dict(o=[outs[0], outs[1].ctypes.data + 2] + outs[2:]),
        "indices out over the indices": dict(o=[idx] + outs[1:]), "records out over the input": dict(o=outs[:4] + [v.ctypes.data + 8 * 4 * 15]),
        "vremap over the vertices": dict(o=outs[:2] + [v.ctypes.data] + outs[3:]), "two outputs overlap": dict(o=outs[:3] + [outs[2].ctypes.data + 4 * 15, outs[4]]),
        "face_firsts over indices out": dict(o=[outs[0], outs[0].ctypes.data + 20] + outs[2:]),
        "faces without vertices": dict(nv=0), "index out of range": dict(indices=np.array([[0, 1, 2], [3, 16, 5]], np.uint32)),
        "index NONE": dict(indices=np.array([[0, 1, 2], [NONE, NONE, NONE]], np.uint32)),
    }
    for what, kw in refusals.items():
        assert call(**kw) == INVALID, what
        assert L.trgl_last_error(None).decode().startswith("trgl_mesh_clean: "), what
    for what, kw in {"too many vertices": dict(nv=2 ** 31), "too many faces": dict(nf=(2 ** 31 - 1) // 3 + 1),
                     "records that do not fit": dict(P=params(vertex_stride=2 ** 31 - 1), nv=2 ** 31 - 1)}.items():
        assert call(**kw) == UNSUPPORTED, what
    assert all((o.view(np.uint32) == S32).all() for o in outs[:4]) and (_bits(outs[4]) == _bits(np.array([S64]))[0]).all() and (n[0], n[1]) == (99, 99), \
        "a refused call wrote something"
    # the stride is not read where no record is written
    assert call(P=params(vertex_stride=0), o=outs[:4] + [None]) == 0 and call(P=params(vertex_stride=-1, flags=1), vertices=None, o=outs[:2] + [None] * 3) == 0
    assert call() == 0 and (n[0], n[1]) == (2, 6)
    assert call(count=None) == 0


def test_every_refusal_of_a_simplification_and_nothing_written():
    L, p = api.load_library(), api._ptr
    idx = np.array([[0, 1, 2], [3, 15, 5]], np.uint32)
    v = LC.records(16, 4, 1)
    outs = [np.full(16, S32, np.uint32), np.full(16, S32, np.uint32), np.full((16, 4), S64), np.full((2, 3), S32, np.uint32), np.full(2, S32, np.uint32)]
    n = (C.c_uint64 * 2)(99, 99)

    def call(P=None, vertices=v, nv=16, indices=idx, nf=2, mem=api.MEM_HOST, o=outs, count=n):
        P = api.make_simplify_params(4, 0.5) if P is None else P
        return L.trgl_mesh_simplify(None, None if P == "null" else C.byref(P), p(vertices), nv, p(indices), nf, mem, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), count)

    def params(**kw):
        P = api.make_simplify_params(4, 0.5)
        for k, x in kw.items():
            setattr(P, k, x)
        return P

    refusals = {
        "bad mem_kind": dict(mem=7), "device memory without a context": dict(mem=api.MEM_DEVICE), "params NULL": dict(P="null"),
        "reserved32": dict(P=params(reserved32=1)), "reserved": dict(P=params(reserved=1)), "unknown fill": dict(P=params(fill=2)),
        "stride 2": dict(P=params(vertex_stride=2, mean_count=0)), "negative mean_count": dict(P=params(mean_count=-1)),
        "mean_count past the record": dict(P=params(mean_count=5)), "negative cell": dict(P=params(cell=-0.5)), "NaN cell": dict(P=params(cell=float("nan"))),
        "infinite cell": dict(P=params(cell=float("inf"))), "null vertices": dict(vertices=None), "null indices": dict(indices=None),
        "misaligned vertices": dict(vertices=v.ctypes.data + 4), "misaligned indices": dict(indices=idx.ctypes.data + 1),
        "misaligned remap": dict(o=[outs[0].ctypes.data + 2] + outs[1:]), "misaligned records out": dict(o=outs[:2] + [outs[2].ctypes.data + 4] + outs[3:]),
        "records out over the input": dict(o=outs[:2] + [v.ctypes.data + 8 * 4 * 15] + outs[3:]), "indices out over the indices": dict(o=outs[:3] + [idx, outs[4]]),
        "remap over the vertices": dict(o=[v.ctypes.data] + outs[1:]), "two outputs overlap": dict(o=[outs[0], outs[0].ctypes.data + 4 * 15] + outs[2:]),
        "face_firsts over indices out": dict(o=outs[:4] + [outs[3].ctypes.data + 20]),
        "faces without vertices": dict(nv=0), "index out of range": dict(indices=np.array([[0, 1, 2], [3, 16, 5]], np.uint32)),
    }
    for what, kw in refusals.items():
        assert call(**kw) == INVALID, what
        assert L.trgl_last_error(None).decode().startswith("trgl_mesh_simplify: "), what
    for what, kw in {"too many vertices": dict(nv=2 ** 31), "too many faces": dict(nf=(2 ** 31 - 1) // 3 + 1),
                     "records that do not fit": dict(P=params(vertex_stride=2 ** 31 - 1, mean_count=0), nv=2 ** 31 - 1)}.items():
        assert call(**kw) == UNSUPPORTED, what
    assert all((o.view(np.uint32) == S32).all() for o in outs[:2] + outs[3:]) and (_bits(outs[2]) == _bits(np.array([S64]))[0]).all() and (n[0], n[1]) == (99, 99), \
        "a refused call wrote something"
    assert call() == 0 and (n[0], n[1]) == M.simplify(v, idx, 0.5)["counts"]
    assert call(count=None) == 0 and call(nv=0, nf=0, vertices=None, indices=None) == 0 and (n[0], n[1]) == (0, 0)


# ---- trgl_mesh_simplify -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 14])
def test_without_a_mean_it_is_the_callers_own_weld_and_clean(stride):
    v, idx = LC.octa_sphere(3, stride)
    for cell in (0.0, 0.3, 0.7):
        want = _check_simplify(v, idx, cell, mean_count=0, what="composition")
        w, U = api.mesh_weld(api.make_weld_params(stride, 0, 3, cell), v, idx)
        c, counts = api.mesh_clean(api.make_clean_params(stride), w["indices"], w["vertices"])
        assert counts == want["counts"]
        for k in ("indices", "face_firsts"):
            assert np.array_equal(c[k], want[k]), k
        assert np.array_equal(_bits(c["vertices"]), _bits(want["vertices"]))
        assert np.array_equal(c["vremap"][w["remap"]], want["remap"])
        assert np.array_equal(w["firsts"][c["vfirsts"][:counts[1]]], want["firsts"][:counts[1]]) and (want["firsts"][counts[1]:] == NONE).all()
        if cell == 0.0:
            assert counts == (idx.shape[0], v.shape[0]) and np.array_equal(want["indices"], idx) and np.array_equal(_bits(want["vertices"]), _bits(v)), \
                "cell 0 on a clean closed mesh is the identity"
            assert np.array_equal(want["remap"], np.arange(v.shape[0])) and np.array_equal(want["face_firsts"], np.arange(idx.shape[0]))
        else:
            assert 0 < counts[0] < idx.shape[0] and 0 < counts[1] < v.shape[0]
    want = _check_simplify(v, idx, 0.0, mean_count=3, what="identity with a mean")
    assert np.array_equal(_bits(want["vertices"]), _bits(v)), "one member per cell: every record keeps its bits"
    want = _check_simplify(v, idx, 8.0, what="a cell wider than the mesh")
    assert want["counts"] == (0, 0) and (want["remap"] == NONE).all() and (want["indices"] == NONE).all() and not _bits(want["vertices"]).any()


def test_the_mean_is_taken_over_referenced_members_in_ascending_order():
    # cell 1.0: vertices 0, 2, 5 and 6 share the cell (0, 0, 0); 6 is named by no face; 1, 3, 4 have cells of their own
    v = np.array([[0.1, 0.2, -0.3, 7.0], [2.0, 0.0, 0.0, 8.0], [1e-17, 0.4, 0.3, 9.0], [0.0, 2.0, 0.0, 10.0], [0.0, 0.0, 2.0, 11.0], [-0.4, 0.1, 0.3, 12.0],
                  [0.45, 0.45, 0.45, 13.0]], np.float64)
    idx = np.array([[0, 1, 3], [2, 3, 4], [5, 4, 1]], np.uint32)
    want = _check_simplify(v, idx, 1.0, mean_count=3, what="mean")
    assert want["counts"] == (3, 4) and want["firsts"][:4].tolist() == [0, 1, 3, 4]
    s = [np.float64(np.float64(v[0, a] + v[2, a]) + v[5, a]) / np.float64(3.0) for a in range(3)]
    assert _bits(want["vertices"][0, :3]).tolist() == _bits(np.array(s)).tolist(), "(v0 + v2) + v5, then one division; vertex 6 is left out"
    assert want["vertices"][0, 3] == 7.0, "doubles behind mean_count are the representative's"
    assert np.array_equal(_bits(want["vertices"][1]), _bits(v[1]))
    # mean_count = the whole record, and 1
    _check_simplify(v, idx, 1.0, mean_count=4, what="mean of the whole record")
    want1 = _check_simplify(v, idx, 1.0, mean_count=1, what="mean of x alone")
    assert want1["vertices"][0, 1] == 0.2
    # one referenced member keeps its bits - here -0.0, which a sum with +0.0 or a division would not all keep -, and when that member is
    # not the representative the record is still the representative's behind mean_count
    w = np.array([[0.25, 0.0, 0.0, 1.0], [-0.0, -0.0, -0.0, 2.0], [3.0, 0.0, 0.0, 3.0], [0.0, 3.0, 0.0, 4.0]], np.float64)
    want = _check_simplify(w, np.array([[1, 2, 3]], np.uint32), 1.0, mean_count=3, what="one referenced member")
    assert want["counts"] == (1, 3) and want["firsts"][0] == 0
    assert np.signbit(want["vertices"][0, :3]).all() and want["vertices"][0, 3] == 1.0
    # a cluster that no face names at all leaves with the clean; its record was the representative's
    want = _check_simplify(w, np.array([[1, 2, 3], [0, 1, 2]], np.uint32), 1.0, mean_count=3, what="both members")
    assert want["counts"] == (1, 3) and want["vertices"][0, 0] == 0.125 and not np.signbit(want["vertices"][0, 1])


def test_special_positions():
    v, idx = LC.special_positions()
    for cell in (0.0, 0.5):
        for mean_count in (0, 3, 5):
            want = _check_simplify(v, idx, cell, mean_count, what="special")
        r = want["remap"].tolist()
        assert r[0] == r[1] == r[10], "-0.0 equals +0.0"
        assert r[4] == r[5] != NONE, "infinities of one sign are equal"
        assert r[6] != r[7] and NONE not in (r[6], r[7]), "a NaN position clusters with nothing"
        assert r[9] == r[8] and r[11] == r[13]
        K = want["counts"][0]
        assert want["face_firsts"][:K].tolist() == [0, 2, 3, 5, 6, 7, 9, 10], "faces 1, 4 and 8 repeat 0, 3 and 7; face 2 is face 0 mirrored and stays; 11 collapses"
    want = _check_simplify(v, idx, 0.0, 3, what="special, cell 0")
    j = want["remap"][0]
    assert not np.signbit(want["vertices"][j, :3]).any(), "(+0.0 + -0.0 + -0.0) / 3 is +0.0"


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_properties_over_seeded_meshes(seed):
    F, V = 400 + 37 * seed, 150 + 11 * seed
    idx = LC.seeded_faces(F, V, 0.2, 0.1, 300 + seed)
    v = LC.records(V, 3 + seed, 400 + seed)
    v[:, :3] /= 3.0
    _check_clean(idx, V, vertices=v, what="properties")                   # (_check_* run check_clean_properties on the library's output)
    for cell in (0.0, 0.5, 1.5, 4.0):
        want = _check_simplify(v, idx, cell, mean_count=seed % 4, what="properties")
        K, U = want["counts"]
        assert (want["remap"][want["firsts"][:U]] == np.arange(U)).all(), "firsts and remap are inverse on the kept clusters"
    # a second level over the first's exact outputs
    first, (K, U) = api.mesh_simplify(api.make_simplify_params(3 + seed, 0.5), v, idx)
    _check_simplify(np.ascontiguousarray(first["vertices"][:U]), np.ascontiguousarray(first["indices"][:K]), 1.0, what="second level")


def test_the_face_hash_brings_rotations_together_and_low_bits_collide_on_the_gpu_tests_seeds():
    idx, V, cls = LC.hand_made()
    h = api.lod_face_hashes(idx, V)
    assert h[0] == h[1] == h[2] == h[12] and h[3] == h[4] and h[11] == h[13] and h[0] != h[3], "rotations hash alike, a mirrored face apart"
    assert len({int(h[f]) for f in (5, 6, 7, 8, 9, 10)}) == 6, "dropped faces are identical to nothing: each sorts by its own number"
    for F, Vn, dup, degen, seed in LC.COLLISION_CASES:
        faces = LC.seeded_faces(F, Vn, dup, degen, seed)
        for bits in (3, 1, 0):
            mixed, walked = LC.collision_proof(faces, Vn, bits)
            assert mixed >= 1 and (dup == 0.0 or walked > 0), f"F={F} bits={bits}: {mixed} mixed runs, {walked} walked faces - the case forces no collision walk"
