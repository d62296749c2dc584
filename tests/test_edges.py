"""Mesh edges in host memory (include/trgl.h: trgl_mesh_edges, trgl_edge_select; no GPU).

The host twins equal tests/edge_model.py on every mesh of tests/edge_cases.py - records, fill, count, code bytes, segments, colours, with
and without compaction.  Beside the model: closed manifolds have E = 3 F / 2 and two faces on every edge, a grid's boundary is its
perimeter, a cube's silhouette has even degree at every vertex, an eye on a face's plane does not see it, a dot product equal to
crease_cos is no crease, NaN positions and zero-area faces get the codes the header gives them; every refusal of the header's list."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_cases as EC
import edge_model as M
from tinyrenderder_amd import api

H = api.MEM_HOST
ALL = M.ANY | M.BOUNDARY | M.SILHOUETTE | M.CREASE
MASKS = [M.ANY, M.BOUNDARY, M.SILHOUETTE, M.CREASE, M.SILHOUETTE | M.CREASE, M.BOUNDARY | M.CREASE, ALL, 0]


def _params(eye, crease_cos=0.5, select=ALL, compact=False, colors=EC.CLASS_COLORS):
    return api.make_edge_params(eye, crease_cos, select, colors, compact)


def _raw_edges(idx, nv, n_faces=None, mem=H, out="alloc", count=True, idx_ptr="given"):
    L = api.load_library()
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    F = idx.shape[0] if n_faces is None else n_faces
    buf = np.full((3 * idx.shape[0] + 2, 4), EC.SENTINEL_U32, np.uint32)
    n = C.c_uint64(12345)
    rc = L.trgl_mesh_edges(None, idx.ctypes.data if idx_ptr == "given" else idx_ptr, F, nv, mem, buf.ctypes.data if out == "alloc" else out,
                           C.byref(n) if count else None)
    return rc, buf, n.value


def _raw_select(P, v, idx, rec, n_edges=None, mem=H, stride=None, nv=None, n_faces=None, outs=(True, True, True), count=True, ptrs=None):
    L = api.load_library()
    v = np.ascontiguousarray(v, np.float64)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 4)
    n = rec.shape[0] if n_edges is None else n_edges
    codes = np.full(rec.shape[0] + 3, EC.SENTINEL_U8, np.uint8)
    seg = np.full((rec.shape[0] + 2, 2), EC.SENTINEL_U32, np.uint32)
    col = np.full(rec.shape[0] + 2, EC.SENTINEL_U32, np.uint32)
    nsel = C.c_uint64(12345)
    a = dict(vertices=v.ctypes.data, indices=idx.ctypes.data, edges=rec.ctypes.data, codes=codes.ctypes.data if outs[0] else None,
             segments=seg.ctypes.data if outs[1] else None, colors=col.ctypes.data if outs[2] else None)
    a.update(ptrs or {})
    rc = L.trgl_edge_select(None, None if P is None else C.byref(P), a["vertices"], v.shape[1] if stride is None else stride,
                            v.shape[0] if nv is None else nv, a["indices"], idx.shape[0] if n_faces is None else n_faces, a["edges"], n, mem,
                            a["codes"], a["segments"], a["colors"], C.byref(nsel) if count else None)
    return rc, codes, seg, col, nsel.value


@pytest.fixture(scope="module")
def meshes():
    return EC.named()


# ---- trgl_mesh_edges against the model ------------------------------------------------------------------------------------------------
def test_host_edges_equal_the_model_records_fill_and_count(meshes):
    cases = dict(meshes)
    cases["soup_top"] = EC.soup(30, EC.TOP, 5, with_vertices=False)
    for name, (_, idx, nv) in cases.items():
        want, E = M.edges(idx, nv)
        rc, buf, n = _raw_edges(idx, nv)
        assert rc == 0 and n == E, name
        assert np.array_equal(buf[:3 * idx.shape[0]], want), name
        assert (buf[3 * idx.shape[0]:] == EC.SENTINEL_U32).all(), f"{name}: words behind the capacity were written"
        got, n2 = api.mesh_edges(idx, nv)
        assert n2 == E and np.array_equal(got, want), name
        assert (want[:E, 0] < want[:E, 1]).all() and (want[E:] == M.NONE).all()
        pairs = [(int(lo), int(hi)) for lo, hi in want[:E, :2]]
        assert all(a < b for a, b in zip(pairs, pairs[1:])), f"{name}: edges do not ascend in (lo, hi)"


def test_the_first_two_half_edges_count_and_a_twice_named_vertex_makes_no_edge(meshes):
    rec, E = api.mesh_edges(meshes["fan"][1], 5)
    assert rec[0].tolist() == [0, 1, 0, 1], "the third face on edge (0, 1) must be ignored"
    rec, E = api.mesh_edges(meshes["twice_named"][1], 5)
    by_pair = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in rec[:E]}
    assert by_pair[(2, 3)] == (1, 1), "face (2, 2, 3) names the pair (2, 3) twice"
    assert by_pair[(0, 1)] == (0, 4) and (4, 4) not in by_pair and not any(4 in p for p in by_pair)
    rec, E = api.mesh_edges(meshes["duplicated"][1], 4)
    assert E == 6 and (rec[:E, 3] != M.NONE).all()


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "icosphere"])
def test_closed_manifolds_have_three_halves_of_their_faces_as_edges(name, meshes):
    _, idx, nv = meshes[name]
    rec, E = api.mesh_edges(idx, nv)
    assert 2 * E == 3 * idx.shape[0] and (rec[:E, 3] != M.NONE).all() and (rec[:E, 2] < rec[:E, 3]).all()
    assert nv - E + idx.shape[0] == 2, "Euler's formula"


def test_a_grids_boundary_is_its_perimeter():
    for m, n in ((7, 4), (1, 1), (12, 3)):
        v, idx, nv = EC.grid(m, n)
        rec, E = api.mesh_edges(idx, nv)
        assert E == 3 * m * n + m + n
        codes, seg, _, k = api.edge_select(_params((0.3, 0.2, 9.0, 1.0), select=M.BOUNDARY), v, idx, rec, E)
        assert k == 2 * (m + n) and int((rec[:E, 3] == M.NONE).sum()) == k
        on_rim = lambda p: (p % (m + 1) in (0, m)) or (p // (m + 1) in (0, n))
        assert all(on_rim(int(a)) and on_rim(int(b)) for a, b in seg[codes & M.BOUNDARY != 0])


# ---- trgl_edge_select against the model -----------------------------------------------------------------------------------------------
def test_host_selection_equals_the_model(meshes):
    k = 0
    for name, (v, idx, nv) in meshes.items():
        rec, E = M.edges(idx, nv)
        for eye in EC.EYES:
            for n_edges in (E, rec.shape[0]):
                mask, compact, cc = MASKS[k % len(MASKS)], bool(k % 2), (0.5, -0.25, 0.999, 2.0)[k % 4]
                k += 1
                want = M.select(rec[:n_edges], v, idx, eye, cc, mask, EC.CLASS_COLORS, compact)
                rc, codes, seg, col, nsel = _raw_select(_params(eye, cc, mask, compact), v, idx, rec[:n_edges])
                what = f"{name} eye={eye} n={n_edges} mask={mask} compact={compact}"
                assert rc == 0 and nsel == want[3], what
                assert np.array_equal(codes[:n_edges], want[0]) and np.array_equal(seg[:n_edges], want[1]) and np.array_equal(col[:n_edges], want[2]), what
                assert (codes[n_edges:] == EC.SENTINEL_U8).all() and (seg[n_edges:] == EC.SENTINEL_U32).all() and (col[n_edges:] == EC.SENTINEL_U32).all(), what


def test_compaction_keeps_record_order_and_fills_the_tail(meshes):
    v, idx, nv = meshes["icosphere"]
    rec, E = api.mesh_edges(idx, nv)
    P = dict(eye=(3.0, 2.0, 5.0, 1.0), crease_cos=0.99, select=M.SILHOUETTE | M.CREASE)
    codes, seg, col, n = api.edge_select(_params(**P), v, idx, rec)
    c_codes, c_seg, c_col, c_n = api.edge_select(_params(compact=True, **P), v, idx, rec)
    chosen = codes & (M.SILHOUETTE | M.CREASE) != 0
    assert 0 < n == c_n == chosen.sum() < E and np.array_equal(codes, c_codes)
    assert np.array_equal(c_seg[:n], rec[chosen][:, :2]) and (c_seg[n:] == M.NONE).all() and (c_col[n:] == 0).all()
    assert np.array_equal(c_col[:n], col[chosen])
    assert set(np.unique(c_col[:n]).tolist()) <= {EC.CLASS_COLORS[2], EC.CLASS_COLORS[3]}
    # each output may be left out; the count still comes
    rc, codes2, seg2, col2, nsel = _raw_select(_params(compact=True, **P), v, idx, rec, outs=(False, False, False))
    assert rc == 0 and nsel == n and (codes2 == EC.SENTINEL_U8).all() and (seg2 == EC.SENTINEL_U32).all() and (col2 == EC.SENTINEL_U32).all()


def test_a_cube_seen_from_outside_has_a_silhouette_of_even_degree():
    v, idx, nv = EC.cube()
    rec, E = api.mesh_edges(idx, nv)
    for eye in ((3.0, 2.0, 5.0, 1.0), (-4.0, 0.5, 0.25, 1.0), (0.2, 0.9, -0.4, 0.0), (0.0, 0.0, 7.0, 1.0)):
        codes, seg, _, n = api.edge_select(_params(eye, select=M.SILHOUETTE, compact=True), v, idx, rec, E)
        degree = np.bincount(seg[:n].reshape(-1), minlength=8)
        assert n >= 4 and (degree % 2 == 0).all(), (eye, degree)
    # from inside, every face looks away: no silhouette, and no face is front
    codes, _, _, n = api.edge_select(_params((0.1, -0.2, 0.05, 1.0), select=M.SILHOUETTE), v, idx, rec, E)
    assert n == 0 and (codes[:E] & M.ANY).all()
    assert not any(M.face(v, idx[f], (0.1, -0.2, 0.05, 1.0))[0] for f in range(12)), "the cube's faces must wind outward"


def test_an_eye_on_a_faces_plane_does_not_see_it():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, -1]], np.float64)
    idx = np.array([[0, 1, 2], [1, 0, 3]], np.uint32)
    rec, E = api.mesh_edges(idx, 4)
    shared = int(np.flatnonzero((rec[:E, 0] == 0) & (rec[:E, 1] == 1))[0])
    on_plane = api.edge_select(_params((5.0, -5.0, 0.0, 1.0), -2.0), v, idx, rec, E)[0]
    above = api.edge_select(_params((5.0, -5.0, 2.0 ** -40, 1.0), -2.0), v, idx, rec, E)[0]
    assert on_plane[shared] == M.ANY | M.SILHOUETTE, "s == 0 is not front, the other face is"
    assert above[shared] == M.ANY


def test_a_dot_product_equal_to_crease_cos_is_no_crease(meshes):
    v, idx, nv = meshes["grid"]
    rec, E = api.mesh_edges(idx, nv)
    eye = (0.0, 0.0, 50.0, 1.0)
    inner = [i for i in range(E) if rec[i, 3] != M.NONE]
    seen = 0
    for i in inner[::5]:
        u0, u1 = M.face(v, idx[rec[i, 2]], eye)[1], M.face(v, idx[rec[i, 3]], eye)[1]
        dot = 0.0
        for a in range(3):
            dot = dot + u0[a] * u1[a]
        at = api.edge_select(_params(eye, dot), v, idx, rec, E)[0][i]
        over = api.edge_select(_params(eye, math.nextafter(dot, 2.0)), v, idx, rec, E)[0][i]
        assert not at & M.CREASE and over & M.CREASE, (i, dot)
        seen += 1
    assert seen >= 10


def test_nan_positions_and_zero_area_faces_get_the_headers_codes():
    v, idx, nv = EC.grid(3, 2, bump=0.3)
    v = v.copy()
    v[5, 1] = np.nan                                                  # an inner vertex: six faces around it
    idx = np.concatenate([idx, np.array([[0, 1, 1], [0, 4, 8]], np.uint32)])       # (0, 1, 1) names a vertex twice; (0, 4, 8) is made collinear below
    v[[0, 4, 8], 2] = 0.0
    v[8, :2] = 2 * v[4, :2] - v[0, :2]                                # 0, 4, 8 on one line: zero area
    rec, E = api.mesh_edges(idx, nv)
    eye = (1.0, 1.0, 30.0, 1.0)
    seen_nan = seen_flat = 0
    for cc in (0.5, -0.5, 0.0):
        codes = api.edge_select(_params(eye, cc), v, idx, rec, E)[0]
        want = M.select(rec[:E], v, idx, eye, cc, ALL)[0]
        assert np.array_equal(codes, want)
        for i in range(E):
            faces = [int(f) for f in rec[i, 2:] if f != M.NONE]
            if len(faces) == 2 and any(5 in idx[f] for f in faces):
                other_front = [M.face(v, idx[f], eye)[0] for f in faces if 5 not in idx[f]]
                assert not codes[i] & M.CREASE, "a NaN dot product is no crease"
                assert bool(codes[i] & M.SILHOUETTE) == (len(other_front) == 1 and other_front[0]), "a NaN face is not front"
                seen_nan += 1
            if len(faces) == 2 and idx.shape[0] - 1 in faces and not any(5 in idx[f] for f in faces):
                assert bool(codes[i] & M.CREASE) == (0.0 < cc), "a zero-area face has the normal 0: the dot product is 0"
                seen_flat += 1
    assert seen_nan >= 3 * 6 and seen_flat >= 3


# ---- refusals and empty calls -----------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_header_and_nothing_is_written(meshes):
    v, idx, nv = meshes["cube"]
    rec, E = api.mesh_edges(idx, nv)
    bad_idx = idx.copy(); bad_idx[7, 2] = nv
    INVALID, UNSUPPORTED = -1, -5
    edges = dict(
        bad_mem_kind=(_raw_edges(idx, nv, mem=7), INVALID), device_without_context=(_raw_edges(idx, nv, mem=api.MEM_DEVICE), INVALID),
        index_out_of_range=(_raw_edges(bad_idx, nv), INVALID), too_many_vertices=(_raw_edges(idx, 2 ** 32), INVALID),
        null_indices=(_raw_edges(idx, nv, idx_ptr=None), INVALID), null_output=(_raw_edges(idx, nv, out=None), INVALID),
        misaligned_output=(_raw_edges(idx, nv, out=np.zeros(200, np.uint32).ctypes.data + 2), INVALID),
        overlap=(_raw_edges(idx, nv, out=idx.ctypes.data + 4), INVALID), too_many_faces=(_raw_edges(idx, nv, n_faces=(2 ** 31 - 1) // 3 + 1), UNSUPPORTED))
    for name, ((rc, buf, n), want) in edges.items():
        assert rc == want, name
        assert (buf == EC.SENTINEL_U32).all() and n == 12345, f"{name}: a refused call wrote something"
        assert api.load_library().trgl_last_error(None).decode().startswith("trgl_mesh_edges: "), name

    P = _params((3.0, 2.0, 5.0, 1.0))
    bad_rec = rec.copy(); bad_rec[3, 3] = idx.shape[0]
    bad_rec0 = rec.copy(); bad_rec0[E - 1, 2] = 0xFFFFFFFE
    reserved = _params((3.0, 2.0, 5.0, 1.0)); reserved.reserved = 1
    other = np.zeros(64, np.uint32)
    sel = dict(
        null_params=(_raw_select(None, v, idx, rec), INVALID), bad_mem_kind=(_raw_select(P, v, idx, rec, mem=2), INVALID),
        device_without_context=(_raw_select(P, v, idx, rec, mem=api.MEM_DEVICE), INVALID),
        unknown_select_bit=(_raw_select(_params((0, 0, 1, 0), select=16), v, idx, rec), INVALID), reserved=(_raw_select(reserved, v, idx, rec), INVALID),
        small_stride=(_raw_select(P, v, idx, rec, stride=2), INVALID), too_many_edges=(_raw_select(P, v, idx, rec, n_edges=3 * idx.shape[0] + 1), INVALID),
        too_many_vertices=(_raw_select(P, v, idx, rec, nv=2 ** 32), INVALID), too_many_faces=(_raw_select(P, v, idx, rec, n_faces=(2 ** 31 - 1) // 3 + 1), UNSUPPORTED),
        null_vertices=(_raw_select(P, v, idx, rec, ptrs=dict(vertices=None)), INVALID), null_edges=(_raw_select(P, v, idx, rec, ptrs=dict(edges=None)), INVALID),
        misaligned_vertices=(_raw_select(P, v, idx, rec, ptrs=dict(vertices=v.ctypes.data + 4)), INVALID),
        misaligned_segments=(_raw_select(P, v, idx, rec, ptrs=dict(segments=other.ctypes.data + 2)), INVALID),
        output_over_input=(_raw_select(P, v, idx, rec, ptrs=dict(colors=rec.ctypes.data + 16)), INVALID),
        outputs_overlap=(_raw_select(P, v, idx, rec, ptrs=dict(colors=other.ctypes.data, segments=other.ctypes.data + 8)), INVALID),
        face_out_of_range=(_raw_select(P, v, idx, bad_rec), INVALID), first_face_out_of_range=(_raw_select(P, v, idx, bad_rec0), INVALID),
        vertex_out_of_range=(_raw_select(P, v, bad_idx, rec), INVALID))
    for name, ((rc, codes, seg, col, nsel), want) in sel.items():
        assert rc == want, name
        assert (codes == EC.SENTINEL_U8).all() and (seg == EC.SENTINEL_U32).all() and (col == EC.SENTINEL_U32).all() and nsel == 12345, name
        assert api.load_library().trgl_last_error(None).decode().startswith("trgl_edge_select: "), name
    assert (other == 0).all() and np.array_equal(rec, api.mesh_edges(idx, nv)[0])
    with pytest.raises(M.OutOfRange):
        M.edges(bad_idx, nv)
    with pytest.raises(M.OutOfRange):
        M.select(bad_rec, v, idx, (3.0, 2.0, 5.0, 1.0), 0.5, ALL)


def test_empty_calls_touch_no_array():
    L = api.load_library()
    n = C.c_uint64(99)
    assert L.trgl_mesh_edges(None, None, 0, 8, H, None, C.byref(n)) == 0 and n.value == 0
    assert L.trgl_mesh_edges(None, None, 0, 0, H, None, None) == 0
    P = _params((0, 0, 1, 0), compact=True)
    n = C.c_uint64(99)
    assert L.trgl_edge_select(None, C.byref(P), None, 3, 0, None, 0, None, 0, H, None, None, None, C.byref(n)) == 0 and n.value == 0
    assert L.trgl_edge_select(None, C.byref(P), None, 3, 8, None, 12, None, 0, H, None, None, None, None) == 0
    rec, E = api.mesh_edges(np.zeros((0, 3), np.uint32), 5)
    assert rec.shape == (0, 4) and E == 0


def test_params_struct_matches_the_header():
    assert C.sizeof(api.EdgeParams) == 4 * 8 + 8 + 4 * 4 + 4 + 4 + 8
    assert (api.EDGE_ANY, api.EDGE_BOUNDARY, api.EDGE_SILHOUETTE, api.EDGE_CREASE, api.EDGE_NONE) == (M.ANY, M.BOUNDARY, M.SILHOUETTE, M.CREASE, M.NONE)
