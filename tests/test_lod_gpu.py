"""Mesh levels of detail on the GPU (include/trgl.h: trgl_mesh_clean, trgl_mesh_simplify; kernels_lod.hip).

What the two calls write in device memory equals the host twins - themselves held to tests/lod_model.py - bit for bit: at face and
vertex counts around a wave, a block and the lower level of the scan, from no duplicate and no degenerate face to all, at 200 000 faces,
with the face hash cut down to 3, 1 and 0 bits - which the model shows to put different triples into one run -, every array at every
alignment its type allows; guard words behind every capacity stay intact and the inputs unchanged; a device index out of range drops
its face.  Two levels queued without a count over the capacities equal the host chain that passes real counts; weld, simplify and edges
queue the same way; a simplified sphere draws the same frame from device-made and host-made arrays, and with fill ZERO over the capacity
the frame of exactly the kept faces."""
import numpy as np
import pytest

import cases
import lod_cases as LC
import lod_model as M
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, PHONG, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
NONE = M.NONE
WAVE, BLOCK, SCAN_CHUNK = 64, 256, 256       # lanes of a wave and of a block (LOD_BLOCK), block counts per lower-level scan block (INST_SCAN_CHUNK)
SIZES = [1, 2, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * SCAN_CHUNK, BLOCK * SCAN_CHUNK + 1]
BIG = 200_003
S32, S64 = LC.SENTINEL_U32, LC.SENTINEL_F64
BOTH = api.CLEAN_DUPLICATES | api.CLEAN_VERTICES


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a, off=0):
    return None if a is None else cases.device_array(np.ascontiguousarray(a), off)


def _sync():
    import torch
    torch.cuda.synchronize()                 # uploads run on torch's stream; a context's own stream is not ordered behind it


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.fixture(scope="module")
def ctx64():
    with Context(64, 64, 3) as ctx:
        yield ctx


def fast_faces(F, V, dup, degen, seed):
    """LC.seeded_faces without its loop, for the large counts: fresh triples a != b != c over V >= 3 vertices, about F * dup of them then
    overwritten by a rotation of an earlier face and about F * degen by a face with two equal indices."""
    r = scenes.SplitMix64(seed).u64(6 * F).reshape(F, 6)
    a = (r[:, 0] % np.uint64(V)).astype(np.int64)
    b = (a + 1 + (r[:, 1] % np.uint64(V - 1)).astype(np.int64)) % V
    c = (r[:, 2] % np.uint64(V)).astype(np.int64)
    for _ in range(2):
        c = np.where((c == a) | (c == b), (c + 1) % V, c)
    f = np.stack([a, b, c], 1)
    src = (r[:, 3] % np.uint64(F)).astype(np.int64) % np.maximum(np.arange(F), 1)        # an earlier face (face 0 for face 0)
    is_dup = ((r[:, 4] % np.uint64(1000)).astype(np.float64) < 1000.0 * dup) & (np.arange(F) > 0)
    f = np.where(is_dup[:, None], np.roll(f[src], 1, axis=1), f)                           # (one level: a copy of a face as first drawn)
    is_deg = (r[:, 5] % np.uint64(1000)).astype(np.float64) < 1000.0 * degen
    f = np.where(is_deg[:, None], np.stack([f[:, 0], f[:, 0], f[:, 2]], 1), f)
    return np.ascontiguousarray(f.astype(np.uint32))


_wanted = {}


def _want_clean(name, idx, V, flags, fill, v):
    """The expected outputs of a named clean, made once: the host twin's - with an index out of range the model's, which the host twin
    refuses -, checked against the model wherever the model is quick."""
    key = (name, flags, fill)
    if key not in _wanted:
        bad = bool((idx >= V).any())
        model = M.clean(idx, V, flags, fill, v, device=True) if bad or idx.shape[0] <= 70_000 or name.startswith("big") else None
        if bad:
            want = model
        else:
            out, counts = api.mesh_clean(api.make_clean_params(0 if v is None else v.shape[1], flags, fill), idx, v, V)
            want = dict(out, counts=counts)
            if model is not None:
                assert counts == model["counts"]
                for k in api.CLEAN_OUTPUTS:
                    assert (want[k] is None and model[k] is None) or np.array_equal(np.ascontiguousarray(want[k]).view(np.uint32),
                                                                                    np.ascontiguousarray(model[k]).view(np.uint32)), f"{name}: host twin and model differ in {k}"
        _wanted[key] = want
    return _wanted[key]


def _compare(what, names, want, guard, out, sizes):
    for k in names:
        flat = _host(guard[k]).reshape(-1)
        flat = flat.view(np.uint64) if k == "vertices" else flat
        sentinel = _bits(np.array([S64]))[0] if k == "vertices" else S32
        assert (flat[sizes[k]:] == sentinel).all(), f"{what}: words behind the capacity of {k} were written"
        if k not in out:
            assert (flat == sentinel).all(), f"{what}: {k} was not asked for and was written"
            continue
        w = _bits(want[k]).reshape(-1) if k == "vertices" else np.ascontiguousarray(want[k]).reshape(-1)
        bad = np.argwhere(flat[:sizes[k]] != w)
        assert bad.size == 0, f"{what}: {bad.shape[0]} words of {k} differ, first at {bad[:4].reshape(-1).tolist()}"


def _check_clean(ctx, name, idx, V, v=None, flags=BOTH, fill=api.CLEAN_FILL_NONE, offs=(0, 0, 0, 0, 0, 0, 0), count=True, outputs=None):
    """trgl_mesh_clean over device arrays at the byte offsets offs = (indices, vertices, indices out, face_firsts, vremap, vfirsts,
    records), with guard words behind every capacity, against _want_clean()."""
    F = idx.shape[0]
    S = 0 if v is None else v.shape[1]
    want = _want_clean(name, idx, V, flags, fill, v)
    names = [k for k in api.CLEAN_OUTPUTS if (flags & api.CLEAN_VERTICES or k in ("indices", "face_firsts")) and (k != "vertices" or v is not None)]
    d_idx, d_v = _dev(idx, offs[0]), _dev(v, offs[1])
    guard = dict(indices=_dev(np.full(3 * F + 3, S32, np.uint32), offs[2]), face_firsts=_dev(np.full(F + 3, S32, np.uint32), offs[3]),
                 vremap=_dev(np.full(V + 3, S32, np.uint32), offs[4]), vfirsts=_dev(np.full(V + 3, S32, np.uint32), offs[5]),
                 vertices=_dev(np.full(V * S + 3, S64), offs[6]))
    views = dict(indices=guard["indices"][:3 * F].view(F, 3), face_firsts=guard["face_firsts"][:F], vremap=guard["vremap"][:V], vfirsts=guard["vfirsts"][:V],
                 vertices=guard["vertices"][:V * S].view(V, S) if S else None)
    out = {k: views[k] for k in (names if outputs is None else outputs)}
    _sync()
    _, counts = ctx.mesh_clean(api.make_clean_params(S, flags, fill), d_idx, d_v, V, device=True, out=out, count=count)
    ctx.sync()
    what = f"{name}: F={F} V={V} stride={S} flags={flags} fill={fill} offsets {offs}"
    assert counts == (want["counts"] if count else None), f"{what}: counts {counts}, expected {want['counts']}"
    _compare(what, api.CLEAN_OUTPUTS, want, guard, out, dict(indices=3 * F, face_firsts=F, vremap=V, vfirsts=V, vertices=V * S))
    assert np.array_equal(_host(d_idx), idx) and (v is None or np.array_equal(_bits(_host(d_v)), _bits(v))), f"{what}: an input was written to"
    return want


def _want_simplify(name, v, idx, cell, mean_count, fill):
    key = (name, cell, mean_count, fill)
    if key not in _wanted:
        bad = bool((idx >= v.shape[0]).any())
        model = M.simplify(v, idx, cell, mean_count, fill, device=True) if bad or v.shape[0] + idx.shape[0] <= 20_000 else None
        if bad:
            want = model
        else:
            out, counts = api.mesh_simplify(api.make_simplify_params(v.shape[1], cell, mean_count, fill), v, idx)
            want = dict(out, counts=counts)
            if model is not None:
                assert counts == model["counts"]
                for k in api.SIMPLIFY_OUTPUTS:
                    assert np.array_equal(np.ascontiguousarray(want[k]).view(np.uint32), np.ascontiguousarray(model[k]).view(np.uint32)), \
                        f"{name}: host twin and model differ in {k}"
        _wanted[key] = want
    return _wanted[key]


def _check_simplify(ctx, name, v, idx, cell, mean_count=3, fill=api.CLEAN_FILL_NONE, offs=(0, 0, 0, 0, 0, 0, 0), count=True, outputs=api.SIMPLIFY_OUTPUTS):
    """trgl_mesh_simplify over device arrays at the byte offsets offs = (vertices, indices, remap, firsts, records, indices out,
    face_firsts), with guard words behind every capacity, against the host twin."""
    n, S = v.shape
    F = idx.shape[0]
    want = _want_simplify(name, v, idx, cell, mean_count, fill)
    d_v, d_idx = _dev(v, offs[0]), _dev(idx, offs[1])
    guard = dict(remap=_dev(np.full(n + 3, S32, np.uint32), offs[2]), firsts=_dev(np.full(n + 3, S32, np.uint32), offs[3]),
                 vertices=_dev(np.full(n * S + 3, S64), offs[4]), indices=_dev(np.full(3 * F + 3, S32, np.uint32), offs[5]),
                 face_firsts=_dev(np.full(F + 3, S32, np.uint32), offs[6]))
    views = dict(remap=guard["remap"][:n], firsts=guard["firsts"][:n], vertices=guard["vertices"][:n * S].view(n, S),
                 indices=guard["indices"][:3 * F].view(F, 3), face_firsts=guard["face_firsts"][:F])
    out = {k: views[k] for k in outputs}
    _sync()
    _, counts = ctx.mesh_simplify(api.make_simplify_params(S, cell, mean_count, fill), d_v, d_idx, device=True, out=out, count=count)
    ctx.sync()
    what = f"{name}: n={n} F={F} stride={S} cell={cell} mean_count={mean_count} offsets {offs}"
    assert counts == (want["counts"] if count else None), f"{what}: counts {counts}, expected {want['counts']}"
    _compare(what, api.SIMPLIFY_OUTPUTS, want, guard, out, dict(remap=n, firsts=n, vertices=n * S, indices=3 * F, face_firsts=F))
    assert np.array_equal(_bits(_host(d_v)), _bits(v)) and np.array_equal(_host(d_idx), idx), f"{what}: an input was written to"
    return want


def _positions(n, stride, spread, seed):
    v = LC.records(n, stride, seed)
    v[:, :3] = scenes.SplitMix64(seed + 1).uniform(3 * n, -spread, spread).reshape(n, 3)
    return np.ascontiguousarray(v)


# ---- counts and rates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", [(0.0, 0.0), (0.4, 0.2), (1.0, 0.0), (0.0, 1.0)], ids=["none", "some", "all duplicates", "all degenerate"])
def test_every_count_at_the_edges_of_the_machinery(rates, ctx64):
    dup, degen = rates
    n = (api.C.c_uint64 * 2)(7, 7)
    P = api.make_clean_params(3)
    assert ctx64.L.trgl_mesh_clean(ctx64.h, api.C.byref(P), None, 0, None, 0, api.MEM_DEVICE, None, None, None, None, None, n) == 0 and (n[0], n[1]) == (0, 0)
    for k, F in enumerate(SIZES):
        V = max(3, SIZES[(k + 3) % len(SIZES)])                          # face and vertex counts both visit every size
        stride = (3, 5, 8, 14)[k % 4] if V < 10_000 else 3
        idx = fast_faces(F, V, dup, degen, 40 + k)
        v = LC.records(V, stride, k)
        want = _check_clean(ctx64, f"count{F}/{rates}", idx, V, v, fill=k % 2,
                            offs=(4 * (k % 4), 8 * (k % 2), 4 * ((k + 1) % 4), 4 * ((k + 2) % 4), 4 * ((k + 3) % 4), 4 * (k % 4), 8 * ((k + 1) % 2)))
        # ... and the simplification over the same faces and as many vertices: the weld, the mean and the composed maps at every size
        w = _positions(V, stride, 3.0, 70 + k)
        _check_simplify(ctx64, f"count{F}/{rates}", w, idx, 0.5 if k % 2 else 0.0, mean_count=(3, 0, stride)[k % 3], fill=k % 2,
                        offs=(8 * (k % 2), 4 * (k % 4), 4 * ((k + 1) % 4), 4 * ((k + 2) % 4), 8 * ((k + 1) % 2), 4 * ((k + 3) % 4), 4 * (k % 4)))
        K, U = want["counts"]
        if degen == 1.0:
            assert (K, U) == (0, 0)
        elif dup == 0.0 and degen == 0.0 and V >= 60_000:
            assert K >= F - F // 100
        elif dup == 1.0:
            assert K < F or F < 2, "face 1 repeats face 0"
    assert BLOCK * SCAN_CHUNK in SIZES and BLOCK * SCAN_CHUNK + 1 in SIZES, "the second level of the scan starts behind 65 536 entries"
    # no face at all: every vertex leaves
    empty = np.zeros((0, 3), np.uint32)
    for V in (1, BLOCK + 1):
        want = _check_clean(ctx64, f"no faces/{V}", empty, V, LC.records(V, 3, 1))
        assert want["counts"] == (0, 0)
        assert _check_simplify(ctx64, f"no faces/{V}", _positions(V, 3, 3.0, 1), empty, 0.5)["counts"] == (0, 0)
    _check_clean(ctx64, "no faces, old numbers", empty, 5, flags=api.CLEAN_DUPLICATES)
    # one and two vertices: no face over them has three distinct indices
    for V in (1, 2):
        idx = (scenes.SplitMix64(V).u64(3 * 70) % np.uint64(V)).astype(np.uint32).reshape(-1, 3)
        assert _check_clean(ctx64, f"few vertices/{V}", idx, V, LC.records(V, 3, V))["counts"] == (0, 0)
        assert _check_simplify(ctx64, f"few vertices/{V}", _positions(V, 3, 3.0, V), idx, 0.5)["counts"] == (0, 0)


@pytest.mark.parametrize("rates", [(0.0, 0.0), (0.5, 0.25), (1.0, 0.0)], ids=["none", "some", "all duplicates"])
def test_two_hundred_thousand_faces(rates, ctx64):
    idx = fast_faces(BIG, 70_001, rates[0], rates[1], 7)
    v = LC.records(70_001, 5, 7)
    want = _check_clean(ctx64, f"big/{rates}", idx, 70_001, v, offs=(4, 8, 12, 8, 4, 12, 8))
    assert rates != (0.5, 0.25) or 0.2 * BIG < want["counts"][0] < 0.6 * BIG
    _check_clean(ctx64, f"big/{rates}", idx, 70_001, None, flags=api.CLEAN_DUPLICATES, fill=api.CLEAN_FILL_ZERO, offs=(8, 0, 4, 12, 0, 0, 0))
    if rates[0] == 0.5:
        w = _positions(70_001, 4, 3.0, 9)
        want = _check_simplify(ctx64, "big", w, idx, 0.25, offs=(8, 4, 12, 8, 8, 4, 0))
        assert 1000 < want["counts"][1] < 20_000 and want["counts"][0] > 1000


# ---- the hash cut down ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.COLLISION_CASES, ids=lambda c: f"F{c[0]}")
def test_outputs_do_not_change_with_the_hash_bits(case, ctx64):
    F, V, dup, degen, seed = case
    idx = LC.seeded_faces(F, V, dup, degen, seed)
    v = _positions(V, 5, 2.0, seed)
    try:
        for bits in (64, 3, 1, 0, 17):
            ctx64.debug_lod_hash_bits(bits)
            _check_clean(ctx64, f"bits/{seed}", idx, V, v, offs=(4, 0, 8, 12, 4, 0, 8))
            _check_simplify(ctx64, f"bits/{seed}", v, idx, 0.5, offs=(0, 4, 8, 12, 8, 0, 4))
            if bits in (3, 1, 0):
                mixed, walked = LC.collision_proof(idx, V, bits)
                assert mixed >= 1, f"{bits} bits: no run holds several distinct triples"
                assert dup == 0.0 or walked > 0, f"{bits} bits: no duplicate behind a run's head"
        ctx64.debug_lod_hash_bits(0)                                     # the sizes around a wave and a block in one run each
        for m in [1, 2, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1]:
            if m <= F:
                _check_clean(ctx64, f"bits0/{seed}/{m}", np.ascontiguousarray(idx[:m]), V, v)
        ctx64.debug_weld_hash_bits(2)                                    # ... and the weld's runs mixed: the mean walks past other clusters
        ctx64.debug_lod_hash_bits(2)
        _check_simplify(ctx64, f"bits/{seed}", v, idx, 0.5, offs=(8, 0, 4, 4, 0, 0, 0))
        with pytest.raises(api.TrglError, match="trgl_debug_lod_hash_bits"):
            ctx64.debug_lod_hash_bits(65)
    finally:
        ctx64.debug_lod_hash_bits(64)
        ctx64.debug_weld_hash_bits(64)


# ---- alignment, flags, outputs left out ---------------------------------------------------------------------------------------------------
def test_arrays_at_every_alignment(ctx64):
    idx = LC.seeded_faces(777, 300, 0.3, 0.1, 11)                        # 777 faces: a block's piece of the triples starts at every word of a 16-byte line
    v = _positions(300, 5, 2.0, 11)                                      # an odd stride: a block's piece of the records starts at either parity
    for which in range(7):                                                # one array moves at a time
        for off in ((0, 8) if which in (1, 6) else (0, 4, 8, 12)):
            offs = [0] * 7
            offs[which] = off
            _check_clean(ctx64, "alignment", idx, 300, v, offs=tuple(offs))
    for which in range(7):
        for off in ((0, 8) if which in (0, 4) else (0, 4, 8, 12)):
            offs = [0] * 7
            offs[which] = off
            _check_simplify(ctx64, "alignment", v, idx, 0.75, offs=tuple(offs))
    for off8 in (0, 8):
        for off4 in (4, 8, 12):
            _check_clean(ctx64, "alignment", idx, 300, v, fill=api.CLEAN_FILL_ZERO, offs=(off4, off8, (off4 + 4) % 16, (off4 + 8) % 16, off4, (off4 + 12) % 16, 8 - off8))
            _check_simplify(ctx64, "alignment", v, idx, 0.75, mean_count=5, offs=(off8, off4, (off4 + 4) % 16, (off4 + 8) % 16, 8 - off8, off4, (off4 + 12) % 16))


def test_every_flag_stride_and_output_left_out(ctx64):
    idx = LC.seeded_faces(600, 250, 0.3, 0.15, 21)
    for stride in (3, 8, 14):
        v = _positions(250, stride, 2.0, stride)
        for flags in (0, api.CLEAN_DUPLICATES, api.CLEAN_VERTICES, BOTH):
            for fill in (api.CLEAN_FILL_NONE, api.CLEAN_FILL_ZERO):
                _check_clean(ctx64, f"flags/{stride}", idx, 250, v if flags & api.CLEAN_VERTICES else None, flags=flags, fill=fill)
        for mean_count in (0, 1, 3, stride):
            _check_simplify(ctx64, f"flags/{stride}", v, idx, 0.5, mean_count=mean_count, fill=mean_count % 2)
    v = _positions(250, 8, 2.0, 8)
    for left_out in api.CLEAN_OUTPUTS:
        _check_clean(ctx64, "flags/8", idx, 250, v, outputs=[k for k in api.CLEAN_OUTPUTS if k != left_out], count=left_out != "vfirsts")
    _check_clean(ctx64, "flags/8", idx, 250, v, outputs=["indices"], count=False)       # (the vertex map then lives in scratch)
    _check_clean(ctx64, "no records", idx, 250, None, outputs=["indices", "vremap"])
    for left_out in api.SIMPLIFY_OUTPUTS:
        _check_simplify(ctx64, "flags/8", v, idx, 0.5, outputs=[k for k in api.SIMPLIFY_OUTPUTS if k != left_out], count=left_out != "firsts")
    _check_simplify(ctx64, "flags/8", v, idx, 0.5, outputs=["indices"], count=False)
    # a record wider than any tile still moves whole
    w = _positions(70, 1031, 2.0, 2)
    _check_simplify(ctx64, "wide", w, LC.seeded_faces(90, 70, 0.1, 0.1, 3), 1.0, mean_count=1031, offs=(8, 0, 0, 0, 8, 0, 0))
    d_v, d_idx = _dev(v), _dev(idx)
    with pytest.raises(api.TrglError, match="trgl_mesh_clean: an output overlaps an input"):
        ctx64.mesh_clean(api.make_clean_params(8), d_idx, d_v, device=True, out=dict(indices=d_idx))
    with pytest.raises(api.TrglError, match="trgl_mesh_simplify: an output overlaps an input"):
        ctx64.mesh_simplify(api.make_simplify_params(8, 0.5), d_v, d_idx, device=True, out=dict(vertices=d_v))
    with pytest.raises(api.TrglError, match="trgl_mesh_clean: arrays need natural alignment"):
        ctx64._chk(ctx64.L.trgl_mesh_clean(ctx64.h, api.C.byref(api.make_clean_params(8)), d_idx.data_ptr() + 2, 5, None, 250, api.MEM_DEVICE,
                                           None, None, None, None, None, None))
    with pytest.raises(api.TrglError, match="need TRGL_CLEAN_VERTICES"):
        ctx64._chk(ctx64.L.trgl_mesh_clean(ctx64.h, api.C.byref(api.make_clean_params(8, api.CLEAN_DUPLICATES)), d_idx.data_ptr(), 600, None, 250, api.MEM_DEVICE,
                                           None, None, _dev(np.zeros(250, np.uint32)).data_ptr(), None, None, None))


def test_a_device_index_out_of_range_drops_its_face_and_special_positions(ctx64):
    V = 300
    idx = LC.seeded_faces(400, V, 0.2, 0.1, 31)
    bad = idx.copy()
    bad[3, 1], bad[9, 0], bad[20, 2], bad[399] = V, NONE, V + 7, (V, 0x80000000, 5)
    bad[21] = bad[20]                                                     # the twin of an invalid face is invalid itself
    v = _positions(V, 4, 2.0, 31)
    want = _check_clean(ctx64, "bad indices", bad, V, v)
    cls = M.classes(bad, V)
    assert [cls[f] for f in (3, 9, 20, 21, 399)] == [M.INVALID] * 5 and not set(want["face_firsts"].tolist()) & {3, 9, 20, 21, 399}
    _check_clean(ctx64, "bad indices", bad, V, None, flags=0, fill=api.CLEAN_FILL_ZERO)
    _check_simplify(ctx64, "bad indices", v, bad, 0.5)
    _check_simplify(ctx64, "bad indices", v, bad, 0.0, mean_count=0)
    sv, sidx = LC.special_positions()
    for cell in (0.0, 0.5):
        for mean_count in (0, 3, 5):
            _check_simplify(ctx64, "special", sv, sidx, cell, mean_count=mean_count, offs=(8, 0, 4, 8, 0, 0, 12))
    ov, oidx = LC.octa_sphere(4, 14)
    want = _check_simplify(ctx64, "sphere, identity", ov, oidx, 0.0)
    assert want["counts"] == (oidx.shape[0], ov.shape[0])
    want = _check_simplify(ctx64, "sphere, nothing left", ov, oidx, 8.0)
    assert want["counts"] == (0, 0)


# ---- chains -------------------------------------------------------------------------------------------------------------------------------
def test_two_levels_queued_over_the_capacities_equal_the_host_chain_with_real_counts(ctx64):
    v, idx = LC.octa_sphere(5, 8)                                         # 8192 faces, 4098 vertices
    n, F = v.shape[0], idx.shape[0]
    P1, P2 = api.make_simplify_params(8, 0.1, 3), api.make_simplify_params(8, 0.2, 3)
    h1, (K1, U1) = api.mesh_simplify(P1, v, idx)
    h2, (K2, U2) = api.mesh_simplify(P2, np.ascontiguousarray(h1["vertices"][:U1]), np.ascontiguousarray(h1["indices"][:K1]))
    assert 0 < K2 < K1 < F and 0 < U2 < U1 < n
    d_v, d_idx = _dev(v, 8), _dev(idx, 4)
    _sync()
    d1, none1 = ctx64.mesh_simplify(P1, d_v, d_idx, device=True, count=False)
    d2, none2 = ctx64.mesh_simplify(P2, d1["vertices"], d1["indices"], device=True, count=False)
    ctx64.sync()
    assert none1 is None and none2 is None
    g = {k: _host(t) for k, t in d2.items()}
    assert np.array_equal(_bits(g["vertices"][:U2]), _bits(h2["vertices"][:U2])) and not _bits(g["vertices"][U2:]).any()
    assert np.array_equal(g["indices"][:K2], h2["indices"][:K2]) and (g["indices"][K2:] == NONE).all()
    assert np.array_equal(g["face_firsts"][:K2], h2["face_firsts"][:K2]) and (g["face_firsts"][K2:] == NONE).all()
    assert np.array_equal(g["firsts"][:U2], h2["firsts"][:U2]) and (g["firsts"][U2:] == NONE).all()
    assert np.array_equal(g["remap"][:U1], h2["remap"])
    assert (g["remap"][U1:] == NONE).all(), "no vertex of the sphere lies in the origin's cell: the fill records are a cluster nobody names, and it leaves"
    one = {k: _host(t) for k, t in d1.items()}
    assert np.array_equal(one["indices"][:K1], h1["indices"][:K1]) and (one["indices"][K1:] == NONE).all() and not _bits(one["vertices"][U1:]).any()


def test_zero_records_behind_a_count_do_not_pull_the_origins_mean(ctx64):
    # a mesh with vertices in the origin's cell; the first level leaves zero records behind its count, and the second runs over them
    v = _positions(500, 3, 1.0, 61)
    idx = LC.seeded_faces(900, 500, 0.1, 0.05, 62)
    P1, P2 = api.make_simplify_params(3, 0.25, 3), api.make_simplify_params(3, 1.0, 3)
    h1, (K1, U1) = api.mesh_simplify(P1, v, idx)
    h2, (K2, U2) = api.mesh_simplify(P2, np.ascontiguousarray(h1["vertices"][:U1]), np.ascontiguousarray(h1["indices"][:K1]))
    q = np.floor(h1["vertices"][:U1] / 1.0 + 0.5)
    assert U1 < 500 and ((q == 0).all(1)).sum() > 1, "several first-level vertices lie in the origin's cell, and there are fill records"
    d_v, d_idx = _dev(v), _dev(idx)
    _sync()
    d1, _ = ctx64.mesh_simplify(P1, d_v, d_idx, device=True, count=False)
    d2, _ = ctx64.mesh_simplify(P2, d1["vertices"], d1["indices"], device=True, count=False)
    ctx64.sync()
    assert np.array_equal(_bits(_host(d2["vertices"])[:U2]), _bits(h2["vertices"][:U2]))
    assert np.array_equal(_host(d2["indices"])[:K2], h2["indices"][:K2])


def test_weld_simplify_and_edges_queued_over_the_capacities_equal_the_host_chain(ctx64):
    import weld_cases as WC
    _, v, idx = WC.head_soup()
    n, F = v.shape[0], idx.shape[0]
    W, P = api.make_weld_params(14, 0, 3), api.make_simplify_params(14, 0.4, 3)
    w, U = api.mesh_weld(W, v, idx)
    s, (K, Vk) = api.mesh_simplify(P, np.ascontiguousarray(w["vertices"][:U]), w["indices"])
    rec, E = api.mesh_edges(np.ascontiguousarray(s["indices"][:K]), Vk)
    assert 0 < K < F and 0 < E
    d_v, d_idx = _dev(v, 8), _dev(idx, 4)
    _sync()
    d_w, none = ctx64.mesh_weld(W, d_v, d_idx, device=True, count=False)
    d_s, none2 = ctx64.mesh_simplify(P, d_w["vertices"], d_w["indices"], device=True, count=False)
    d_rec, none3 = ctx64.mesh_edges(d_s["indices"], n, device=True, count=False)           # the fill faces name no vertex: no edge
    ctx64.sync()
    assert none is None and none2 is None and none3 is None
    assert np.array_equal(_host(d_rec)[:E], rec[:E])
    assert np.array_equal(_bits(_host(d_s["vertices"])[:Vk]), _bits(s["vertices"][:Vk])) and np.array_equal(_host(d_s["indices"])[:K], s["indices"][:K])


# ---- drawing ------------------------------------------------------------------------------------------------------------------------------
def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _sphere_frame(device, over_capacity):
    """The sphere of 2048 faces, its normals the positions, simplified once with fill ZERO and drawn with PHONG: device - simplified in
    device memory and drawn from there -; over_capacity - the draw runs over all 2048 faces, else over exactly the kept ones."""
    hd = scenes.head_standin(2, 64, 64)
    v, idx = LC.octa_sphere(4, 14)
    v[:, :3] *= 0.8
    v[:, 3:6] = v[:, :3] / 0.8
    P = api.make_simplify_params(14, 0.3, 3, api.CLEAN_FILL_ZERO)
    with Context(64, 64, 3) as ctx:
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
        if device:
            d_v, d_idx = _dev(v, 8), _dev(idx, 4)
            _sync()
            out, counts = ctx.mesh_simplify(P, d_v, d_idx, device=True, count=not over_capacity)
            faces = out["indices"] if over_capacity else out["indices"][:counts[0]]
            ctx.draw_indexed(PHONG, u, hd["projection"], out["vertices"], faces, device=True)
        else:
            out, counts = ctx.mesh_simplify(P, v, idx)
            faces = out["indices"] if over_capacity else np.ascontiguousarray(out["indices"][:counts[0]])
            ctx.draw_indexed(PHONG, u, hd["projection"], out["vertices"], faces)
        return _result(ctx), counts


def test_a_simplified_sphere_draws_the_same_frame_from_device_and_host_arrays_and_over_the_capacity():
    want, (K, U) = _sphere_frame(False, False)
    assert 0 < K < 2048 and want[2][1] > 0, "a coarser sphere, and some of it was drawn"
    got, counts = _sphere_frame(True, False)
    assert counts == (K, U)
    same(got, want, what="simplified in device memory against host memory")
    got, none = _sphere_frame(True, True)
    assert none is None
    same(got, want, stats=False, what="fill ZERO over the capacity against exactly the kept faces")
    got, _ = _sphere_frame(False, True)
    same(got, want, stats=False, what="fill ZERO over the capacity, host arrays")


def test_a_simplification_between_draws_on_a_begun_flush_leaves_their_frame_unchanged():
    from tinyrenderder_amd.api import FLAT
    back = scenes.random_triangles(12, 64, 64, seed=141, rmin=4, rmax=16, perspective_w=True)
    front = scenes.random_triangles(6, 64, 64, seed=142, rmin=3, rmax=9, perspective_w=True)
    v, idx = LC.octa_sphere(3, 8)
    P = api.make_simplify_params(8, 0.4)
    expect, counts = api.mesh_simplify(P, v, idx)
    with Context(64, 64, 3) as ctx:
        ctx.draw(FLAT, back[0], colors=back[1])
        ctx.draw(FLAT, front[0], colors=front[1])
        want = _result(ctx)
    for begun in (False, True):
        with Context(64, 64, 3) as ctx:
            ctx.draw(FLAT, back[0], colors=back[1])
            if begun:
                ctx.flush_begin()                                           # the call completes it, as trgl_clip_stage does
            d_v, d_idx = _dev(v), _dev(idx)
            _sync()
            out, got = ctx.mesh_simplify(P, d_v, d_idx, device=True, count=not begun)
            c_out, _ = ctx.mesh_clean(api.make_clean_params(0, api.CLEAN_DUPLICATES), d_idx, None, v.shape[0], device=True, count=False)
            ctx.draw(FLAT, front[0], colors=front[1])
            same(_result(ctx), want, what=f"simplify between draws, begun={begun}")
            assert got == (None if begun else counts) and np.array_equal(_host(out["remap"]), expect["remap"]) and np.array_equal(_host(c_out["indices"]), idx)
