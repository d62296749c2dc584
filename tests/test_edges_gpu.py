"""Mesh edges on the GPU (include/trgl.h: trgl_mesh_edges, trgl_edge_select, trgl_draw_outline; kernels_edge.hip).

Edge records made from indices in device memory, and code bytes, segments and colours selected from them, equal tests/edge_model.py bit
for bit: at the half-edge and record counts around a wave, a block and the lower level of the scan, with sort keys of every width,
arrays at every alignment the header allows, sentinels behind every output intact and the inputs unchanged; device entries that are
out of range make no edge and get code 0.  Edges built once are selected over two poses straight from trgl_skin_stage's device output.
trgl_draw_outline gives the frame, depths and counters of the two calls by hand, and the non-compacted segments draw the same frame."""
import numpy as np
import pytest

import cases
import edge_cases as EC
import edge_model as M
import sprite_cases as SC
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
D = api.MEM_DEVICE
BLOCK, SCAN_CHUNK = 256, 256              # EDGE_BLOCK and INST_SCAN_CHUNK of csrc/launch.h: lanes of a block, block counts per scan block
WAVE = 64
ALL = M.ANY | M.BOUNDARY | M.SILHOUETTE | M.CREASE
# faces whose 3 F half-edges lie around a wave (63, 66), a block (255, 258), several blocks, and one lower-level scan block's
# BLOCK * SCAN_CHUNK entries (the 105 x 105 grid: 22050 faces, 66150 half-edges)
FACE_COUNTS = [1, 2, WAVE // 3, WAVE // 3 + 1, BLOCK // 3, BLOCK // 3 + 1, 700]
PAST_SCAN_GRID = 105
assert 3 * 2 * PAST_SCAN_GRID ** 2 > BLOCK * SCAN_CHUNK > 3 * 2 * (PAST_SCAN_GRID - 1) ** 2


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


def _params(eye, crease_cos=0.5, select=ALL, compact=False):
    return api.make_edge_params(eye, crease_cos, select, EC.CLASS_COLORS, compact)


def _check_edges(ctx, idx, nv, what, ioff=0, ooff=0):
    """trgl_mesh_edges over device indices `ioff` bytes and records `ooff` bytes into their allocations, against the model."""
    F = idx.shape[0]
    want, E = M.edges(idx, nv, device=True)
    d_idx = _dev(idx, ioff)
    d_out = _dev(np.full(12 * F + 9, EC.SENTINEL_U32, np.uint32), ooff)
    _sync()
    got, n = ctx.mesh_edges(d_idx, nv, device=True, out=d_out[:12 * F].view(3 * F, 4))
    what = f"{what}: F={F} nv={nv} offsets idx{ioff} out{ooff}"
    flat = _host(d_out)
    assert n == E, f"{what}: {n} edges, the model has {E}"
    assert (flat[12 * F:] == EC.SENTINEL_U32).all(), f"{what}: words behind the capacity were written"
    bad = np.argwhere(_host(got) != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} words differ, first at {bad[:4].tolist()}"
    assert np.array_equal(_host(d_idx), idx), f"{what}: the indices were written to"
    return want, E


def _check_select(ctx, v, idx, rec, eye, cc, mask, compact, what, offs=(0, 0, 0, 0, 0, 0), count=True):
    """trgl_edge_select over device arrays at the byte offsets offs = (vertices, indices, records, codes, segments, colours)."""
    n = rec.shape[0]
    want = M.select(rec, v, idx, eye, cc, mask, EC.CLASS_COLORS, compact, device=True)
    d_v, d_idx, d_rec = _dev(v, offs[0]), _dev(idx, offs[1]), _dev(rec, offs[2])
    d_codes = _dev(np.full(n + 5, EC.SENTINEL_U8, np.uint8), offs[3])
    d_seg = _dev(np.full(2 * n + 5, EC.SENTINEL_U32, np.uint32), offs[4])
    d_col = _dev(np.full(n + 5, EC.SENTINEL_U32, np.uint32), offs[5])
    _sync()
    out = (d_codes[:n], d_seg[:2 * n].view(n, 2), d_col[:n])
    *_, nsel = ctx.edge_select(_params(eye, cc, mask, compact), d_v, d_idx, d_rec, device=True, out=out, count=count and compact)
    ctx.sync()
    what = f"{what}: n={n} mask={mask} compact={compact} offsets {offs}"
    if count and compact:
        assert nsel == want[3], f"{what}: {nsel} selected, the model has {want[3]}"
    else:
        assert nsel is None
    codes, seg, col = _host(d_codes), _host(d_seg), _host(d_col)
    assert (codes[n:] == EC.SENTINEL_U8).all() and (seg[2 * n:] == EC.SENTINEL_U32).all() and (col[n:] == EC.SENTINEL_U32).all(), \
        f"{what}: bytes behind an output were written"
    for name, got, w in (("codes", codes[:n], want[0]), ("segments", seg[:2 * n].reshape(n, 2), want[1]), ("colours", col[:n], want[2])):
        bad = np.argwhere(got != w)
        assert bad.size == 0, f"{what}: {bad.shape[0]} {name} differ, first at {bad[:4].tolist()}"
    assert np.array_equal(_host(d_v).view(np.uint64), v.view(np.uint64)) and np.array_equal(_host(d_idx), idx) and np.array_equal(_host(d_rec), rec), \
        f"{what}: an input was written to"
    return want


# ---- trgl_mesh_edges ----------------------------------------------------------------------------------------------------------------
def test_edges_from_device_indices_equal_the_model_at_every_count(ctx64):
    n = api.C.c_uint64(7)
    assert ctx64.L.trgl_mesh_edges(ctx64.h, None, 0, 9, D, None, api.C.byref(n)) == 0 and n.value == 0
    for i, F in enumerate(FACE_COUNTS):
        for nv, seed in ((5, 10 + i), (max(F // 2, 3), 20 + i)):              # few vertices: long runs of one edge; more: runs of one and two
            _, idx, _ = EC.soup(F, nv, seed, with_vertices=False)
            _, E = _check_edges(ctx64, idx, nv, "soup", ioff=4 * (i % 4), ooff=4 * ((i + 1) % 4))
            assert E <= 3 * F
    for name, (_, idx, nv) in EC.named().items():
        _check_edges(ctx64, idx, nv, name)
    got, n = ctx64.mesh_edges(_dev(EC.cube()[1]), 8, device=True, count=False)      # NULL count: no wait; the stream orders the read
    ctx64.sync()
    assert n is None and np.array_equal(_host(got), M.edges(EC.cube()[1], 8)[0])


def test_edges_past_the_lower_level_of_the_scan(ctx64):
    v, idx, nv = EC.grid(PAST_SCAN_GRID, PAST_SCAN_GRID, bump=0.5)
    rec, E = _check_edges(ctx64, idx, nv, "grid", ioff=4, ooff=8)
    m = PAST_SCAN_GRID
    assert E == 3 * m * m + 2 * m and idx.shape[0] * 3 > BLOCK * SCAN_CHUNK
    # ... and the selection over the whole capacity, plain and compacted: 66150 records, more than one lower-level scan block
    for compact in (False, True):
        want = _check_select(ctx64, v, idx, rec, (40.0, 30.0, 60.0, 1.0), 0.98, M.BOUNDARY | M.CREASE | M.SILHOUETTE, compact, "grid")
        assert 4 * m < want[3] < E
    _check_select(ctx64, v, idx, rec[:BLOCK * SCAN_CHUNK + 1], (40.0, 30.0, 60.0, 1.0), 0.98, M.ANY, True, "one record past the scan block")


@pytest.mark.parametrize("nv", EC.KEY_WIDTH_VERTICES)
def test_every_width_of_the_sort_key(nv, ctx64):
    """The largest vertex numbers are used: a sort over too few bits would misplace them."""
    for F, seed in ((9, 1), (300, 2)):
        _, idx, _ = EC.soup(F, nv, seed, top=6, with_vertices=False)
        assert idx.max() == nv - 1
        rec, E = _check_edges(ctx64, idx, nv, "key width", ioff=8)
        assert rec[E - 1, 1] == nv - 1 or nv == 2
    if nv > 7:                                                          # just below a power of two and at it: the neighbours of the top bit
        idx = np.array([[nv - 1, nv - 2, 0], [0, nv - 2, nv - 1], [nv // 2, nv // 2 - 1, nv - 1], [1, 0, nv // 2]], np.uint32)
        _check_edges(ctx64, idx, nv, "top bits")


def test_arrays_at_every_alignment(ctx64):
    v, idx, nv = EC.icosphere(1, 5)
    rec = None
    for ioff in (0, 4, 8, 12):
        for ooff in (0, 4, 8, 12):
            rec, E = _check_edges(ctx64, idx, nv, "alignment", ioff, ooff)
    k = 0
    for off4 in (0, 4, 8, 12):
        for which in range(1, 6):                                       # indices, records, codes, segments, colours: one array moves at a time
            offs = [8 * (k % 2), 0, 0, 0, 0, 0]
            offs[which] = off4 if which != 3 else off4 // 4
            for compact in (False, True):
                _check_select(ctx64, v, idx, rec, EC.EYES[k % 3], 0.9, ALL if k % 2 else M.SILHOUETTE | M.CREASE, compact, "alignment", tuple(offs))
            k += 1
    for coff in range(8):                                               # codes at every byte offset
        _check_select(ctx64, v, idx, rec[:E], EC.EYES[0], 0.9, M.CREASE, bool(coff % 2), "codes", (0, 4, 4, coff, 4, 12))


@pytest.mark.parametrize("n", [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_selection_at_every_record_count(n, ctx64):
    v, idx, nv = EC.icosphere(3, 4)
    rec, E = M.edges(idx, nv)
    assert E >= n
    P = api.make_edge_params((0, 0, 1, 0), 0.5, ALL, EC.CLASS_COLORS, True)
    assert ctx64.L.trgl_edge_select(ctx64.h, api.C.byref(P), None, 3, 0, None, 0, None, 0, D, None, None, None, None) == 0
    for k, (mask, compact) in enumerate([(M.SILHOUETTE, True), (M.CREASE | M.SILHOUETTE, False), (M.ANY, True), (0, True)]):
        _check_select(ctx64, v, idx, rec[:n], EC.EYES[k % 3], 0.97, mask, compact, "count", (8, 4, 0, 1, 4, 8), count=k != 2)
    # outputs left out: only what is given is written
    d = [_dev(v), _dev(idx), _dev(rec[:n])]
    d_col = _dev(np.full(n + 2, EC.SENTINEL_U32, np.uint32))
    _sync()
    want = M.select(rec[:n], v, idx, EC.EYES[0], 0.97, M.SILHOUETTE, EC.CLASS_COLORS, True)
    *_, nsel = ctx64.edge_select(_params(EC.EYES[0], 0.97, M.SILHOUETTE, True), *d, device=True, out=(None, None, d_col[:n]))
    assert nsel == want[3] and np.array_equal(_host(d_col)[:n], want[2]) and (_host(d_col)[n:] == EC.SENTINEL_U32).all()


def test_device_entries_out_of_range_make_no_edge_and_get_code_zero(ctx64):
    v, idx, nv = EC.icosphere(1, 3)
    bad = idx.copy()
    bad[3, 1], bad[9, 0], bad[20, 2], bad[21] = nv, 0xFFFFFFFF, nv + 7, (nv, nv, nv + 1)
    rec, E = _check_edges(ctx64, bad, nv, "indices out of range")
    good, E0 = M.edges(idx, nv)
    # (the mesh is closed: an edge that loses one half-edge keeps the other and becomes a boundary)
    assert 0 < E <= E0 and (good[:E0, 3] != M.NONE).all() and (rec[:E, 3] == M.NONE).sum() >= 6 and rec[:E, :2].max() < nv
    # records that name a face >= n_faces, and faces that name a vertex >= n_vertices
    wild = good.copy()
    wild[2, 2], wild[5, 3], wild[7, 2], wild[11, 3] = idx.shape[0], 0xFFFFFFFE, 0x80000000, idx.shape[0] + 1
    for compact in (False, True):
        want = _check_select(ctx64, v, idx, wild, EC.EYES[0], 0.5, ALL, compact, "records out of range")
        codes = M.select(wild, v, idx, EC.EYES[0], 0.5, ALL, device=True)[0]
        assert (codes[[2, 5, 7, 11]] == 0).all() and (codes[:E0] != 0).sum() == E0 - 4 and want[3] == E0 - 4
        want = _check_select(ctx64, v, bad, good, EC.EYES[0], 0.5, ALL, compact, "faces with vertices out of range")
        assert 0 < want[3] < E0


# ---- the skinned chain --------------------------------------------------------------------------------------------------------------
def test_edges_built_once_are_selected_over_two_skinned_poses_in_device_memory(ctx64):
    v, idx, nv = EC.icosphere(2, 8)
    t = np.clip((v[:, 1] + 1.0) / 2.0, 0.0, 1.0)
    joints = np.tile(np.array([0, 1], np.uint16), (nv, 1))
    weights = np.stack([1.0 - t, t], axis=1)
    c, s = np.cos(0.9), np.sin(0.9)
    bend = np.array([c, -s, 0, 0.4, s, c, 0, 0.1, 0, 0, 1, 0, 0, 0, 0, 1], np.float64)
    twist = np.array([c, 0, s, 0, 0, 1.5, 0, 0.3, -s, 0, c, 0, 0, 0, 0, 1], np.float64)
    pal = np.stack([np.stack([np.eye(4).reshape(16), bend]), np.stack([twist, np.eye(4).reshape(16)])])
    skinned = api.skin_stage(v, joints, weights, pal)                                # the host twin: [2, nv, 8]
    import torch
    d_idx = _dev(idx, 4)
    d_j = torch.from_numpy(joints.view(np.int16)).cuda()
    d = [_dev(v, 8), d_j, _dev(weights), _dev(pal)]
    _sync()
    d_rec, E = ctx64.mesh_edges(d_idx, nv, device=True)                               # once, at load time
    d_skinned = ctx64.skin_stage(*d, device=True)
    eye, P = (1.5, 2.5, 4.0, 1.0), dict(crease_cos=0.95, select=M.SILHOUETTE | M.CREASE)
    rec = _host(d_rec)
    sets = []
    for q in range(2):
        codes, seg, col, n = ctx64.edge_select(api.make_edge_params(eye, P["crease_cos"], P["select"], EC.CLASS_COLORS, True), d_skinned[q], d_idx,
                                               d_rec, n_edges=E, device=True)
        want = M.select(rec[:E], skinned[q], idx, eye, 0.95, P["select"], EC.CLASS_COLORS, True)
        assert n == want[3] and np.array_equal(_host(codes), want[0]) and np.array_equal(_host(seg), want[1]) and np.array_equal(_host(col), want[2]), f"pose {q}"
        assert 20 < n < E
        sets.append(want[0].tobytes())
    assert sets[0] != sets[1], "the two poses must differ in their outlines"
    assert np.array_equal(rec, M.edges(idx, nv)[0])


# ---- drawing ------------------------------------------------------------------------------------------------------------------------
def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _outline_frame(how, device, kind_K=0, begun=False):
    """how: "one" - trgl_draw_outline; "hand" - trgl_edge_select with compaction and trgl_draw_lines of the count; "plain" - the
    non-compacted segments of the whole capacity through trgl_draw_lines."""
    w = h = 64
    v, idx, nv = EC.icosphere(2, 8)
    v = v.copy(); v[:, :3] *= 0.9
    rec, E = M.edges(idx, nv)
    LP = SC.api_line_params(SC.line_params(width=2.0, identity_view=False))
    eye = (0.3, 0.2, 3.0, 1.0)                                          # the camera of SC.camera, in model space
    back = scenes.random_triangles(12, w, h, seed=141, rmin=4, rmax=16, perspective_w=True)
    front = scenes.random_triangles(6, w, h, seed=142, rmin=3, rmax=9, perspective_w=True)
    sel = M.SILHOUETTE | M.CREASE
    with Context(w, h, 3) as ctx:
        kind = FLAT if kind_K == 0 else ctx.register_shader(SIDE_SHADER, 6)
        ctx.draw(FLAT, back[0], colors=back[1])
        if begun:
            ctx.flush_begin()                                           # the selection completes it, as trgl_clip_stage does
        a = [v.copy(), idx.copy(), rec.copy()]
        if device:
            a = [_dev(v, 8), _dev(idx, 4), _dev(rec, 8)]
            _sync()
        n_rows = None
        if how == "one":
            ctx.draw_outline(kind, LP, _params(eye, 0.96, sel), a[0], a[1], a[2], device=device)
        else:
            compact = how == "hand"
            _, seg, col, n = ctx.edge_select(_params(eye, 0.96, sel, compact), a[0], a[1], a[2], device=device)
            n_rows = n if compact else rec.shape[0]
            ctx.draw_lines(kind, LP, a[0], seg.reshape(-1) if device else seg, col, n_segments=n_rows, device=device)
        if device:                                                      # device arrays are read when the stages run on the stream
            ctx.sync()
            a[0].fill_(float("nan")); a[2].zero_()
            _sync()
        else:
            a[0][:] = np.nan; a[2][:] = 0
        ctx.draw(FLAT, front[0], colors=front[1])
        return _result(ctx), n_rows


# a user kind with the line stage's 6 varyings - (t, side) per vertex: the colour fades along the segment
SIDE_SHADER = r"""
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    const double t = (v[0] * in.bar[0] + v[2] * in.bar[1]) + v[4] * in.bar[2];
    const uint32_t fade = (uint32_t)(fmin(fmax(t, 0.0), 1.0) * 200.0);
    return 0xFF000000u | (in.color & 0x00FFFF00u) | fade;
}
"""


@pytest.mark.parametrize("kind_K, begun", [(0, False), (0, True), (6, False)])
def test_draw_outline_equals_the_two_calls_by_hand(kind_K, begun):
    want, n = _outline_frame("hand", False, kind_K, begun=begun)
    assert n > 20 and want[2][0] == 12 + 6 + 2 * n and want[2][1] > 0
    for device in (False, True):
        got, _ = _outline_frame("one", device, kind_K, begun=begun)
        same(got, want, what=f"draw_outline K={kind_K} device={device} begun={begun}")
    got, n_dev = _outline_frame("hand", True, kind_K, begun=begun)
    assert n_dev == n
    same(got, want, what="by hand on the device")


def test_the_plain_segments_draw_the_same_frame_with_the_dropped_rows_counted():
    want, n = _outline_frame("hand", False)
    got, cap = _outline_frame("plain", True)
    same(got, want, stats=False, what="plain segments in device memory")
    assert got[2][0] - want[2][0] == 2 * (cap - n) and got[2][1:] == want[2][1:]
    # in host memory trgl_line_stage refuses an index that names no point: host callers compact
    with pytest.raises(api.TrglError, match="trgl_draw_lines: index out of range"):
        _outline_frame("plain", False)


def test_draw_outline_of_nothing_and_its_refusals_queue_nothing():
    v, idx, nv = EC.cube(3)
    rec, E = M.edges(idx, nv)
    LP = SC.api_line_params(SC.line_params(identity_view=False))
    with Context(64, 64, 3) as ctx:
        inside = _params((0.0, 0.1, 0.2, 1.0), -2.0, M.SILHOUETTE)
        for device in (False, True):
            a = [_dev(v), _dev(idx), _dev(rec)] if device else [v, idx, rec]
            if device:
                _sync()
            ctx.draw_outline(FLAT, LP, inside, *a, device=device)       # from inside a cube nothing is a silhouette
        assert ctx.stats()[0] == 0
        bad = _params((0.0, 0.1, 0.2, 1.0), -2.0, 16)
        with pytest.raises(api.TrglError, match="trgl_draw_outline: unknown bit"):
            ctx.draw_outline(FLAT, LP, bad, v, idx, rec)
        with pytest.raises(api.TrglError, match="trgl_draw_lines: the shader kind"):
            ctx.draw_outline(api.PHONG, LP, inside, v, idx, rec)
        wild = rec.copy(); wild[0, 2] = 99
        with pytest.raises(api.TrglError, match="trgl_draw_outline: a record"):
            ctx.draw_outline(FLAT, LP, inside, v, idx, wild)
        assert ctx.stats()[0] == 0, "a refused call queued triangles"
        ctx.draw_outline(FLAT, LP, _params((3.0, 2.0, 5.0, 1.0), -2.0, M.ANY), v, idx, rec)
        assert ctx.stats()[0] == 2 * E
