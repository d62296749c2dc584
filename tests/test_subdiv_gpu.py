"""Mesh subdivision on the GPU (include/trgl.h: trgl_subdiv_topology, trgl_subdiv_vertices, trgl_draw_subdivided; kernels_subdiv.hip).

Refined indices, stencils and refined vertices made in device memory equal tests/subdiv_model.py bit for bit: at face counts around a
wave and a block, with the seam between even and odd records inside a block of the vertex kernel and exactly on its boundary, a sort of
more than one tile, cones of every valence, vertex counts at which the sort key changes width, every stride, arrays at every alignment
the header allows, counts passed as capacities; sentinels behind every output stay intact and the inputs unchanged.  Device entries
out of range give the header's harmless output.  One topology serves two skinned poses, and a second level is built from the refined
mesh without a count visiting the host.  trgl_draw_subdivided gives the frame, depths and counters of the two calls by hand."""
import numpy as np
import pytest

import cases
import edge_cases as EC
import edge_model as EM
import subdiv_cases as SC
import subdiv_model as M
import vertex_shader_sources as V
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
D = api.MEM_DEVICE
WAVE, BLOCK = 64, 256
FACE_COUNTS = [1, 2, WAVE // 3, WAVE // 3 + 1, BLOCK // 3, BLOCK // 3 + 1, 700]      # as tests/test_edges_gpu.py
TILE_DOUBLES = api.SUBDIV_BLOCK * api.SUBDIV_ITEMS                                     # doubles of the output per block of the vertex kernel
BIG_GRID = 105
SENTINEL_F64 = np.array([SC.SENTINEL_F64_BITS], np.uint64).view(np.float64)[0]
LOOP3 = [(3, 3, M.LOOP)]


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


def _check_topology(ctx, idx, nv, rec, n, what, offs=(0, 0, 0, 0)):
    """trgl_subdiv_topology over device arrays at the byte offsets offs = (indices, records, refined indices, stencils), against the
    model; returns the model's (refined, stencils) and the device stencils."""
    F = idx.shape[0]
    want_ref, want_st = M.topology(idx, nv, rec[:n], device=True)
    words = M.stencil_words(nv, n)
    d_idx, d_rec = _dev(idx, offs[0]), _dev(rec[:n], offs[1])
    d_ref = _dev(np.full(12 * F + 5, SC.SENTINEL_U32, np.uint32), offs[2])
    d_st = _dev(np.full(words + 5, SC.SENTINEL_U32, np.uint32), offs[3])
    _sync()
    ctx.subdiv_topology(d_idx, nv, d_rec, n, device=True, out=(d_ref[:12 * F].view(4 * F, 3), d_st[:words]))
    ctx.sync()
    what = f"{what}: F={F} V={nv} E={n} offsets {offs}"
    ref, st = _host(d_ref), _host(d_st)
    assert (ref[12 * F:] == SC.SENTINEL_U32).all() and (st[words:] == SC.SENTINEL_U32).all(), f"{what}: words behind an output were written"
    bad = np.argwhere(ref[:12 * F].reshape(4 * F, 3) != want_ref)
    assert bad.size == 0, f"{what}: {bad.shape[0]} refined indices differ, first at {bad[:4].tolist()}"
    bad = np.flatnonzero(st[:words] != want_st)
    assert bad.size == 0, f"{what}: {bad.size} stencil words differ, first at {bad[:4].tolist()} (even at {4 * n}, ring at {4 * n + 4 * nv})"
    assert np.array_equal(_host(d_idx), idx) and np.array_equal(_host(d_rec), rec[:n]), f"{what}: an input was written to"
    return want_ref, want_st, d_st[:words]


def _check_vertices(ctx, v, st, d_st, n, stride_modes, what, voff=0, ooff=0):
    nv = v.shape[0]
    for stride, smooth, mode in stride_modes:
        vs = SC.restride((v, None, nv), stride, seed=stride + smooth)[0]
        want = M.vertices(vs, st, n, mode, smooth, device=True)
        d_v = _dev(vs, voff)
        d_out = _dev(np.full((nv + n) * stride + 3, SENTINEL_F64), ooff)
        _sync()
        ctx.subdiv_vertices(api.make_subdiv_params(stride, mode, smooth), d_v, d_st, n, device=True, out=d_out[:(nv + n) * stride].view(nv + n, stride))
        ctx.sync()
        w = f"{what}: V={nv} E={n} stride {stride} smooth {smooth} mode {mode} offsets v{voff} out{ooff}"
        got = _host(d_out)
        assert (_bits(got[(nv + n) * stride:]) == SC.SENTINEL_F64_BITS).all(), f"{w}: doubles behind the output were written"
        bad = np.argwhere(_bits(got[:(nv + n) * stride].reshape(nv + n, stride)) != _bits(want))
        assert bad.size == 0, f"{w}: {bad.shape[0]} doubles differ, first at {bad[:4].tolist()}"
        assert np.array_equal(_bits(_host(d_v)), _bits(vs)), f"{w}: the vertices were written to"
    assert np.array_equal(_host(d_st), st), f"{what}: the stencils were written to"


def _check(ctx, mesh, what, capacity=True, stride_modes=LOOP3, offs=(0, 0, 0, 0), voff=0, ooff=0, rec=None):
    v, idx, nv = mesh
    if rec is None:
        rec, E = EM.edges(idx, nv, device=True)
    else:
        E = rec.shape[0]
    n = rec.shape[0] if capacity else E
    want_ref, want_st, d_st = _check_topology(ctx, idx, nv, rec, n, what, offs)
    pos = np.zeros((nv, 3)) if v is None else v
    _check_vertices(ctx, pos, want_st, d_st, n, stride_modes, what, voff, ooff)
    return want_ref, want_st, n


# ---- counts ---------------------------------------------------------------------------------------------------------------------------
def test_nothing_to_do_is_ok_and_touches_nothing(ctx64):
    L, h = ctx64.L, ctx64.h
    assert L.trgl_subdiv_topology(h, None, 0, 9, None, 0, D, None, None) == 0
    assert L.trgl_subdiv_topology(h, None, 9, 0, None, 0, D, None, None) == 0
    assert L.trgl_subdiv_vertices(h, api.C.byref(api.make_subdiv_params(3)), None, 0, None, 0, D, None) == 0


def test_device_results_equal_the_model_at_every_face_count(ctx64):
    for i, F in enumerate(FACE_COUNTS):
        for nv, seed in ((5, 30 + i), (max(F // 2, 3), 40 + i)):
            mesh = EC.soup(F, nv, seed, stride=3)
            _check(ctx64, mesh, "soup", capacity=bool(i % 2), stride_modes=[(3, 3, M.LOOP), (5, 3, M.LINEAR)],
                   offs=(4 * (i % 4), 4 * ((i + 1) % 4), 4 * ((i + 2) % 4), 4 * ((i + 3) % 4)), voff=8 * (i % 2), ooff=8 * ((i + 1) % 2))
    for name, mesh in SC.named().items():
        if mesh[2] > 4096:
            continue                                                     # (the wide soups: test_every_width_of_the_sort_key)
        for capacity in (False, True):
            _check(ctx64, mesh, name, capacity=capacity, stride_modes=[(3, 3, M.LOOP), (8, 8, M.LOOP), (5, 0, M.LINEAR)])


def test_the_seam_between_even_and_odd_records_inside_a_block_and_on_its_boundary(ctx64):
    # a cone of n rim vertices has n + 1 vertices and 2 n edges; with stride 8 the vertex kernel's blocks hold TILE_DOUBLES / 8 records
    per_block = TILE_DOUBLES // 8
    for n in (per_block - 1, per_block - 2, 2 * per_block - 1, per_block // 2):
        want_ref, want_st, E = _check(ctx64, SC.cone(n), f"cone {n}", capacity=False, stride_modes=[(8, 8, M.LOOP), (8, 3, M.LINEAR)])
        assert ((n + 1) * 8 % TILE_DOUBLES == 0) == (n in (per_block - 1, 2 * per_block - 1))
    # the seam in the middle of a wave's 64 doubles, with a stride that divides nothing
    _check(ctx64, SC.cone(23), "cone 23", capacity=False, stride_modes=[(7, 5, M.LOOP)])


def test_a_sort_of_more_than_one_tile(ctx64):
    mesh = EC.grid(BIG_GRID, BIG_GRID, bump=0.5)
    want_ref, want_st, n = _check(ctx64, mesh, "grid", capacity=True, offs=(4, 8, 12, 4), voff=8)
    assert n == 3 * 2 * BIG_GRID ** 2 and (want_ref.reshape(-1, 12) != 0).any(axis=1).all()


# ---- cones and key widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.CONE_SIZES)
def test_cones_a_long_ring_in_every_lane_of_a_record(n, ctx64):
    want_ref, want_st, E = _check(ctx64, SC.cone(n), f"cone {n}", capacity=False, stride_modes=[(5, 3, M.LOOP), (14, 14, M.LOOP)], voff=8)
    assert want_st[4 * E:4 * E + 4].tolist() == [0, n, M.NONE, M.NONE]


@pytest.mark.parametrize("nv", [k for k in EC.KEY_WIDTH_VERTICES if k < 2 ** 24])
def test_every_width_of_the_sort_key(nv, ctx64):
    """The largest vertex numbers are used: a sort over too few bits would misplace their ring entries."""
    for F, seed in ((9, 1), (300, 2)):
        mesh = EC.soup(F, nv, seed, top=6, stride=3)
        assert mesh[1].max() == nv - 1
        want_ref, want_st, n = _check(ctx64, mesh, "key width", capacity=True, offs=(8, 0, 4, 12))
        even = want_st[4 * n:4 * n + 4 * nv].reshape(nv, 4)
        assert even[nv - 1, 1] > 0, "the last vertex has a ring"


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def test_every_stride_and_every_alignment(ctx64):
    mesh = EC.icosphere(1, 3)
    grid = EC.grid(7, 4, 3, bump=0.4)
    modes = [(s, sm, mode) for s, sm in SC.STRIDES for mode in (M.LOOP, M.LINEAR)] + [(1, 1, M.LOOP), (2, 1, M.LOOP), (300, 299, M.LOOP)]
    for m, name in ((mesh, "icosphere"), (grid, "grid")):
        for voff in (0, 8):
            for ooff in (0, 8):
                _check(ctx64, m, name, capacity=(voff == ooff), stride_modes=modes if voff == 0 and ooff == 0 else [(3, 3, M.LOOP), (5, 3, M.LOOP), (14, 3, M.LOOP)],
                       voff=voff, ooff=ooff)
    k = 0
    for off in (0, 4, 8, 12):
        for which in range(4):                                          # indices, records, refined indices, stencils: one array moves at a time
            offs = [0, 0, 0, 0]
            offs[which] = off
            _check(ctx64, (grid, mesh)[k % 2], "alignment", capacity=bool(k % 3), offs=tuple(offs), stride_modes=[(5, 3, M.LOOP)])
            k += 1


def test_capacities_give_zero_records_and_none_stencils(ctx64):
    v, idx, nv = SC.cone(6, 4)
    rec, E = EM.edges(idx, nv)
    want_ref, want_st, n = _check(ctx64, (v, idx, nv), "cone", capacity=True, stride_modes=[(4, 4, M.LOOP)])
    assert n == 3 * idx.shape[0] and (want_st[4 * E:4 * n] == M.NONE).all() and (want_st[4 * n + 4 * nv + 2 * E:] == M.NONE).all()
    out = M.vertices(v, want_st, n, M.LOOP, 4, device=True)
    assert not out[nv + E:].any() and not np.signbit(out[nv + E:]).any()


# ---- bad device entries: data the kernels compare and skip ------------------------------------------------------------------------------
def test_device_entries_out_of_range_give_the_defined_harmless_output(ctx64):
    v, idx, nv = EC.icosphere(1, 3)
    F = idx.shape[0]
    good, E = EM.edges(idx, nv)
    bad = idx.copy()
    bad[3, 1], bad[9, 0], bad[20, 2], bad[21] = nv, 0xFFFFFFFF, nv + 7, (nv, nv, nv + 1)
    # indices out of range, with the records trgl_mesh_edges makes of them and with those of the sound mesh
    for rec in (None, good):
        want_ref, want_st, n = _check(ctx64, (v, bad, nv), "indices out of range", capacity=True, rec=rec)
        four = want_ref.reshape(F, 12)
        # (a record whose face names a vertex out of range is inconsistent - "no edge" -, so the faces across such an edge go too)
        gone = (four == 0).all(axis=1)
        assert gone[[3, 9, 20, 21]].all() and 4 <= gone.sum() <= 4 + 3 * 4 and not gone[4]
    # records out of range or inconsistent: "no edge", and the faces on them become (0, 0, 0)
    wild = good[:E].copy()
    wild[2, 2], wild[5, 3], wild[7, 2], wild[11, 3] = F, 0xFFFFFFFE, 0x80000000, F + 1
    wild[13, 1], wild[17, 0], wild[19, 1] = 0xFFFFFFFE, wild[17, 1], nv
    wild[23, 2] = (int(wild[23, 2]) + 5) % F                           # a face that does not hold the pair
    wild[29] = M.NONE                                                  # a "no edge" record in the middle
    want_ref, want_st, n = _check(ctx64, (v, idx, nv), "records out of range", capacity=False, rec=wild, stride_modes=[(3, 3, M.LOOP), (5, 3, M.LINEAR)])
    odd = want_st[:4 * E].reshape(E, 4)
    assert (odd[[2, 5, 7, 11, 13, 17, 19, 23, 29]] == M.NONE).all() and (odd[:, 0] != M.NONE).sum() >= E - 12
    assert 0 < (want_ref.reshape(F, 12) == 0).all(axis=1).sum() < F
    # stencil words out of range, over a sound table
    _, st = api.subdiv_topology(idx, nv, good[:E], E)
    even, ring = 4 * E, 4 * E + 4 * nv
    inner_e = int(np.flatnonzero(st[:even].reshape(E, 4)[:, 2] != M.NONE)[3])
    worse = st.copy()
    for at, value in ((4 * 2, nv), (4 * 4 + 1, M.NONE), (4 * inner_e + 2, nv + 3), (4 * (inner_e + 1) + 3, M.NONE), (4 * 9, M.NONE), (4 * 9 + 1, M.NONE),
                      (even + 4 * 1, 2 * E), (even + 4 * 3 + 1, 2 * E + 1), (even + 4 * 5 + 2, 1), (even + 4 * 6 + 3, nv), (even + 4 * 8 + 2, 0x80000000),
                      (ring + int(st[even + 4 * 10]), nv), (ring + int(st[even + 4 * 12]) + 1, M.NONE)):
        worse[at] = value
    d_st = _dev(worse, 4)
    _sync()
    _check_vertices(ctx64, v, worse, d_st, E, [(3, 3, M.LOOP), (5, 5, M.LOOP), (3, 0, M.LINEAR)], "stencil words out of range")
    out = M.vertices(v, worse, E, M.LOOP, 3, device=True)
    assert not out[nv + 2].any() and not out[nv + 4].any() and not out[nv + inner_e].any() and np.array_equal(out[[1, 3, 5, 6, 8, 10, 12]], v[[1, 3, 5, 6, 8, 10, 12]])


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
def test_one_topology_serves_two_skinned_poses_and_a_second_level_needs_no_count(ctx64):
    v, idx, nv = EC.icosphere(1, 8)
    F = idx.shape[0]
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
    # level 1, at load time: capacities everywhere, no count comes back
    n1, nv1 = 3 * F, nv + 3 * F
    d_rec, none = ctx64.mesh_edges(d_idx, nv, device=True, count=False)
    d_ref, d_st = ctx64.subdiv_topology(d_idx, nv, d_rec, device=True)
    d_rec2, none2 = ctx64.mesh_edges(d_ref, nv1, device=True, count=False)
    d_ref2, d_st2 = ctx64.subdiv_topology(d_ref, nv1, d_rec2, device=True)
    assert none is None and none2 is None
    # per pose
    d_skinned = ctx64.skin_stage(*d, device=True)
    P = api.make_subdiv_params(8, M.LOOP, 3)
    level1 = [ctx64.subdiv_vertices(P, d_skinned[q], d_st, device=True) for q in range(2)]
    level2 = [ctx64.subdiv_vertices(P, level1[q], d_st2, device=True) for q in range(2)]
    ctx64.sync()
    rec, E = EM.edges(idx, nv)
    ref, st = M.topology(idx, nv, rec, device=True)
    rec2, E2 = EM.edges(ref, nv1, device=True)
    ref2, st2 = M.topology(ref, nv1, rec2, device=True)
    assert E2 == 2 * E + 3 * F and rec2.shape[0] == 12 * F
    assert np.array_equal(_host(d_rec), rec) and np.array_equal(_host(d_ref), ref) and np.array_equal(_host(d_st), st)
    assert np.array_equal(_host(d_rec2), rec2) and np.array_equal(_host(d_ref2), ref2) and np.array_equal(_host(d_st2), st2)
    for q in range(2):
        want1 = M.vertices(skinned[q], st, n1, M.LOOP, 3, device=True)
        assert np.array_equal(_bits(_host(level1[q])), _bits(want1)), f"pose {q}, level 1"
        want2 = M.vertices(want1, st2, 12 * F, M.LOOP, 3, device=True)
        assert np.array_equal(_bits(_host(level2[q])), _bits(want2)), f"pose {q}, level 2"
        assert want2.shape == (nv1 + 12 * F, 8) and not want1[nv + E:].any(), "unreferenced zero records behind the edges"
    assert not np.array_equal(_host(level2[0]), _host(level2[1])), "the two poses must differ"


# ---- drawing ----------------------------------------------------------------------------------------------------------------------------
def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _coarse_head(w, h):
    """the head stand-in as an indexed mesh of 14-double records with its table"""
    hd = scenes.head_standin(2, w, h)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    rng = scenes.SplitMix64(23)
    verts = np.ascontiguousarray(np.concatenate([pos, nrm, uv, rng.uniform(pos.shape[0] * 6, -1.0, 1.0).reshape(-1, 6)], 1))
    idx = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
    # weld the corners that share a position, so that the mesh has interior edges
    _, first, inverse = np.unique(np.round(pos, 9), axis=0, return_index=True, return_inverse=True)
    verts, idx = np.ascontiguousarray(verts[first]), inverse.reshape(-1, 3).astype(np.uint32)
    rec, E = EM.edges(idx, verts.shape[0])
    refined, st = M.topology(idx, verts.shape[0], rec[:E])
    return hd, verts, idx, E, refined, st


def _subdivided_frame(kind_name, how, device, begun=False):
    """how: "one" - trgl_draw_subdivided; "hand" - trgl_subdiv_vertices, then trgl_draw_indexed(_vs) of its output."""
    w = h = 64
    hd, verts, idx, E, refined, st = _coarse_head(w, h)
    back = scenes.random_triangles(12, w, h, seed=141, rmin=4, rmax=16, perspective_w=True)
    front = scenes.random_triangles(10, w, h, seed=142, rmin=3, rmax=9, perspective_w=True)
    col = ((scenes.SplitMix64(5).u64(refined.shape[0]) & np.uint64(0xFFFFFF)) | np.uint64(0xFF000000)).astype(np.uint32)
    P = api.make_subdiv_params(14, M.LOOP, 3)
    with Context(w, h, 3) as ctx:
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
        vs, colors = None, None
        if kind_name != "builtin":
            vs, colors = ctx.register_vertex_shader(V.RESTATED, 24), col
        ctx.draw(FLAT, back[0], colors=back[1])
        if begun:
            ctx.flush_begin()                                            # the vertex kernel completes it, as trgl_clip_stage does
        a = [verts.copy(), st.copy(), refined.copy(), None if colors is None else colors.copy()]
        if device:
            a = [_dev(verts, 8), _dev(st, 4), _dev(refined, 8), _dev(colors, 4)]
            _sync()
        if how == "one":
            ctx.draw_subdivided(PHONG, u, hd["projection"], P, a[0], a[1], a[2], E, device=device, vertex_shader=vs, colors=a[3])
        else:
            fine = ctx.subdiv_vertices(P, a[0], a[1], E, device=device)
            ctx.draw_indexed(PHONG, u, hd["projection"], fine, a[2], device=device, vertex_shader=vs, colors=a[3])
        # host arrays are read before the call returns; device arrays when the stages run on the stream
        if device:
            ctx.sync()
            a[0].fill_(float("nan")); a[1].zero_()
            _sync()
        else:
            a[0][:] = np.nan; a[1][:] = 0; a[2][:] = 0
        ctx.draw(FLAT, front[0], colors=front[1])
        return _result(ctx), refined.shape[0]


@pytest.mark.parametrize("kind_name, begun", [("builtin", False), ("builtin", True), ("vertex_shader", False), ("vertex_shader", True)])
def test_draw_subdivided_equals_the_two_calls_by_hand(kind_name, begun):
    want, n_faces = _subdivided_frame(kind_name, "hand", False, begun)
    assert want[2][0] == 12 + 10 + n_faces and want[2][1] > 0
    for device in (False, True):
        got, _ = _subdivided_frame(kind_name, "one", device, begun)
        same(got, want, what=f"draw_subdivided {kind_name} device={device} begun={begun}")
    got, _ = _subdivided_frame(kind_name, "hand", True, begun)
    same(got, want, what=f"{kind_name} by hand on the device")


def test_draw_subdivided_refusals_queue_nothing():
    hd, verts, idx, E, refined, st = _coarse_head(64, 64)
    with Context(64, 64, 3) as ctx:
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
        P = api.make_subdiv_params(14, M.LOOP, 3)
        with pytest.raises(api.TrglError, match="trgl_draw_subdivided: smooth"):
            ctx.draw_subdivided(PHONG, u, hd["projection"], api.make_subdiv_params(14, M.LOOP, 15), verts, st, refined, E)
        with pytest.raises(api.TrglError, match="trgl_draw_subdivided: colors"):
            ctx.draw_subdivided(PHONG, u, hd["projection"], P, verts, st, refined, E, colors=np.zeros(refined.shape[0], np.uint32))
        wild = refined.copy(); wild[5, 1] = verts.shape[0] + E
        with pytest.raises(api.TrglError, match="trgl_draw_indexed: index out of range"):
            ctx.draw_subdivided(PHONG, u, hd["projection"], P, verts, st, wild, E)
        bad = st.copy(); bad[1] = verts.shape[0]
        with pytest.raises(api.TrglError, match="trgl_draw_subdivided: a stencil word"):
            ctx.draw_subdivided(PHONG, u, hd["projection"], P, verts, bad, refined, E)
        assert ctx.stats()[0] == 0, "a refused call queued triangles"
        ctx.draw_subdivided(PHONG, u, hd["projection"], P, verts, st, refined, E)
        assert ctx.stats()[0] == refined.shape[0]
