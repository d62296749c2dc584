"""Skeletal animation on the GPU (include/trgl.h: trgl_skin_stage, trgl_pose_palette, trgl_draw_skinned; kernels_skin.hip).

Vertex arrays skinned from device memory equal tests/skin_model.py bit for bit: at the edges of a wave and of a block, with records of
odd and even sizes, arrays at every alignment the header allows, palettes staged in LDS and read through the cache (SKIN_LDS_JOINTS and
one more), several poses, sentinels behind the output intact and the inputs unchanged; a device joint number that names no joint
contributes nothing.  Palettes composed on the device equal the model for chains, stars and forests, with world matrices kept in LDS
and (300 joints) passed through memory.  trgl_draw_skinned gives the frame, depths and counters of trgl_skin_stage followed by
trgl_draw_indexed / trgl_draw_indexed_vs by hand.  The chain palette - skin - bounds - normals - draw in device memory equals the chain
of host twins."""
import numpy as np
import pytest

import cases
import discard_shader_sources as DS
import skin_cases as SC
import skin_model as M
import vertex_shader_sources as V
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
D = api.MEM_DEVICE
BLOCK, LDS_JOINTS, POSE_LDS_JOINTS = 256, 128, 96      # SKIN_BLOCK, SKIN_LDS_JOINTS, POSE_LDS_JOINTS of csrc/launch.h
COUNTS = SC.COUNTS + [5000]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a, off=0):
    """a device tensor holding `a`, `off` bytes into its allocation; 16-bit joints travel as int16"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint16:
        return cases.device_array(a, off)
    import torch
    assert off % 2 == 0
    lead = off // 2
    buf = torch.empty(a.size + lead + 1, dtype=torch.int16, device="cuda")
    t = buf[lead:lead + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a.view(np.int16)))
    assert t.data_ptr() == buf.data_ptr() + off
    return t


def _sync():
    import torch
    torch.cuda.synchronize()                 # uploads run on torch's stream; a context's own stream is not ordered behind it


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32) if a.dtype == np.int32 else a


def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


@pytest.fixture(scope="module")
def ctx64():
    with Context(64, 64, 3) as ctx:
        yield ctx


def _dev_palette(pal, off=0):
    """the padded palette array of SC.palette on the device, and the view of its matrices [n_poses, n_joints, 16]"""
    buf = pal.base if pal.base is not None else pal
    t = _dev(buf, off)
    return t, t[:, :16 * pal.shape[1]].unflatten(1, (pal.shape[1], 16))


def _check_skin(ctx, v, j, w, pal, flags, i, what, out_of_range=False):
    """One call over device arrays at the alignments of round i, against the model."""
    n, stride = v.shape
    poses = pal.shape[0]
    want = M.skin(v, j, w, pal, flags, skip_out_of_range=out_of_range)
    voff, woff, ooff, joff, poff = (0, 8)[i % 2], (8, 0)[(i // 2) % 2], (0, 8)[(i // 3) % 2], (0, 2, 4, 6)[i % 4], (8, 0)[i % 2]
    d_v, d_j, d_w = _dev(v, voff), _dev(j, joff), _dev(w, woff)
    d_buf, d_pal = _dev_palette(pal, poff)
    d_out = _dev(np.full(poses * n * stride + 2 * stride + 1, SC.SENTINEL_F64), ooff)
    _sync()
    got = ctx.skin_stage(d_v, d_j, d_w, d_pal, flags, device=True, out=d_out[:poses * n * stride].view(poses, n, stride))
    ctx.sync()
    what = f"{what} offsets v{voff} w{woff} out{ooff} j{joff} pal{poff}"
    flat = _host(d_out)
    assert (_bits(flat[poses * n * stride:]) == _bits(SC.SENTINEL_F64)).all(), f"doubles behind the output were written: {what}"
    bad = np.argwhere(_bits(_host(got)) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.shape[0]} doubles differ, first at {bad[:4].tolist()}"
    for t, a in ((d_v, v), (d_j, j), (d_w, w), (d_buf, pal.base if pal.base is not None else pal)):
        assert np.array_equal(_host(t).view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), f"an input was written to: {what}"
    return want


# ---- the skin stage against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_infl", SC.INFLUENCES)
@pytest.mark.parametrize("stride", SC.STRIDES)
def test_skinned_arrays_from_device_memory_equal_the_model(stride, n_infl, ctx64):
    big = stride in (3, 17)                                          # 5000 vertices: one narrow record and one wide
    flag_sets = SC.flag_sets(stride)
    i = 0
    for n in COUNTS:
        if n == 5000 and not big:
            continue
        if n == 0:
            P = api.SkinParams(stride, n_infl, 7, 0, 1, 0, 0)
            assert ctx64.L.trgl_skin_stage(ctx64.h, api.C.byref(P), None, 0, None, None, None, D, None) == 0
            continue
        for flags in (flag_sets if n in (65, 257) else [flag_sets[-1], flag_sets[i % len(flag_sets)]]):
            n_poses, pad = ((1, 0), (2, 3), (5, 0))[i % 3]
            v, j, w = SC.mesh(n, stride, n_infl, 7, seed=2000 * stride + 10 * n_infl + n)
            _check_skin(ctx64, v, j, w, SC.palette(n_poses, 7, seed=n + flags, pad=pad), flags, i, f"n={n} flags={flags} poses={n_poses}")
            i += 1


@pytest.mark.parametrize("n_joints", [1, 2, LDS_JOINTS, LDS_JOINTS + 1, 65536])
def test_both_palette_paths_give_the_models_bits(n_joints, ctx64):
    """Up to SKIN_LDS_JOINTS joints the three used rows of each are staged in LDS; more are read through the cache."""
    for i, (n, stride, n_infl, flags, n_poses) in enumerate([(257, 8, 4, M.NORMAL, 1), (300, 14, 3, 7, 2), (65, 3, 8, 0, 5)]):
        if n_joints == 65536 and i:
            continue
        v, j, w = SC.mesh(n, stride, n_infl, n_joints, seed=77 + i)
        j[20:24] = n_joints - 1                                      # the last joint is used, whatever the draw of the others
        want = _check_skin(ctx64, v, j, w, SC.palette(n_poses, n_joints, seed=5 + i, pad=(0, 2)[i % 2]), flags, i, f"{n_joints} joints, case {i}")
        assert np.isfinite(want[..., :3]).mean() > 0.5


def test_a_wide_record_takes_fewer_vertices_per_block(ctx64):
    """A record of 61 doubles: 83 vertices fill a block's tile, so 300 vertices make four blocks of uneven size."""
    v, j, w = SC.mesh(300, 61, 2, 9, seed=88)
    _check_skin(ctx64, v, j, w, SC.palette(3, 9, 6, pad=1), 7, 1, "stride 61")


def test_the_widest_record_fills_a_tile_and_a_wider_one_is_refused(ctx64):
    """SKIN_TILE_DOUBLES = 5120: one vertex per block at that stride; one double more is TRGL_E_UNSUPPORTED with device memory."""
    v, j, w = SC.mesh(3, 5120, 2, 4, seed=89)
    _check_skin(ctx64, v, j, w, SC.palette(2, 4, 7), 7, 2, "stride 5120")
    v, j, w = SC.mesh(2, 5121, 2, 4, seed=90)
    pal = SC.palette(1, 4, 8)
    d = _dev(v), _dev(j), _dev(w), _dev(np.ascontiguousarray(pal)), _dev(np.full(2 * 5121, SC.SENTINEL_F64))
    _sync()
    P = api.SkinParams(5121, 2, 4, 0, 1, 0, 0)
    assert ctx64.L.trgl_skin_stage(ctx64.h, api.C.byref(P), d[0].data_ptr(), 2, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), D, d[4].data_ptr()) == -5
    ctx64.sync()
    assert (_bits(_host(d[4])) == _bits(SC.SENTINEL_F64)).all()
    assert np.array_equal(_bits(api.skin_stage(v, j, w, pal)), _bits(M.skin(v, j, w, pal))), "host memory takes any stride"


def test_device_joints_that_name_no_joint_contribute_nothing(ctx64):
    for i, (n, stride, n_infl, n_joints) in enumerate([(257, 8, 4, 7), (100, 6, 1, 1), (300, 14, 8, LDS_JOINTS + 1)]):
        v, j, w = SC.mesh(n, stride, n_infl, n_joints, seed=91 + i, out_of_range=True)
        bad = j >= n_joints
        assert bad.any() and not bad.all()
        want = _check_skin(ctx64, v, j, w, SC.palette(2, n_joints, 7 + i), M.NORMAL, i, f"out of range, case {i}", out_of_range=True)
        alone = bad.all(axis=1) & np.isfinite(v[:, :3]).all(axis=1)
        if n_infl == 1:
            assert alone.any() and (want[:, alone, :3] == 0).all(), "a vertex whose joints all name no joint has B = 0"


# ---- palettes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain", "star", "forest"])
@pytest.mark.parametrize("n_joints", [1, 2, 17, 64, POSE_LDS_JOINTS, POSE_LDS_JOINTS + 1, 300])
def test_palettes_composed_on_the_device_equal_the_model(n_joints, kind, ctx64):
    ctx = ctx64
    parents = SC.hierarchy(kind, n_joints, seed=n_joints)
    for i, n_poses in enumerate([1, 63, 64, 65, 1000]):
        loc, ib = SC.locals_(n_poses, n_joints, seed=300 + n_joints + n_poses)
        for with_ib in (True, False):
            want = M.pose_palette(parents, loc, ib if with_ib else None)
            pad = (0, 5)[i % 2]
            d_par, d_loc, d_ib = _dev(parents, (0, 4)[i % 2]), _dev(loc, (8, 0)[i % 2]), (_dev(ib, (0, 8)[i % 2]) if with_ib else None)
            d_buf = _dev(np.full((n_poses, 16 * n_joints + pad), SC.SENTINEL_F64), (0, 8)[(i + with_ib) % 2])
            d_out = d_buf[:, :16 * n_joints].unflatten(1, (n_joints, 16))
            _sync()
            got = ctx.pose_palette(d_par, d_loc, d_ib, device=True, out=d_out)
            ctx.sync()
            what = f"{kind} {n_joints} joints {n_poses} poses inverse_bind={with_ib}"
            bad = np.argwhere(_bits(_host(got)) != _bits(want))
            assert bad.size == 0, f"{what}: {bad.shape[0]} doubles differ, first at {bad[:4].tolist()}"
            assert (_bits(_host(d_buf)[:, 16 * n_joints:]) == _bits(SC.SENTINEL_F64)).all(), f"the padding was written: {what}"
            assert np.array_equal(_bits(_host(d_loc)), _bits(loc)) and np.array_equal(_host(d_par).view(np.int32), parents)


def test_a_device_parent_that_is_not_below_its_joint_is_a_root(ctx64):
    for n_joints in (17, 300):
        parents = SC.hierarchy("forest", n_joints, seed=4)
        parents[5], parents[9], parents[11], parents[16] = 5, 12, -7, 0x7FFFFFFF
        loc, ib = SC.locals_(9, n_joints, seed=12)
        want = M.pose_palette(parents, loc, ib, bad_parent_is_root=True)
        d = _dev(parents), _dev(loc), _dev(ib)
        _sync()
        got = ctx64.pose_palette(*d[:2], d[2], device=True)
        ctx64.sync()
        assert np.array_equal(_bits(_host(got)), _bits(want)), n_joints
        as_roots = parents.copy(); as_roots[[5, 9, 11, 16]] = -1
        assert np.array_equal(_bits(want), _bits(M.pose_palette(as_roots, loc, ib)))


# ---- trgl_draw_skinned against the two calls by hand ------------------------------------------------------------------------------------
def _head(w, h):
    """The head stand-in as an indexed mesh of 14-double records (tangent and bitangent random), on a neck: joint 0 the neck, joint 1
    the skull; the weight of the skull grows with height."""
    hd = scenes.head_standin(2, w, h)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    rng = scenes.SplitMix64(17)
    verts = np.concatenate([pos, nrm, uv, rng.uniform(pos.shape[0] * 6, -1.0, 1.0).reshape(-1, 6)], 1)
    perm = np.argsort(rng.u64(pos.shape[0]), kind="stable")
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    verts, idx = np.ascontiguousarray(verts[perm]), inv.astype(np.uint32).reshape(-1, 3)
    t = np.clip((verts[:, 1] - verts[:, 1].min()) / np.ptp(verts[:, 1]), 0.0, 1.0)
    weights = np.stack([1.0 - t, t], axis=1)
    joints = np.tile(np.array([0, 1], np.uint16), (verts.shape[0], 1))
    nod = np.eye(4); nod[:3, :3] = SC.rot_z(20.0)[:3, :3]; nod[0, 3] = 0.1
    pal = np.stack([np.eye(4).reshape(16), nod.reshape(16)])[None]
    return hd, verts, idx, joints, weights, pal


DRAW_MODES = {"one": {}, "begun": dict(begun=True), "strip": dict(strip=(9, 41))}


def _skinned_frame(kind_name, how, device, begun=False, strip=None):
    """how: "one" - trgl_draw_skinned; "hand" - trgl_skin_stage, then trgl_draw_indexed(_vs) of its output."""
    w = h = 64
    hd, verts, idx, joints, weights, pal = _head(w, h)
    flags = M.NORMAL | M.TANGENT
    back = scenes.random_triangles(12, w, h, seed=141, rmin=4, rmax=16, perspective_w=True)
    front = scenes.random_triangles(10, w, h, seed=142, rmin=3, rmax=9, perspective_w=True)
    col = ((scenes.SplitMix64(5).u64(idx.shape[0]) & np.uint64(0xFFFFFF)) | np.uint64(0xFF000000)).astype(np.uint32)
    with Context(w, h, 3) as ctx:
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
        kind, vs, colors = PHONG, None, None
        if kind_name != "builtin":
            vs, colors = ctx.register_vertex_shader(V.RESTATED, 24), col
        if kind_name == "discard":
            kind = ctx.register_shader(DS.PHONG, 24, True)
        if strip:
            ctx.set_strip(*strip)
        ctx.draw(FLAT, back[0], colors=back[1])
        if begun:
            ctx.flush_begin()                                        # the skin stage completes it, as trgl_clip_stage does
        a = [verts.copy(), joints.copy(), weights.copy(), pal.copy(), idx.copy(), None if colors is None else colors.copy()]
        if device:
            a = [_dev(verts, 8), _dev(joints, 2), _dev(weights, 8), _dev(pal, 8), _dev(idx, 4), _dev(colors, 4)]
            _sync()
        if how == "one":
            ctx.draw_skinned(kind, u, hd["projection"], a[0], a[1], a[2], a[3], a[4], flags, device=device, vertex_shader=vs, colors=a[5])
        else:
            skinned = ctx.skin_stage(a[0], a[1], a[2], a[3], flags, device=device)[0]
            ctx.draw_indexed(kind, u, hd["projection"], skinned, a[4], device=device, vertex_shader=vs, colors=a[5])
        # host arrays are read before the call returns; device arrays when the stages run on the stream
        if device:
            ctx.sync()
            a[0].fill_(float("nan")); a[2].zero_(); a[3].zero_()
            _sync()
        else:
            a[0][:] = np.nan; a[2][:] = 0; a[3][:] = 0; a[4][:] = 0
        ctx.draw(FLAT, front[0], colors=front[1])
        return _result(ctx)


@pytest.mark.parametrize("kind_name", ["builtin", "vertex_shader", "discard"])
def test_draw_skinned_equals_skin_stage_and_draw_indexed_by_hand(kind_name):
    for name, kw in DRAW_MODES.items():
        want = _skinned_frame(kind_name, "hand", False, **kw)
        for device in (False, True):
            same(_skinned_frame(kind_name, "one", device, **kw), want, what=f"{kind_name} {name} device={device}")
        same(_skinned_frame(kind_name, "hand", True, **kw), want, what=f"{kind_name} {name} by hand on the device")
        if name == "one":
            assert want[2][0] == 12 + 10 + _head(64, 64)[2].shape[0] and want[2][1] > 0


def test_draw_skinned_refusals_queue_nothing():
    hd, verts, idx, joints, weights, pal = _head(64, 64)
    C = api.C
    with Context(64, 64, 3) as ctx:
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
        pj = np.ascontiguousarray(hd["projection"], np.float64).reshape(16)
        bad_idx = idx.copy(); bad_idx[3, 1] = verts.shape[0]
        bad_j = joints.copy(); bad_j[7, 0] = 2
        col = np.zeros(idx.shape[0], np.uint32)

        def call(vs=-1, kind=PHONG, poses=1, flags=1, idx=idx, joints=joints, colors=None, palette=pal):
            P = api.SkinParams(14, 2, 2, flags, poses, 32 if poses > 1 else 0, 0)
            return ctx.L.trgl_draw_skinned(ctx.h, vs, kind, C.byref(u), pj.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P), verts.ctypes.data,
                                           verts.shape[0], joints.ctypes.data, weights.ctypes.data, None if palette is None else palette.ctypes.data,
                                           idx.ctypes.data, idx.shape[0], None if colors is None else colors.ctypes.data, api.MEM_HOST)

        for name, rc in dict(two_poses=call(poses=2), unknown_flag=call(flags=8), index_out_of_range=call(idx=bad_idx), joint_out_of_range=call(joints=bad_j),
                             colors_with_the_builtin_stage=call(colors=col), unknown_vertex_shader=call(vs=3), flat_kind=call(kind=FLAT),
                             null_palette=call(palette=None)).items():
            assert rc == -1, name
        assert ctx.stats()[0] == 0, "a refused call queued triangles"
        assert call() == 0 and ctx.stats()[0] == idx.shape[0]


# ---- the chain in device memory against the chain of host twins ---------------------------------------------------------------------
def test_palette_skin_bounds_normals_draw_in_device_memory_equal_the_host_chain():
    w = h = 64
    hd, verts, idx, joints, weights, _ = _head(w, h)
    verts[:, 3:6] = 0.0                                              # no normals: trgl_mesh_normals makes them from the skinned positions
    parents = np.array([-1, 0], np.int32)
    loc = np.stack([np.stack([SC.translation(0.02 * q, 0.0), (SC.rot_z(12.0 * q) @ SC.translation(0.0, 0.05 * q).reshape(4, 4)).reshape(16)]) for q in range(3)])
    ib = np.stack([SC.translation(0.0, 0.0), SC.translation(0.0, -0.05)])
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])

    with Context(w, h, 3) as ctx:                                    # host twins, drawn from host memory
        h_pal = api.pose_palette(parents, loc, ib)
        h_skinned = api.skin_stage(verts, joints, weights, h_pal)
        h_bounds = api.mesh_bounds(h_skinned[1])
        h_mesh, generated = api.mesh_normals(h_skinned[1], idx)
        assert generated
        ctx.draw_indexed(PHONG, u, hd["projection"], h_mesh, idx)
        want = _result(ctx)
    with Context(w, h, 3) as ctx:
        d = dict(parents=_dev(parents), loc=_dev(loc, 8), ib=_dev(ib), v=_dev(verts, 8), j=_dev(joints, 2), w=_dev(weights), idx=_dev(idx, 4))
        _sync()
        d_pal = ctx.pose_palette(d["parents"], d["loc"], d["ib"], device=True)
        d_skinned = ctx.skin_stage(d["v"], d["j"], d["w"], d_pal, device=True)
        d_bounds = ctx.mesh_bounds(d_skinned[1], device=True)
        d_mesh, _ = ctx.mesh_normals(d_skinned[1], d["idx"], device=True, wait=False)
        ctx.draw_indexed(PHONG, u, hd["projection"], d_mesh, d["idx"], device=True)
        got = _result(ctx)
        assert np.array_equal(_bits(_host(d_pal)), _bits(h_pal))
        assert np.array_equal(_bits(_host(d_skinned)[[0, 2]]), _bits(h_skinned[[0, 2]])) and np.array_equal(_bits(_host(d_skinned)[1]), _bits(h_mesh))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(d_bounds, h_bounds))
    same(got, want, what="the chain in device memory")
    assert want[2][1] > 0 and not np.array_equal(_bits(h_skinned[0]), _bits(h_skinned[1]))
