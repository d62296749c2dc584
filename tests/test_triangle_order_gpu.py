"""Depth-ordered triangle draws on the GPU (include/trgl.h: trgl_triangle_depths, trgl_order_stage, trgl_draw_ordered;
kernels_triorder.hip).

Depths equal tests/triangle_order_model.py bit for bit - NaN payloads and signs included - and exactly G of them are written.  Gathered
rows equal the model on every access path (16-, 8- and 4-byte units), with nothing written behind them and zero rows for the entries of
a device list that name no group.  A frame drawn by trgl_draw_ordered equals trgl_draw of arrays permuted on the host: bytes, depths,
counters and the stats line, whole and on strips and bands, for every mix of host and device memory.  A translucent mesh drawn through
depths, order and the ordered draw, all in device memory, equals the blending model played in sorted order."""
import numpy as np
import pytest

import blend_model as B
import cases
import order_model as O
import triangle_order_cases as TC
import triangle_order_model as T
import user_shader_sources as US
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, CHECKER, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
E_INVALID, E_UNSUPPORTED = -1, -5
SENTINEL = 0x5EA7BEEF
SENTINEL_F64 = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]
H, D = api.MEM_HOST, api.MEM_DEVICE


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a, off=0):
    return None if a is None else cases.device_array(a, off)


def _sync():
    import torch
    torch.cuda.synchronize()                 # uploads run on torch's stream; a context's own stream is not ordered behind it


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


@pytest.fixture(scope="module")
def ctx64():
    with Context(64, 64, 3) as ctx:
        yield ctx


# ---- depths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", TC.DEPTH_GROUP_SIZES)
@pytest.mark.parametrize("G", TC.DEPTH_GROUPS)
def test_depths_equal_the_model(G, g, ctx64):
    ctx = ctx64
    clip = TC.planted_clip(G, g, seed=G + g)
    if G == 0:
        for mode in T.MODES:
            assert ctx.L.trgl_triangle_depths(ctx.h, None, 0, g, mode, D, None) == 0
            assert ctx.triangle_depths(clip, g, mode).shape == (0,)
        return
    d_clip = _dev(clip, 8)                                           # 8 mod 16: nothing wider than 8-byte alignment is assumed
    assert d_clip.data_ptr() % 16 == 8
    for mode in T.MODES:
        want = T.depths(clip, g, mode)
        assert np.array_equal(_bits(ctx.triangle_depths(clip, g, mode)), _bits(want)), "host memory through a context"
        out = _dev(np.full(G + 5, SENTINEL_F64), 8 if mode == T.NEAREST else 0)
        _sync()
        assert ctx.L.trgl_triangle_depths(ctx.h, d_clip.data_ptr(), G * g, g, mode, D, out.data_ptr()) == 0
        ctx.sync()
        got = _host(out)
        assert (_bits(got[G:]) == _bits(SENTINEL_F64)).all(), "depths behind G were written"
        bad = np.flatnonzero(_bits(got[:G]) != _bits(want))
        assert bad.size == 0, f"G={G} g={g} mode={mode}: {bad.size} depths differ, first at {bad[:5]}: {_bits(got[:G])[bad[:5]]} != {_bits(want)[bad[:5]]}"
        depths = ctx.triangle_depths(d_clip, g, mode, device=True)                       # the binding: a tensor, not waited for
        for direction in (O.BACK_TO_FRONT, O.FRONT_TO_BACK):                             # ... and straight into the sort
            order = ctx.depth_order(depths, front_to_back=bool(direction), device=True)
            ctx.sync()
            assert np.array_equal(_host(order), O.order(want, direction)), f"order of the depths, direction {direction}"
        assert np.array_equal(_bits(_host(depths)), _bits(want))
    assert np.array_equal(_bits(_host(d_clip)), _bits(clip)), "the clip rows were written to"


# ---- the gather --------------------------------------------------------------------------------------------------------------
DOUBLE_OFFS = (8, 0)                     # 8 mod 16 first: the 8-byte units; 0: the 16-byte ones where the row length allows
WORD_OFFS = (4, 12, 0)                   # 4 mod 16 (and so 4 mod 8), 12 mod 16 (4 mod 8), aligned


@pytest.mark.parametrize("colors", [False, True], ids=["no_colors", "colors"])
@pytest.mark.parametrize("K", TC.GATHER_K)
def test_gathered_rows_equal_the_model(K, colors, ctx64):
    ctx = ctx64
    for i, (rows, g, kind, n_order, G) in enumerate(TC.list_plan()):
        clip, vary, col = TC.gather_rows(G * g, K, colors)
        out_rows = n_order * g
        for bad_entries in (False, True):
            order = TC.order_list(kind, G, n_order, out_of_range=bad_entries)
            want = T.gather(clip, vary, col, order, g, zero_out_of_range=bad_entries)
            if not bad_entries:
                host = ctx.order_stage(clip, vary, col, order, g)
                assert np.array_equal(_bits(host[0]), _bits(want[0])) and (K == 0 or np.array_equal(_bits(host[1]), _bits(want[1])))
                assert not colors or np.array_equal(host[2], want[2])
            doff, woff = DOUBLE_OFFS[(i + bad_entries) % 2], WORD_OFFS[(i + bad_entries) % 3]
            ooff = DOUBLE_OFFS[(i // 2) % 2]
            a = (_dev(clip, doff), _dev(vary, doff), _dev(col, woff), _dev(order, woff))
            out = (_dev(np.full((out_rows + 3, 12), SENTINEL_F64), ooff), _dev(np.full((out_rows + 3, K), SENTINEL_F64), ooff) if K else None,
                   _dev(np.full(out_rows + 3, SENTINEL, np.uint32), WORD_OFFS[(i + 1) % 3]) if colors else None)
            _sync()
            ctx.order_stage(a[0], a[1], a[2], a[3], g, device=True, out=out)
            ctx.sync()
            what = f"rows={rows} g={g} list={kind} n_order={n_order} G={G} bad={bad_entries} offsets={doff},{woff},{ooff}"
            got = [None if t is None else _host(t) for t in out]
            assert (_bits(got[0][out_rows:]) == _bits(SENTINEL_F64)).all(), "clip rows behind the output were written: " + what
            assert np.array_equal(_bits(got[0][:out_rows]), _bits(want[0])), "clip rows differ: " + what
            if K:
                assert (_bits(got[1][out_rows:]) == _bits(SENTINEL_F64)).all(), "varyings behind the output were written: " + what
                assert np.array_equal(_bits(got[1][:out_rows]), _bits(want[1])), "varyings differ: " + what
            if colors:
                assert (got[2][out_rows:] == np.uint32(SENTINEL)).all(), "colours behind the output were written: " + what
                assert np.array_equal(got[2][:out_rows], want[2]), "colours differ: " + what
            assert np.array_equal(_bits(_host(a[0])), _bits(clip)) and np.array_equal(_host(a[3]), order), "inputs were written to: " + what
            assert (K == 0 or np.array_equal(_bits(_host(a[1])), _bits(vary))) and (not colors or np.array_equal(_host(a[2]), col)), what


# ---- frames: the ordered draw against trgl_draw of arrays permuted on the host ------------------------------------------------
N_TRIS = 150
MODES = {"one": {}, "halves": dict(halves=True), "strip": dict(strip=(5, 23)), "bands0": dict(interleave=(32, 0, 2)),
         "bands1": dict(interleave=(32, 1, 2))}
USER_K5 = (US.GOURAUD_PADDED, 5, False, False, True)                 # a user kind that does not discard, with an odd K
BLEND_OVER = (B.OVER_SRC, 0, True, True, False)                      # reads the pixel, leaves the depth alone
FRAME_KINDS = {"flat": FLAT, "gouraud": GOURAUD, "phong": PHONG, "checker": CHECKER, "user_k5": USER_K5, "blend_over": BLEND_OVER}
MEMORY = [(False, False), (False, True), (True, False), (True, True)]      # (rows in device memory, list in device memory)


def _frame_inputs(kind_name, w, h, group):
    """(background, kind, uniforms, clip, varyings, colours, textures, order list) of a frame."""
    back = scenes.random_triangles(40, w, h, seed=141, rmin=4, rmax=30, perspective_w=True)
    clip, col = scenes.random_triangles(N_TRIS, w, h, seed=142 + len(kind_name), rmin=3, rmax=28, perspective_w=True)
    r = scenes.SplitMix64(143)
    u, vary, tex = None, None, {}
    if kind_name == "gouraud":
        vary = r.uniform(N_TRIS * 3, -0.2, 1.3).reshape(N_TRIS, 3)
    elif kind_name == "phong":
        hd = scenes.head_standin(1, w, h)
        d, n, s = scenes.procedural_textures(64)
        tex = {0: d, 1: n, 2: s}
        u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.7, 0, 1, 2)
        vary, col = cases.phong_soup_varyings(N_TRIS, 144), None
    elif kind_name == "checker":
        u = make_uniforms(cells=4)
    elif kind_name == "user_k5":
        vary = r.uniform(N_TRIS * 5, -0.2, 1.3).reshape(N_TRIS, 5)
    elif kind_name == "blend_over":
        col = (r.u64(N_TRIS) >> np.uint64(32)).astype(np.uint32)     # random alphas
    G = N_TRIS // group
    perm = np.argsort(r.u64(G), kind="stable")
    order = np.concatenate([perm[:G - G // 5], perm[:7]]).astype(np.uint32)          # a subset, a few groups twice
    return back, FRAME_KINDS[kind_name], u, clip, vary, col, tex, order


def _rows_of(order, group):
    return (np.asarray(order, np.int64)[:, None] * group + np.arange(group)[None, :]).reshape(-1)


def _draw_frame(kind_name, w, h, group, how, strip=None, interleave=None, halves=False, order=None):
    """how: "permuted" - trgl_draw of the arrays permuted on the host; or (rows in device memory, list in device memory)."""
    (bclip, bcol), frag, u, clip, vary, col, tex, order0 = _frame_inputs(kind_name, w, h, group)
    order = order0 if order is None else order
    with Context(w, h, 3) as ctx:
        kind = frag if isinstance(frag, int) else ctx.register_shader(frag[0], frag[1], frag[2], reads_dest=frag[3], depth_write=frag[4])
        if strip:
            ctx.set_strip(*strip)
        if interleave:
            ctx.set_interleave(*interleave)
        for slot, t in tex.items():
            ctx.upload_texture(slot, t)
        ctx.draw(FLAT, bclip, colors=bcol)
        if how == "permuted":
            rows = _rows_of(order, group)
            ctx.draw(kind, clip[rows], None if vary is None else vary[rows], None if col is None else col[rows], u)
        else:
            rows_dev, list_dev = how
            a = (_dev(clip, 8), _dev(vary, 8), _dev(col, 4)) if rows_dev else (clip, vary, col)
            o = _dev(order, 4) if list_dev else order
            _sync()
            ctx.draw(kind, a[0], a[1], a[2], u, device=rows_dev, order=o, order_device=list_dev, group=group)
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        return _result(ctx)


@pytest.mark.parametrize("size", [(96, 64, 1), (37, 29, 2)], ids=["96x64_g1", "37x29_g2"])
@pytest.mark.parametrize("kind_name", sorted(FRAME_KINDS))
def test_ordered_frame_equals_the_draw_of_permuted_arrays(kind_name, size):
    w, h, group = size
    for name, kw in MODES.items():
        want = _draw_frame(kind_name, w, h, group, "permuted", **kw)
        for how in (MEMORY if name == "one" else [MEMORY[(len(name) + w) % 4]]):
            same(_draw_frame(kind_name, w, h, group, how, **kw), want, what=f"{kind_name} {w}x{h} {name} device rows/list={how}")
        if name != "one":
            continue
        assert want[2][1] > 0 and want[2][0] == 40 + (len(_frame_inputs(kind_name, w, h, group)[7])) * group
        if isinstance(FRAME_KINDS[kind_name], int):                  # built-in kinds: the oracle fed the permuted arrays
            (bclip, bcol), kind, u, clip, vary, col, tex, order = _frame_inputs(kind_name, w, h, group)
            rows = _rows_of(order, group)
            case = cases.make_case(w, h, [(FLAT, None, bclip, None, bcol),
                                          (kind, u, clip[rows], None if vary is None else vary[rows], None if col is None else col[rows])], textures=tex)
            same(want, cases.run_oracle(case), what=f"{kind_name} {w}x{h} against the oracle")


@pytest.mark.parametrize("kind_name", ["flat", "blend_over"])
def test_out_of_range_entries_of_a_device_list_are_counted_and_leave_no_other_trace(kind_name):
    w, h, group = 96, 64, 2
    order = _frame_inputs(kind_name, w, h, group)[7]
    G = N_TRIS // group
    bad = np.insert(order, [0, 3, 3, 50, len(order)], np.array([G, 0xFFFFFFFF, 1 << 31, G + 7, G], np.uint64).astype(np.uint32))
    want = _draw_frame(kind_name, w, h, group, "permuted")
    for rows_dev in (False, True):
        got = _draw_frame(kind_name, w, h, group, (rows_dev, True), order=bad)
        same(got, want, stats=False, what=f"{kind_name}, device rows={rows_dev}")
        assert got[2][0] == 40 + len(bad) * group == want[2][0] + 5 * group, "triangles_rasterized counts the zero rows"
        assert got[2][1:] == want[2][1:], "the zero rows left a trace in the counters"


# ---- a translucent mesh: depths, order and the draw in device memory, against the blending model -----------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", ["96x64_bpp3", "32x32_long_list"])
def test_translucent_mesh_equals_the_blend_model_in_sorted_order(name, group):
    cfg, clip, col = B.frame(name)
    mode = T.CENTROID if group == 1 else T.FARTHEST
    perm = O.order(T.depths(clip, group, mode))
    rows = _rows_of(perm, group)
    m = B.Model(**cfg)
    m.draw(clip[rows], col[rows], B.f_over, depth_write=False)
    want_sorted = m.result()
    want_array = B.model_frame(name, B.f_over, depth_write=False)
    assert not np.array_equal(want_sorted[0], want_array[0]), "the scene does not depend on the order: a draw that ignored the list would pass"
    with Context(cfg["w"], cfg["h"], cfg["bpp"]) as ctx:
        over = ctx.register_shader(B.OVER_SRC, 0, True, reads_dest=True, depth_write=False)
        ctx.set_viewport(cfg["viewport"])
        ctx.clear(cfg["clear"], cfg["zclear"])
        d_clip, d_col = _dev(clip), _dev(col)
        _sync()
        depths = ctx.triangle_depths(d_clip, group, mode, device=True)
        order = ctx.depth_order(depths, device=True)
        ctx.draw(over, d_clip, colors=d_col, device=True, order=order, order_device=True, group=group)
        got = _result(ctx)
        assert np.array_equal(_host(order), perm)
    same(got, want_sorted, what=f"{name}, group {group}: sorted on the device")
    with Context(cfg["w"], cfg["h"], cfg["bpp"]) as ctx:
        over = ctx.register_shader(B.OVER_SRC, 0, True, reads_dest=True, depth_write=False)
        ctx.set_viewport(cfg["viewport"])
        ctx.clear(cfg["clear"], cfg["zclear"])
        ctx.draw(over, clip, colors=col)
        same(_result(ctx), want_array, what=f"{name}: array order")


# ---- queue order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["between_draws", "after_clear", "after_flush_begin", "after_set_stream"])
def test_an_ordered_draw_keeps_its_place_in_the_queue(where):
    import torch
    w, h, group = 96, 64, 1
    (bclip, bcol), _, _, clip, _, col, _, order = _frame_inputs("flat", w, h, group)
    front = scenes.random_triangles(30, w, h, seed=151, rmin=4, rmax=30, perspective_w=True)
    rows = _rows_of(order, group)

    def prologue(ctx):
        ctx.draw(FLAT, bclip, colors=bcol)
        if where == "after_clear":
            ctx.flush()
            ctx.clear((9, 8, 7, 255), 0.75)
        if where == "after_flush_begin":
            ctx.flush_begin()
        if where == "after_set_stream":
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    with Context(w, h, 3) as ctx:
        prologue(ctx)
        ctx.draw(FLAT, clip[rows], colors=col[rows])
        ctx.draw(FLAT, front[0], colors=front[1])
        want = _result(ctx)
        if where == "after_set_stream":
            ctx.set_stream(None, use_own=True)
    for rows_dev, list_dev in MEMORY:
        a = [_dev(clip, 8), _dev(col, 4)] if rows_dev else [clip.copy(), col.copy()]
        o = _dev(order, 4) if list_dev else order.copy()
        _sync()
        with Context(w, h, 3) as ctx:
            prologue(ctx)
            ctx.draw(FLAT, a[0], colors=a[1], device=rows_dev, order=o, order_device=list_dev, group=group)
            # host arrays are copied before the call returns; device arrays are read when the gather runs on the stream
            if not rows_dev:
                a[0][:] = np.nan
                a[1][:] = 0
            if not list_dev:
                o[:] = 0
            if rows_dev or list_dev:
                ctx.sync()
                if rows_dev:
                    a[0].fill_(float("nan"))
                    a[1].zero_()
                if list_dev:
                    o.zero_()
                _sync()
            ctx.draw(FLAT, front[0], colors=front[1])
            got = _result(ctx)
            if where == "after_set_stream":
                ctx.set_stream(None, use_own=True)
        same(got, want, what=f"{where}, device rows/list={rows_dev}/{list_dev}")


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable():
    w, h = 64, 64
    clip, col = scenes.random_triangles(12, w, h, seed=161, rmin=4, rmax=30)
    vary = scenes.SplitMix64(162).uniform(36, 0.0, 1.0).reshape(12, 3)
    order = np.array([3, 0, 5, 1], np.uint32)
    bad_order = np.array([3, 6, 0], np.uint32)
    d_clip, d_vary, d_col, d_order = _dev(clip), _dev(vary), _dev(col), _dev(order)
    d_out = _dev(np.zeros((16, 12)))
    d_vout, d_cout, d_depths = _dev(np.zeros((16, 3))), _dev(np.zeros(16, np.uint32)), _dev(np.zeros(16))
    _sync()
    with Context(w, h, 3) as ctx:
        L = ctx.L
        # trgl_triangle_depths in device memory
        td = lambda clip=d_clip.data_ptr(), n=12, g=2, mode=0, mem=D, out=d_depths.data_ptr(): L.trgl_triangle_depths(ctx.h, clip, n, g, mode, mem, out)
        for name, kw in dict(bad_mode=dict(mode=3), bad_mem=dict(mem=9), group_zero=dict(g=0), not_a_multiple=dict(g=5), null_clip=dict(clip=None),
                             null_out=dict(out=None), misaligned_clip=dict(clip=d_clip.data_ptr() + 4), misaligned_out=dict(out=d_depths.data_ptr() + 4)).items():
            assert td(**kw) == E_INVALID, name
            assert L.trgl_last_error(ctx.h), name
        assert td(n=1 << 31, g=1) == E_UNSUPPORTED
        assert td(n=0, clip=None, out=None) == 0
        # trgl_order_stage in device memory
        base = dict(K=3, clip=d_clip.data_ptr(), vary=d_vary.data_ptr(), col=d_col.data_ptr(), n=12, order=d_order.data_ptr(), n_order=4, g=2, mem=D,
                    oc=d_out.data_ptr(), ov=d_vout.data_ptr(), ok=d_cout.data_ptr())

        def stage(**kw):
            a = dict(base, **kw)
            return L.trgl_order_stage(ctx.h, a["K"], a["clip"], a["vary"], a["col"], a["n"], a["order"], a["n_order"], a["g"], a["mem"], a["oc"], a["ov"], a["ok"])

        for name, kw in dict(bad_mem=dict(mem=-1), K_negative=dict(K=-1), K_too_large=dict(K=65), group_zero=dict(g=0), not_a_multiple=dict(g=5),
                             null_order=dict(order=None), null_clip=dict(clip=None), null_vary=dict(vary=None), null_clip_out=dict(oc=None),
                             null_vary_out=dict(ov=None), null_colors_out=dict(ok=None), misaligned_clip=dict(clip=d_clip.data_ptr() + 4),
                             misaligned_vary_out=dict(ov=d_vout.data_ptr() + 4), misaligned_colors=dict(col=d_col.data_ptr() + 2),
                             misaligned_order=dict(order=d_order.data_ptr() + 2),
                             host_entry_out_of_range=dict(mem=H, clip=clip.ctypes.data, vary=vary.ctypes.data, col=col.ctypes.data, order=bad_order.ctypes.data,
                                                          n_order=3, oc=np.zeros((6, 12)).ctypes.data, ov=np.zeros((6, 3)).ctypes.data,
                                                          ok=np.zeros(6, np.uint32).ctypes.data)).items():
            assert stage(**kw) == E_INVALID, name
            assert L.trgl_last_error(ctx.h), name
        assert stage(n=1 << 31, g=1) == E_UNSUPPORTED
        assert stage(n_order=1 << 30) == E_UNSUPPORTED
        assert stage(n_order=0, order=None) == 0
        ctx.sync()
        assert (_host(d_out) == 0).all() and (_host(d_cout) == 0).all(), "a refused call wrote rows"
        # trgl_draw_ordered
        dbase = dict(kind=GOURAUD, u=None, clip=clip.ctypes.data, vary=vary.ctypes.data, col=col.ctypes.data, n=12, mem=H, order=order.ctypes.data,
                     n_order=4, g=2, omem=H)

        def draw(**kw):
            a = dict(dbase, **kw)
            return L.trgl_draw_ordered(ctx.h, a["kind"], a["u"], a["clip"], a["vary"], a["col"], a["n"], a["mem"], a["order"], a["n_order"], a["g"], a["omem"])

        for name, kw in dict(bad_order_mem=dict(omem=2), null_order_with_count=dict(order=None), order_without_count=dict(n_order=0),
                             unknown_kind=dict(kind=999), bad_mem=dict(mem=4), group_zero=dict(g=0), not_a_multiple=dict(g=5), null_clip=dict(clip=None),
                             null_varyings=dict(vary=None), checker_without_uniforms=dict(kind=CHECKER, vary=None),
                             host_entry_out_of_range=dict(order=bad_order.ctypes.data, n_order=3),
                             host_entry_out_of_range_device_rows=dict(order=bad_order.ctypes.data, n_order=3, mem=D, clip=d_clip.data_ptr(),
                                                                      vary=d_vary.data_ptr(), col=d_col.data_ptr()),
                             misaligned_device_order=dict(order=d_order.data_ptr() + 2, omem=D),
                             misaligned_device_clip=dict(mem=D, clip=d_clip.data_ptr() + 4, vary=d_vary.data_ptr(), col=d_col.data_ptr()),
                             misaligned_device_colors=dict(mem=D, clip=d_clip.data_ptr(), vary=d_vary.data_ptr(), col=d_col.data_ptr() + 2)).items():
            assert draw(**kw) == E_INVALID, name
            assert L.trgl_last_error(ctx.h), name
        assert draw(n=1 << 31, g=1) == E_UNSUPPORTED
        assert draw(n_order=1 << 30, order=d_order.data_ptr(), omem=D) == E_UNSUPPORTED
        assert ctx.stats()[0] == 0, "a refused call queued triangles"
        # a null list with no entries is trgl_draw
        assert draw(order=None, n_order=0, g=0) == 0
        got_plain = _result(ctx)
    with Context(w, h, 3) as ctx:
        ctx.draw(GOURAUD, clip, vary, col)
        same(got_plain, _result(ctx), what="a null list after the refused calls")
    rows = _rows_of(order, 2)
    case = cases.make_case(w, h, [(GOURAUD, None, clip[rows], vary[rows], col[rows])])
    with Context(w, h, 3) as ctx:                                    # and after a refusal an ordered draw is what a fresh context draws
        assert ctx.L.trgl_draw_ordered(ctx.h, GOURAUD, None, clip.ctypes.data, vary.ctypes.data, col.ctypes.data, 12, H, bad_order.ctypes.data, 3, 2, H) == E_INVALID
        ctx.draw(GOURAUD, clip, vary, col, order=order, group=2)
        got = _result(ctx)
    same(got, cases.run_oracle(case), what="after the refused call, against the oracle")
    assert got[2][0] == 8
