"""Point sprites and wide lines on the GPU (include/trgl.h: trgl_sprite_stage, trgl_draw_sprites, trgl_line_stage, trgl_draw_lines;
kernels_sprite.hip).

Rows made from device memory equal tests/sprite_model.py bit for bit on both store widths (outputs at 0 and 8 mod 16), at the edges of
a wave and of a block, with nothing written behind them and the inputs left alone; device indices that name no point give zero rows.
A frame drawn by trgl_draw_sprites / trgl_draw_lines equals trgl_draw of the model's rows - bytes, depths, counters and the stats line -
whole and on strips and bands, between queued draws and across a begun flush.  A line and a sprite colour exactly the pixels they must.
Sprites sorted and blended without leaving the device equal the blending model played in sorted order."""
import numpy as np
import pytest

import blend_model as B
import cases
import order_model as O
import sprite_cases as SC
import sprite_model as M
import triangle_order_model as T
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, CHECKER, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
E_INVALID, E_UNSUPPORTED = -1, -5
SENTINEL = 0x5EA7BEEF
SENTINEL_F64 = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]
H, D = api.MEM_HOST, api.MEM_DEVICE
BLOCK = 256                                   # SPRITE_BLOCK of csrc/launch.h
COUNTS = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 257, 5000]


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


def _check_stage(ctx, run, inputs, want, K, what, i):
    """run(out) queues the stage over device inputs; out: sentinel-filled arrays with 3 rows of room behind the 2 n of `want`."""
    rows = want[0].shape[0]
    ooff, coff = (0, 8)[i % 2], (4, 0, 12)[i % 3]
    out = (_dev(np.full((rows + 3, 12), SENTINEL_F64), ooff), _dev(np.full((rows + 3, K), SENTINEL_F64), (8, 0)[(i // 2) % 2]),
           None if want[2] is None else _dev(np.full(rows + 3, SENTINEL, np.uint32), coff))
    _sync()
    run(out)
    ctx.sync()
    got = [None if t is None else _host(t) for t in out]
    what = f"{what} output offsets {ooff},{coff}"
    for name, g, w in zip(("clip", "varyings"), got[:2], want[:2]):
        assert (_bits(g[rows:]) == _bits(SENTINEL_F64)).all(), f"{name} rows behind the output were written: {what}"
        bad = np.argwhere(_bits(g[:rows]) != _bits(w))
        assert bad.size == 0, f"{what}: {bad.shape[0]} {name} doubles differ, first at {bad[:4].tolist()}"
    if want[2] is not None:
        assert (got[2][rows:] == np.uint32(SENTINEL)).all() and np.array_equal(got[2][:rows], want[2]), f"colours: {what}"
    for t, a in inputs:
        if a is not None:
            assert np.array_equal(_host(t).view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), f"an input was written to: {what}"


# ---- the stages against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [M.VIEW, M.SCREEN], ids=["view", "screen"])
@pytest.mark.parametrize("layout", SC.LAYOUTS, ids=lambda l: f"stride{l[0]}_attr{l[1]}")
def test_sprite_rows_from_device_memory_equal_the_model(layout, mode, ctx64):
    ctx = ctx64
    big = layout in (SC.LAYOUTS[3], SC.LAYOUTS[6])                   # 5000 points: one narrow row and the widest
    for i, n in enumerate(COUNTS):
        if n == 5000 and not big:
            continue
        P = SC.sprite_params(mode, layout, size=0.3 if mode == M.VIEW else 6.0)
        pts, col = SC.points(n, layout, seed=300 + n), (SC.colors(n, 9) if i % 4 != 3 else None)
        aP = SC.api_sprite_params(P)
        if n == 0:
            assert ctx.L.trgl_sprite_stage(ctx.h, api.C.byref(aP), None, layout[0], None, 0, D, None, None, None) == 0
            continue
        want = M.sprites(P, pts, col)
        d_pts, d_col = _dev(pts, (8, 0)[i % 2]), _dev(col, (4, 8, 0)[i % 3])
        _check_stage(ctx, lambda out: ctx.sprite_stage(aP, d_pts, d_col, device=True, out=out), [(d_pts, pts), (d_col, col)], want,
                     6 + layout[1], f"n={n} layout={layout} mode={mode}", i)
    # the binding allocates its outputs; without attributes the varyings may be left out
    P = SC.sprite_params(mode, layout)
    pts = SC.points(65, layout, 1)
    got = ctx.sprite_stage(SC.api_sprite_params(P), _dev(pts), device=True)
    ctx.sync()
    assert got[2] is None and np.array_equal(_bits(_host(got[0])), _bits(M.sprites(P, pts)[0]))


@pytest.mark.parametrize("indexed", [False, True], ids=["pairs", "indexed"])
@pytest.mark.parametrize("stride", [3, 4, 9])
def test_line_rows_from_device_memory_equal_the_model(stride, indexed, ctx64):
    ctx = ctx64
    for i, n in enumerate(COUNTS):
        if n == 5000 and stride == 4:
            continue
        P = SC.line_params(width=3.0)
        n_points = 40 if indexed and n < 1000 else max(2 * n, 12)
        pts, idx = SC.segments(n_points, n, seed=400 + n, stride=stride, out_of_range=indexed)
        if not indexed:
            pts, idx = pts[idx.astype(np.int64)], None
        col = SC.colors(n, 10) if i % 4 != 2 else None
        aP = SC.api_line_params(P)
        if n == 0:
            assert ctx.L.trgl_line_stage(ctx.h, api.C.byref(aP), None, stride, 0, None, None, 0, D, None, None, None) == 0
            continue
        want = M.lines(P, pts, idx, col, n_segments=n)
        if indexed:
            bad = (idx.reshape(-1, 2) >= pts.shape[0]).any(axis=1)
            assert bad.any() and (want[0].reshape(n, 24)[bad] == 0).all(), "indices that name no point must give zero rows"
        d_pts, d_idx, d_col = _dev(pts, (0, 8)[i % 2]), _dev(idx, (4, 0, 8)[i % 3]), _dev(col, (4, 8, 0)[i % 3])
        _check_stage(ctx, lambda out: ctx.line_stage(aP, d_pts, d_idx, d_col, n_segments=n, device=True, out=out),
                     [(d_pts, pts), (d_idx, idx), (d_col, col)], want, 6, f"n={n} stride={stride} indexed={indexed}", i)


# ---- frames: the draws against trgl_draw of the model's rows -----------------------------------------------------------------------
# a user kind that samples the diffuse texture at the interpolated uv of `vec2 varying_uv[3]`
TEXTURED_SRC = r"""
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (v[0] * in.bar[0] + v[2] * in.bar[1]) + v[4] * in.bar[2], (v[1] * in.bar[0] + v[3] * in.bar[1]) + v[5] * in.bar[2] };
    return trgl_sample2D(in, in.u->tex_diffuse, uv).bgra;
}
"""
MODES = {"one": {}, "begun": dict(begun=True), "halves": dict(halves=True), "strip": dict(strip=(5, 23)), "bands0": dict(interleave=(32, 0, 2)),
         "bands1": dict(interleave=(32, 1, 2))}
N_PRIMS = 150


def _frame_inputs(prim, w, h):
    """(model rows, params for the model, points, indices, colours) of the frame's sprites or lines."""
    if prim == "sprites":
        layout = SC.LAYOUTS[2]
        P = SC.sprite_params(M.SCREEN, layout, w, h)
        pts = SC.points(N_PRIMS, layout, 51)
        with np.errstate(invalid="ignore"):
            pts[:, 3] *= 30.0                                        # 1.5 .. 15 pixels, the planted sizes among them
        idx, col = None, SC.colors(N_PRIMS, 52)
        return M.sprites(P, pts, col), P, pts, idx, col
    P = SC.line_params(width=3.0, w=w, h=h)
    pts, idx = SC.segments(60, N_PRIMS, 53)
    col = SC.colors(N_PRIMS, 54)
    return M.lines(P, pts, idx, col), P, pts, idx, col


def _draw_frame(prim, kind_name, w, h, how, strip=None, interleave=None, halves=False, begun=False):
    """how: "rows" - trgl_draw of the model's rows; "host" / "device" - trgl_draw_sprites / trgl_draw_lines over such arrays."""
    rows, P, pts, idx, col = _frame_inputs(prim, w, h)
    back = scenes.random_triangles(12, w, h, seed=141, rmin=4, rmax=16, perspective_w=True)
    front = scenes.random_triangles(20, w, h, seed=142, rmin=3, rmax=12, perspective_w=True)
    with Context(w, h, 3) as ctx:
        u, K = None, 0
        if kind_name == "flat":
            kind = FLAT
        elif kind_name == "checker":
            kind, u = CHECKER, make_uniforms(cells=4)
        else:
            kind, K = ctx.register_shader(TEXTURED_SRC, 6), 6
            ctx.upload_texture(0, scenes.procedural_textures(64)[0])
            u = make_uniforms(tex_diffuse=0)
        if strip:
            ctx.set_strip(*strip)
        if interleave:
            ctx.set_interleave(*interleave)
        ctx.draw(FLAT, back[0], colors=back[1])
        if begun:
            ctx.flush_begin()                                        # the stage completes it, as trgl_clip_stage does
        if how == "rows":
            ctx.draw(kind, rows[0], rows[1] if K else None, rows[2], u)
        else:
            dev = how == "device"
            a = (_dev(pts, 8), _dev(idx, 4), _dev(col, 4)) if dev else (pts.copy(), None if idx is None else idx.copy(), col.copy())
            if dev:
                _sync()
            if prim == "sprites":
                ctx.draw_sprites(kind, SC.api_sprite_params(P), a[0], a[2], uniforms=u, device=dev)
            else:
                ctx.draw_lines(kind, SC.api_line_params(P), a[0], a[1], a[2], uniforms=u, device=dev)
            # host arrays are expanded before the call returns; device arrays are read when the stage runs on the stream
            if dev:
                ctx.sync()
                a[0].fill_(float("nan"))
                a[2].zero_()
                _sync()
            else:
                a[0][:] = np.nan
                a[2][:] = 0
        ctx.draw(FLAT, front[0], colors=front[1])
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        return _result(ctx)


@pytest.mark.parametrize("size", [(96, 64), (37, 29)], ids=["96x64", "37x29"])
@pytest.mark.parametrize("kind_name", ["flat", "checker", "textured"])
@pytest.mark.parametrize("prim", ["sprites", "lines"])
def test_drawn_frame_equals_the_draw_of_the_models_rows(prim, kind_name, size):
    w, h = size
    for name, kw in MODES.items():
        want = _draw_frame(prim, kind_name, w, h, "rows", **kw)
        for how in (("host", "device") if name in ("one", "begun") else ("device",)):
            same(_draw_frame(prim, kind_name, w, h, how, **kw), want, what=f"{prim} {kind_name} {w}x{h} {name} {how}")
        if name == "one":
            assert want[2][0] == 12 + 2 * N_PRIMS + 20 and want[2][1] > 0
    if kind_name != "textured":                                      # built-in kinds: the oracle fed the model's rows
        rows, P, pts, idx, col = _frame_inputs(prim, w, h)
        back = scenes.random_triangles(12, w, h, seed=141, rmin=4, rmax=16, perspective_w=True)
        front = scenes.random_triangles(20, w, h, seed=142, rmin=3, rmax=12, perspective_w=True)
        kind, u = (FLAT, None) if kind_name == "flat" else (CHECKER, make_uniforms(cells=4))
        case = cases.make_case(w, h, [(FLAT, None, back[0], None, back[1]), (kind, u, rows[0], None, rows[2]), (FLAT, None, front[0], None, front[1])])
        got = _draw_frame(prim, kind_name, w, h, "device")
        same(got, cases.run_oracle(case), what=f"{prim} {kind_name} {w}x{h} against the oracle")
        fb_without = cases.run_oracle(cases.make_case(w, h, [case["draws"][0], case["draws"][2]]))[0]
        assert (got[0] != fb_without).any(axis=-1).sum() > 40, "the sprites or lines left hardly a pixel: the frame proves nothing"


# ---- known coverage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_known_coverage_on_the_gpu(device):
    for prim, (P, pts, want) in (("line", SC.coverage_line()), ("sprite", SC.coverage_sprite())):
        col = np.array([SC.RED], np.uint32)
        with Context(SC.W, SC.H, 3) as ctx:
            ctx.clear((0, 0, 0, 255))
            a = (_dev(pts), _dev(col)) if device else (pts, col)
            if device:
                _sync()
            if prim == "line":
                ctx.draw_lines(FLAT, SC.api_line_params(P), a[0], None, a[1], device=device)
            else:
                ctx.draw_sprites(FLAT, SC.api_sprite_params(P), a[0], a[1], device=device)
            fb = ctx.read_framebuffer()
            assert ctx.stats()[0] == 2
        red = (fb == np.array([0, 0, 255], np.uint8)).all(axis=-1)
        assert np.array_equal(red, want) and np.array_equal((fb != 0).any(axis=-1), want), f"{prim}: {np.argwhere(red != want)[:6].tolist()}"


# ---- the all-device chain: sprites, depths, order, blended draw -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [M.VIEW, M.SCREEN], ids=["view", "screen"])
def test_sprites_sorted_and_blended_on_the_device_equal_the_blend_model(mode):
    w, h, n = 96, 64, 110
    layout = SC.LAYOUTS[2]
    P = SC.sprite_params(mode, layout, w, h)
    pts = SC.points(n, layout, 61, planted=False)
    pts[:, 3] = pts[:, 3] * (1.6 if mode == M.VIEW else 40.0)
    col = SC.colors(n, 62)                                           # random alphas
    clip, _, col2 = M.sprites(P, pts, col)
    perm = O.order(T.depths(clip, 2, T.CENTROID))
    rows = (np.asarray(perm, np.int64)[:, None] * 2 + np.arange(2)[None, :]).reshape(-1)
    cfg = dict(w=w, h=h, bpp=3, viewport=scenes.init_viewport(0, 0, w, h), clear=(0, 30, 40, 255), zclear=np.inf)
    m = B.Model(**cfg)
    m.draw(clip[rows], col2[rows], B.f_over, depth_write=False)
    want_sorted = m.result()
    m = B.Model(**cfg)
    m.draw(clip, col2, B.f_over, depth_write=False)
    assert not np.array_equal(want_sorted[0], m.result()[0]), "the scene does not depend on the order: a draw that ignored the list would pass"
    with Context(w, h, 3) as ctx:
        over = ctx.register_shader(B.OVER_SRC, 0, True, reads_dest=True, depth_write=False)
        ctx.set_viewport(cfg["viewport"])
        ctx.clear(cfg["clear"], cfg["zclear"])
        d_pts, d_col = _dev(pts, 8), _dev(col, 4)
        _sync()
        q_clip, _, q_col = ctx.sprite_stage(SC.api_sprite_params(P), d_pts, d_col, device=True)
        depths = ctx.triangle_depths(q_clip, 2, T.CENTROID, device=True)
        order = ctx.depth_order(depths, device=True)
        ctx.draw(over, q_clip, colors=q_col, device=True, order=order, order_device=True, group=2)
        got = _result(ctx)
        assert np.array_equal(_host(order), perm)
    same(got, want_sorted, what=f"mode {mode}: sorted on the device")


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable():
    w, h, n = 64, 64, 6
    layout = SC.LAYOUTS[3]
    P, LP = SC.sprite_params(M.SCREEN, layout), SC.line_params()
    pts, col = SC.points(n, layout, 71, planted=False), SC.colors(n, 72)
    lpts, idx = SC.segments(12, n, 73, planted=False)
    d_pts, d_col, d_lpts, d_idx = _dev(pts), _dev(col), _dev(lpts), _dev(idx)
    d_oc, d_ov, d_ok = _dev(np.zeros((2 * n, 12))), _dev(np.zeros((2 * n, 7))), _dev(np.zeros(2 * n, np.uint32))
    _sync()
    C = api.C
    with Context(w, h, 3) as ctx:
        L = ctx.L
        k7 = ctx.register_shader(TEXTURED_SRC, 7)
        k6 = ctx.register_shader(TEXTURED_SRC, 6)

        def sprite(P=P, points=d_pts.data_ptr(), stride=4, colors=d_col.data_ptr(), n=n, mem=D, oc=d_oc.data_ptr(), ov=d_ov.data_ptr(), ok=d_ok.data_ptr(), **kw):
            return L.trgl_sprite_stage(ctx.h, C.byref(SC.api_sprite_params(dict(P, **kw))), points, stride, colors, n, mem, oc, ov, ok)

        for name, kw in dict(bad_mode=dict(mode=9), bad_mem=dict(mem=3), stride_below_3=dict(stride=2), size_offset_outside=dict(size_offset=4),
                             attr_outside=dict(attr_offset=4), null_points=dict(points=None), null_clip_out=dict(oc=None), null_vary_out=dict(ov=None),
                             null_colors_out=dict(ok=None), misaligned_points=dict(points=d_pts.data_ptr() + 4), misaligned_vary_out=dict(ov=d_ov.data_ptr() + 4),
                             misaligned_colors_out=dict(ok=d_ok.data_ptr() + 2), output_over_input=dict(oc=d_pts.data_ptr())).items():
            assert sprite(**kw) == E_INVALID, name
            assert L.trgl_last_error(ctx.h), name
        assert sprite(n=1 << 30) == E_UNSUPPORTED and sprite(n=0, points=None, oc=None, ov=None, ok=None, colors=None) == 0

        def line(points=d_lpts.data_ptr(), stride=3, n_points=12, indices=d_idx.data_ptr(), colors=d_col.data_ptr(), n=n, mem=D, oc=d_oc.data_ptr(),
                 ov=d_ov.data_ptr(), ok=d_ok.data_ptr(), **kw):
            return L.trgl_line_stage(ctx.h, C.byref(SC.api_line_params(dict(LP, **kw))), points, stride, n_points, indices, colors, n, mem, oc, ov, ok)

        for name, kw in dict(bad_mem=dict(mem=3), stride_below_3=dict(stride=2), w_min_zero=dict(w_min=0.0), w_min_nan=dict(w_min=np.nan),
                             too_few_points=dict(indices=None, n=7), null_points=dict(points=None), null_clip_out=dict(oc=None),
                             misaligned_indices=dict(indices=d_idx.data_ptr() + 2), misaligned_clip_out=dict(oc=d_oc.data_ptr() + 4),
                             output_over_indices=dict(ok=d_idx.data_ptr())).items():
            assert line(**kw) == E_INVALID, name
            assert L.trgl_last_error(ctx.h), name
        assert line(n=1 << 30) == E_UNSUPPORTED and line(n=0, points=None, indices=None, colors=None, oc=None, ov=None, ok=None) == 0
        ctx.sync()
        assert (_host(d_oc) == 0).all() and (_host(d_ok) == 0).all(), "a refused call wrote rows"

        def draw_sprites(kind=FLAT, u=None, P=P, points=d_pts.data_ptr(), stride=4, colors=d_col.data_ptr(), n=n, mem=D, **kw):
            return L.trgl_draw_sprites(ctx.h, kind, u, C.byref(SC.api_sprite_params(dict(P, **kw))), points, stride, colors, n, mem)

        def draw_lines(kind=FLAT, u=None, points=d_lpts.data_ptr(), stride=3, n_points=12, indices=d_idx.data_ptr(), colors=d_col.data_ptr(), n=n, mem=D, **kw):
            return L.trgl_draw_lines(ctx.h, kind, u, C.byref(SC.api_line_params(dict(LP, **kw))), points, stride, n_points, indices, colors, n, mem)

        for name, rc in dict(unknown_kind=draw_sprites(kind=999), k6_with_an_attribute=draw_sprites(kind=k6), k0_with_an_attribute=draw_sprites(kind=FLAT),
                             checker_without_uniforms=draw_sprites(kind=CHECKER, n_attr=0), bad_mode=draw_sprites(mode=4, n_attr=0),
                             null_points=draw_sprites(points=None, n_attr=0), misaligned_points=draw_sprites(points=d_pts.data_ptr() + 4, n_attr=0),
                             host_null_points=draw_sprites(points=None, mem=H, n_attr=0),
                             lines_k7=draw_lines(kind=k7), lines_unknown_kind=draw_lines(kind=-3), lines_w_min=draw_lines(w_min=-1.0),
                             lines_null_points=draw_lines(points=None), lines_misaligned_indices=draw_lines(indices=d_idx.data_ptr() + 2)).items():
            assert rc == E_INVALID, name
        assert draw_sprites(n=1 << 30, n_attr=0) == E_UNSUPPORTED and draw_lines(n=1 << 30) == E_UNSUPPORTED
        assert ctx.stats()[0] == 0, "a refused call queued triangles"
        assert draw_sprites(n=0, n_attr=0, points=None, colors=None) == 0 and draw_lines(n=0, points=None, indices=None, colors=None) == 0
        # after the refusals the context draws what a fresh one draws: a kind with 7 varyings takes the attribute, FLAT takes the lines
        assert draw_sprites(kind=k7, u=C.byref(make_uniforms(tex_diffuse=-1))) == 0 and draw_lines() == 0
        got = _result(ctx)
    rows, lrows = M.sprites(P, pts, col), M.lines(LP, lpts, idx, col)
    with Context(w, h, 3) as ctx:
        k7 = ctx.register_shader(TEXTURED_SRC, 7)
        ctx.draw(k7, rows[0], rows[1], rows[2], make_uniforms(tex_diffuse=-1))
        ctx.draw(FLAT, lrows[0], colors=lrows[2])
        same(got, _result(ctx), what="after the refused calls")
    assert got[2][0] == 4 * n and got[2][1] > 0
