"""Depth-ordered instanced draws on the GPU (include/trgl.h: trgl_instance_depths, trgl_depth_order, trgl_draw_instanced_ordered,
trgl_instance_stage_ordered; kernels_order.hip and the ordered kernels of kernels_instance.hip).

Depths and orders equal tests/order_model.py bit for bit, in host and device memory, and exactly n entries are written.  The rows of an
ordered stage equal tests/instance_model.py fed the instances in the order's sequence - every kind of list, every visibility pattern,
every mix of host and device memory - with nothing written behind them.  A frame drawn by an ordered call equals the frame of
trgl_draw_instanced over arrays permuted on the host: bytes, depths, counters and the stats line, whole and on strips and bands.  A
translucent scene drawn through depths, order and draw equals the blending model played in sorted order, and occlusion codes, depths
and the order stay on the device from the query to the draw."""
import ctypes as C
import os

import numpy as np
import pytest

import blend_model as B
import cases
import instance_model as M
import instanced_cases as IC
import occlusion_model as om
import order_cases as OC
import order_model as O
import vertex_shader_sources as V
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
E_INVALID, E_UNSUPPORTED = -1, -5
NAN_BITS = np.float64(np.nan).view(np.uint64)
SENTINEL = 0x5EA7BEEF


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a):
    return None if a is None else cases.device_array(a)


def _dev_bytes(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()                 # uploads run on torch's stream; a context's own stream is not ordered behind it


def _same_doubles(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.fixture(scope="module")
def ctx64():
    with Context(64, 64, 3) as ctx:
        vs = {name: ctx.register_vertex_shader(src, K) for name, (src, K) in IC.STAGES.items()}
        yield ctx, vs


@pytest.fixture(scope="module")
def camera():
    hd = scenes.head_standin(1, 64, 64)
    return hd, make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])


# ---- depths and order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", OC.SIZES)
def test_depths_equal_the_model(n, ctx64, camera):
    import torch
    ctx, _ = ctx64
    hd, _ = camera
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_depth_golden.npz"))["abp"].view(np.float64)
    point = np.array([0.25, -0.5, 0.125])
    for stride in (16, 19):
        inst = IC.instances(n, stride, seed=40) if n else np.zeros((0, stride))
        if n > 100:
            inst[4:100, :16] = g[:, 16:32]                             # the special matrices of the fixture among them
        want = O.depths(hd["model_view"], point, inst)
        _same_doubles(ctx.instance_depths(hd["model_view"], point, inst), want)
        if n == 0:
            assert ctx.L.trgl_instance_depths(ctx.h, api._dp(np.ascontiguousarray(hd["model_view"]).reshape(16)), api._dp(point), None, stride, 0,
                                              api.MEM_DEVICE, None) == 0
            continue
        # device memory, through the C ABI into a buffer that is longer than n: exactly n entries are written
        d_inst = _dev(inst)
        out = torch.full((n + 5,), float("nan"), dtype=torch.float64, device="cuda")
        _sync()
        mv = np.ascontiguousarray(hd["model_view"], np.float64).reshape(16)
        assert ctx.L.trgl_instance_depths(ctx.h, api._dp(mv), api._dp(point), d_inst.data_ptr(), stride, n, api.MEM_DEVICE, out.data_ptr()) == 0
        ctx.sync()
        got = out.cpu().numpy()
        assert (_bits(got[n:]) == NAN_BITS).all(), "depths behind n were written"
        _same_doubles(got[:n], want)
        got = ctx.instance_depths(hd["model_view"], point, d_inst, device=True)          # the binding: a tensor, not waited for
        ctx.sync()
        _same_doubles(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", OC.SIZES)
def test_order_equals_the_model(n, ctx64):
    import torch
    ctx, _ = ctx64
    d = OC.depths_of(n)
    for front in (False, True):
        want = O.order(d, int(front))
        assert np.array_equal(ctx.depth_order(d, front_to_back=front), want)
        if n == 0:
            assert ctx.L.trgl_depth_order(ctx.h, None, 0, int(front), api.MEM_DEVICE, None) == 0
            continue
        dd = _dev(d)
        out = torch.full((n + 5,), SENTINEL, dtype=torch.int32, device="cuda")
        _sync()
        assert ctx.L.trgl_depth_order(ctx.h, dd.data_ptr(), n, int(front), api.MEM_DEVICE, out.data_ptr()) == 0
        ctx.sync()
        got = out.cpu().numpy().view(np.uint32)
        assert (got[n:] == np.uint32(SENTINEL)).all(), "order entries behind n were written"
        assert np.array_equal(got[:n], want)
        got = ctx.depth_order(dd, front_to_back=front, device=True)
        ctx.sync()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    if n:
        assert np.array_equal(dd.cpu().numpy().view(np.uint64), d.view(np.uint64)), "the depths were written to"


# ---- the stage's rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_ordered_stage_rows_equal_the_model(name, camera, ctx64):
    import torch
    c = OC.CASES[name]
    hd, u = camera
    ctx, vs_of = ctx64
    verts, idx, inst, vis, fc, ic, order = OC.case_inputs(c)
    builtin = c.stage == "builtin"
    K = 24 if builtin else IC.STAGES[c.stage][1]
    drawn = O.visit(order, c.n, vis, skip_out_of_range=c.order == "out_of_range")
    if builtin:                                                      # the unordered model, fed instances[order]
        want_clip, want_vary, _ = M.builtin_rows(hd["model_view"], hd["projection"], verts, idx, inst[drawn], None)
    else:                                                            # in.instance (slot 0 of k5, slot 63 of k64) is the ORIGINAL number
        want_clip, want_vary = IC.expect_user(c.stage, hd["model_view"], hd["projection"], hd["key"], verts, idx, inst, drawn)
    want_col = M.colors(drawn, c.nf, fc, ic)
    rows = len(drawn) * c.nf
    vs = -1 if builtin else vs_of[c.stage]
    d_order = _dev(order) if c.order_device else order
    if c.inst_device:
        cap = len(order) * c.nf + 3
        out = (torch.full((cap, 12), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((cap, max(K, 1)), float("nan"), dtype=torch.float64, device="cuda") if K else None,
               torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda") if c.colors else None)
        a_inst, a_ic, a_vis = _dev(inst), _dev(ic), _dev_bytes(vis)
        _sync()
        clip, vary, col, n_out = ctx.instance_stage(vs, u, hd["projection"], verts, idx, instances=a_inst, face_colors=fc, instance_colors=a_ic,
                                                    visible=a_vis, instances_device=True, out=out, order=d_order, order_device=c.order_device)
        ctx.sync()
        clip, vary = clip.cpu().numpy(), None if vary is None else vary.cpu().numpy()
        col = None if col is None else col.cpu().numpy().view(np.uint32)
        assert n_out == rows
        assert (_bits(clip[rows:]) == NAN_BITS).all(), "clip rows behind n_out were written"
        assert vary is None or (_bits(vary[rows:]) == NAN_BITS).all(), "varyings behind n_out were written"
        assert col is None or (col[rows:] == np.uint32(SENTINEL)).all(), "colours behind n_out were written"
        clip, vary, col = clip[:rows], None if vary is None else vary[:rows], None if col is None else col[:rows]
    else:
        if c.order_device:
            _sync()
        clip, vary, col, n_out = ctx.instance_stage(vs, u, hd["projection"], verts, idx, instances=inst, face_colors=fc, instance_colors=ic,
                                                    visible=vis, order=d_order, order_device=c.order_device)
        assert n_out == rows and clip.shape == (rows, 12) and vary.shape == (rows, K)
    assert np.array_equal(_bits(clip), _bits(want_clip)), "clip rows differ from the model"
    if K:
        assert np.array_equal(_bits(vary), _bits(want_vary)), "varyings differ from the model"
    if want_col is None:
        assert col is None
    else:
        assert np.array_equal(col, want_col), "colours differ from the model"


# ---- frames: an ordered call against trgl_draw_instanced over arrays permuted on the host ------------------------------------------
N_FRAME = 40
MODES = {"one": {}, "halves": dict(halves=True), "strip": dict(strip=(5, 23)), "bands0": dict(interleave=(32, 0, 2)),
         "bands1": dict(interleave=(32, 1, 2))}
# kind name -> (stage, fragment kind or (source, K, may_discard, reads_dest, depth_write), which colours)
FRAME_KINDS = {
    "flat_instance_colors": ("k0", FLAT, "instance"),
    "phong_builtin": ("builtin", PHONG, None),
    "blend_over": ("k0", (B.OVER_SRC, 0, True, True, False), "instance"),
}


def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _frame_inputs(w, h):
    hd = scenes.head_standin(1, w, h)
    verts, idx = IC.cube(9, 0.5)
    inst = IC.instances(N_FRAME, 19, seed=77, spread=0.9, scale=(0.15, 0.4))
    vis = IC.visible("random", N_FRAME, seed=8)
    back = scenes.random_triangles(60, w, h, seed=41, rmin=4, rmax=30, perspective_w=True)
    order = O.order(O.depths(hd["model_view"], np.zeros(3), inst))
    order = np.concatenate([order, order[:5]])                       # a few instances twice
    return hd, verts, idx, inst, vis, back, order


def _draw_frame(kind_name, w, h, ordered, device=False, strip=None, interleave=None, halves=False):
    stage, frag, which = FRAME_KINDS[kind_name]
    hd, verts, idx, inst, vis, (bclip, bcol), order = _frame_inputs(w, h)
    d, n, sp = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], tex_diffuse=0, tex_normal=1, tex_specular=2)
    ic = IC.colors(N_FRAME, 9, alpha=isinstance(frag, tuple)) if which == "instance" else None
    with Context(w, h, 3) as ctx:
        kind = frag if isinstance(frag, int) else ctx.register_shader(frag[0], frag[1], frag[2], reads_dest=frag[3], depth_write=frag[4])
        vs = None if stage == "builtin" else ctx.register_vertex_shader(*IC.STAGES[stage])
        if strip:
            ctx.set_strip(*strip)
        if interleave:
            ctx.set_interleave(*interleave)
        for slot, t in enumerate((d, n, sp)):
            ctx.upload_texture(slot, t)
        ctx.draw(FLAT, bclip, colors=bcol)
        if ordered and device:
            a = (_dev(inst), _dev(ic), _dev_bytes(vis), _dev(order))
            _sync()
            ctx.draw_instanced(kind, u, hd["projection"], verts, idx, instances=a[0], vertex_shader=vs, instance_colors=a[1], visible=a[2],
                               instances_device=True, order=a[3], order_device=True)
        elif ordered:
            ctx.draw_instanced(kind, u, hd["projection"], verts, idx, instances=inst, vertex_shader=vs, instance_colors=ic, visible=vis, order=order)
        else:
            drawn = O.visit(order, N_FRAME, vis)
            ctx.draw_instanced(kind, u, hd["projection"], verts, idx, instances=inst[drawn], vertex_shader=vs,
                               instance_colors=None if ic is None else ic[drawn])
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        return _result(ctx)


@pytest.mark.parametrize("size", [(96, 64), (37, 29)])
@pytest.mark.parametrize("kind_name", sorted(FRAME_KINDS))
def test_ordered_frame_equals_the_draw_of_permuted_arrays(kind_name, size):
    w, h = size
    for name, kw in MODES.items():
        got, want = _draw_frame(kind_name, w, h, True, **kw), _draw_frame(kind_name, w, h, False, **kw)
        same(got, want, what=f"{kind_name} {w}x{h} {name}")
        if name == "one":
            assert got[2][1] > 0
            same(_draw_frame(kind_name, w, h, True, device=True), want, what=f"{kind_name} {w}x{h} device arrays")


def _quad_frame(w, h, shader, order_kind, device):
    """The scene of order_cases.quad_scene: the wall FLAT, then the quads under QUAD_VS in array order (order_kind None) or through
    instance_depths, depth_order and the ordered draw - with device=True all of it in device memory."""
    sc = OC.quad_scene(w, h)
    u = make_uniforms(sc["mv"])
    with Context(w, h, 3) as ctx:
        kind = ctx.register_shader(shader[0], 0, True, reads_dest=shader[1], depth_write=shader[2])
        vs = ctx.register_vertex_shader(OC.QUAD_VS, 0)
        ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
        inst, col = (_dev(sc["inst"]), _dev(sc["col"])) if device else (sc["inst"], sc["col"])
        if device:
            _sync()
        order = None
        if order_kind is not None:
            depths = ctx.instance_depths(sc["mv"], sc["point"], inst, device=device)
            order = ctx.depth_order(depths, front_to_back=order_kind == "front", device=device)
        ctx.draw_instanced(kind, u, sc["proj"], sc["verts"], sc["idx"], instances=inst, vertex_shader=vs, instance_colors=col,
                           instances_device=device, order=order, order_device=device and order is not None)
        return _result(ctx)


def test_translucent_scene_equals_the_blend_model_in_sorted_order():
    w, h = 96, 64
    sc = OC.quad_scene(w, h)
    n = len(sc["inst"])
    back = O.order(O.depths(sc["mv"], sc["point"], sc["inst"]))
    over = (B.OVER_SRC, True, False)
    want_sorted = OC.quad_model(w, h, B.f_over, False, back, "back")
    want_array = OC.quad_model(w, h, B.f_over, False, np.arange(n), "array")
    for device in (False, True):
        same(_quad_frame(w, h, over, "back", device), want_sorted, what=f"sorted, device={device}")
    same(_quad_frame(w, h, over, None, False), want_array, what="array order")
    assert not np.array_equal(want_sorted[0], want_array[0])


def test_front_to_back_runs_fewer_fragments_on_the_device():
    w, h = 96, 64
    sc = OC.quad_scene(w, h)
    d = O.depths(sc["mv"], sc["point"], sc["inst"])
    odd = (B.ODD_DISCARD_SRC, False, True)
    frags = {}
    for name, o in (("array", None), ("back", O.order(d)), ("front", O.order(d, O.FRONT_TO_BACK))):
        got = _quad_frame(w, h, odd, None if o is None else name, True)
        same(got, OC.quad_model(w, h, B.f_odd_discard, True, np.arange(len(d)) if o is None else o, name), what=name)
        frags[name] = got[2][1]
    assert frags["front"] < frags["array"] < frags["back"], frags


def test_occlusion_codes_depths_and_order_stay_on_the_device():
    """The codes trgl_occlusion_boxes leaves in device memory gate the instances, their depths and the order are made there, and the
    draw reads all three: nothing comes to the host but the count of drawn instances."""
    import torch
    w, h = 160, 100
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, w / h, 1.0, 30.0)
    wall_v = np.array([[-6.0, -4.0, 0.0], [0.0, -4.0, 0.0], [0.0, 4.0, 0.0], [-6.0, 4.0, 0.0]])
    wall, _ = V.expect_clip(mv, proj, np.concatenate([wall_v, np.zeros((4, 5))], 1), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    wall_col = np.array([0xFF808080, 0xFF808080], np.uint32)
    rng = scenes.SplitMix64(99)
    xs, ys = np.linspace(-2.6, 2.6, 8), np.linspace(-1.5, 1.5, 4)
    centres = np.array([[x, y, 0.0] for y in ys for x in xs])
    n = len(centres)
    centres[:, 2] = -3.0 - rng.uniform(n, 0.0, 2.0)                  # scattered depths behind the wall's plane, overlapping on screen
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10]] = 1.2
    inst[:, [3, 7, 11]] = centres
    inst[:, 15] = 1.0
    half = 0.6 * 1.25
    boxes = np.concatenate([centres - half, centres + half], 1)
    view_proj = M.mat_product(proj, mv).reshape(16)
    ic = IC.colors(n, 9)
    verts, idx = IC.cube(8, 0.5)
    u = make_uniforms(mv)
    with Context(w, h, 3) as ctx:
        vs = ctx.register_vertex_shader(OC.QUAD_VS, 0)
        ctx.draw(FLAT, wall, colors=wall_col)
        z_wall = ctx.read_zbuffer()
        d_boxes, d_inst, d_ic = torch.from_numpy(boxes).cuda(), _dev(inst), _dev(ic)
        _sync()
        codes = ctx.occlusion_boxes(view_proj, d_boxes, device=True)
        depths = ctx.instance_depths(mv, np.zeros(3), d_inst, device=True)
        order = ctx.depth_order(depths, front_to_back=True, device=True)
        ctx.draw_instanced(FLAT, u, proj, verts, idx, instances=d_inst, vertex_shader=vs, instance_colors=d_ic, visible=codes,
                           instances_device=True, order=order, order_device=True)
        got = _result(ctx)
        codes_h, order_h = codes.cpu().numpy(), order.cpu().numpy().view(np.uint32)
    want_codes = om.codes(z_wall, scenes.init_viewport(0, 0, w, h), view_proj, boxes)
    assert np.array_equal(codes_h, want_codes) and 0 < int((want_codes & 1).sum()) < n
    want_order = O.order(O.depths(mv, np.zeros(3), inst), O.FRONT_TO_BACK)
    assert np.array_equal(order_h, want_order)
    drawn = O.visit(want_order, n, want_codes)
    with Context(w, h, 3) as ctx:                                    # the same instances, permuted on the host, unordered
        vs = ctx.register_vertex_shader(OC.QUAD_VS, 0)
        ctx.draw(FLAT, wall, colors=wall_col)
        ctx.draw_instanced(FLAT, u, proj, verts, idx, instances=inst[drawn], vertex_shader=vs, instance_colors=ic[drawn])
        same(got, _result(ctx), what="codes, depths and order on the device")
    assert got[2][0] == 2 + 12 * len(drawn)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable():
    hd = scenes.head_standin(1, 64, 64)
    verts, idx = IC.cube(8, 0.5)
    inst = IC.instances(3, 16, seed=2)
    vis = np.array([1, 0, 1], np.uint8)
    order = np.array([2, 0, 1, 2], np.uint32)
    bad_order = np.array([2, 3, 0], np.uint32)
    pj = np.ascontiguousarray(hd["projection"], np.float64).reshape(16)
    mv = np.ascontiguousarray(hd["model_view"], np.float64).reshape(16)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
    d_order, d_inst = _dev(np.concatenate([order, order])), _dev(inst)
    d_depths = _dev(np.array([1.0, 2.0, 3.0, 4.0]))
    _sync()
    with Context(64, 64, 3) as ctx:
        base = dict(vs=-1, kind=PHONG, u=C.byref(u), pj=api._dp(pj), v=verts.ctypes.data, vstride=8, nv=8, i=idx.ctypes.data, nf=12, fc=None,
                    mmem=api.MEM_HOST, inst=inst.ctypes.data, istride=16, n=3, ic=None, vis=vis.ctypes.data, imem=api.MEM_HOST,
                    order=order.ctypes.data, n_order=4, omem=api.MEM_HOST)

        def call(**kw):
            a = dict(base, **kw)
            return ctx.L.trgl_draw_instanced_ordered(ctx.h, a["vs"], a["kind"], a["u"], a["pj"], a["v"], a["vstride"], a["nv"], a["i"], a["nf"], a["fc"],
                                                     a["mmem"], a["inst"], a["istride"], a["n"], a["ic"], a["vis"], a["imem"],
                                                     a["order"], a["n_order"], a["omem"])

        invalid = dict(null_order_with_count=dict(order=None), order_without_count=dict(n_order=0), bad_order_mem=dict(omem=5),
                       host_entry_out_of_range=dict(order=bad_order.ctypes.data, n_order=3),
                       misaligned_device_order=dict(order=d_order.data_ptr() + 2, omem=api.MEM_DEVICE),
                       null_vertices=dict(v=None), unknown_kind=dict(kind=999), kinds_differ=dict(kind=FLAT), instance_stride=dict(istride=15),
                       bad_instance_mem=dict(imem=-1))
        for name, kw in invalid.items():
            assert call(**kw) == E_INVALID, name
            assert ctx.L.trgl_last_error(ctx.h), name
        assert call(n_order=1 << 31, order=d_order.data_ptr(), omem=api.MEM_DEVICE) == E_UNSUPPORTED
        assert call(n=1 << 31, vis=None, inst=d_inst.data_ptr(), imem=api.MEM_DEVICE) == E_UNSUPPORTED
        # 2^31 triangles: a device list that names one instance often enough
        assert call(order=None, n_order=0, omem=api.MEM_HOST, n=(1 << 31) // 12 + 1, vis=None, inst=d_inst.data_ptr(), imem=api.MEM_DEVICE) == E_UNSUPPORTED
        # depths and order in device memory
        out = d_depths.data_ptr()
        assert ctx.L.trgl_instance_depths(ctx.h, api._dp(mv), api._dp(np.zeros(3)), d_inst.data_ptr() + 4, 16, 3, api.MEM_DEVICE, out) == E_INVALID
        assert ctx.L.trgl_instance_depths(ctx.h, api._dp(mv), api._dp(np.zeros(3)), d_inst.data_ptr(), 15, 3, api.MEM_DEVICE, out) == E_INVALID
        assert ctx.L.trgl_instance_depths(ctx.h, api._dp(mv), api._dp(np.zeros(3)), d_inst.data_ptr(), 16, 1 << 31, api.MEM_DEVICE, out) == E_UNSUPPORTED
        assert ctx.L.trgl_depth_order(ctx.h, d_depths.data_ptr(), 4, 2, api.MEM_DEVICE, d_order.data_ptr()) == E_INVALID
        assert ctx.L.trgl_depth_order(ctx.h, d_depths.data_ptr() + 4, 3, 0, api.MEM_DEVICE, d_order.data_ptr()) == E_INVALID
        assert ctx.L.trgl_depth_order(ctx.h, d_depths.data_ptr(), 4, 0, api.MEM_DEVICE, d_order.data_ptr() + 2) == E_INVALID
        assert ctx.L.trgl_depth_order(ctx.h, d_depths.data_ptr(), 1 << 31, 0, api.MEM_DEVICE, d_order.data_ptr()) == E_UNSUPPORTED
        # nothing to draw: fine, and nothing is read
        assert call(n=0, inst=None, vis=None) == 0
        assert call(nf=0) == 0
        # a null list with no entries is trgl_draw_instanced
        assert ctx.stats()[0] == 0
        assert call(order=None, n_order=0) == 0
        got_plain = _result(ctx)
    with Context(64, 64, 3) as ctx:
        ctx.draw_instanced(PHONG, u, hd["projection"], verts, idx, instances=inst, visible=vis)
        same(got_plain, _result(ctx), what="a null list after the refused calls")
    with Context(64, 64, 3) as ctx:                                  # and after a refusal an ordered draw is what a fresh context draws
        assert ctx.L.trgl_draw_instanced_ordered(ctx.h, -1, PHONG, C.byref(u), api._dp(pj), verts.ctypes.data, 8, 8, idx.ctypes.data, 12, None,
                                                 api.MEM_HOST, inst.ctypes.data, 16, 3, None, vis.ctypes.data, api.MEM_HOST,
                                                 bad_order.ctypes.data, 3, api.MEM_HOST) == E_INVALID
        ctx.draw_instanced(PHONG, u, hd["projection"], verts, idx, instances=inst, visible=vis, order=order)
        got = _result(ctx)
    drawn = O.visit(order, 3, vis)
    clip, vary, _ = M.builtin_rows(hd["model_view"], hd["projection"], verts, idx, inst[drawn], None)
    case = cases.make_case(64, 64, [(PHONG, u, clip, vary, None)])
    same(got, cases.run_oracle(case), what="after the refused call, against the oracle")
    assert got[2][0] == 12 * len(drawn) == 36
