"""Instanced draws on the GPU (include/trgl.h: trgl_draw_instanced, trgl_instance_stage; kernels_instance.hip and the second kernel of
vertex_user.h).

The stage's rows equal tests/instance_model.py bit for bit - built-in stage and user vertex shaders, every visibility pattern, host
and device arrays - and nothing behind the rows it reports is written.  A frame drawn by one instanced call equals the frame of the
loop it replaces (the vertex stage and a draw per visible instance): bytes, depths, counters and the stats line, whole and on strips
and bands.  Submission order holds, one call is one flush, and the codes trgl_occlusion_boxes leaves in device memory gate the
instances without a trip to the host."""
import ctypes as C

import numpy as np
import pytest

import blend_model as B
import cases
import instance_model as M
import instanced_cases as IC
import occlusion_model as om
import vertex_shader_sources as V
from oracle import orc
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, make_uniforms

pytestmark = pytest.mark.gpu
same = cases.assert_same_frame
E_INVALID, E_UNSUPPORTED = -1, -5
NAN_BITS = np.float64(np.nan).view(np.uint64)
SENTINEL = 0x5EA7BEEF                       # what the colour outputs hold before the call


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a):
    return None if a is None else cases.device_array(a)


def _sync():
    import torch
    torch.cuda.synchronize()                 # uploads run on torch's stream; a context's own stream is not ordered behind it


@pytest.fixture(scope="module")
def camera():
    hd = scenes.head_standin(1, 64, 64)
    return hd, make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])


@pytest.fixture(scope="module")
def stage_ctx():
    with Context(64, 64, 3) as ctx:
        vs = {name: ctx.register_vertex_shader(src, K) for name, (src, K) in IC.STAGES.items()}
        yield ctx, vs


# ---- the stage's rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.SHAPES))
def test_stage_rows_equal_the_model(name, camera, stage_ctx):
    import torch
    s = IC.SHAPES[name]
    hd, u = camera
    ctx, vs_of = stage_ctx
    verts, idx, inst, vis, fc, ic = IC.shape_inputs(s)
    builtin = s.stage == "builtin"
    K = 24 if builtin else IC.STAGES[s.stage][1]
    if builtin:
        want_clip, want_vary, drawn = M.builtin_rows(hd["model_view"], hd["projection"], verts, idx, inst, vis)
    else:
        drawn = M.compact(vis, s.n)
        want_clip, want_vary = IC.expect_user(s.stage, hd["model_view"], hd["projection"], hd["key"], verts, idx, inst, drawn)
    want_col = M.colors(drawn, s.nf, fc, ic)
    rows = len(drawn) * s.nf
    mesh_device = s.nf in (12, 65)                               # the mesh's memory kind is its own
    mv, mi, mfc = (_dev(verts), _dev(idx), _dev(fc)) if mesh_device else (verts, idx, fc)
    vs = -1 if builtin else vs_of[s.stage]
    if s.inst_device:
        cap = s.n * s.nf + 3                                     # room for every instance, and rows nobody may touch
        out = (torch.full((cap, 12), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((cap, max(K, 1)), float("nan"), dtype=torch.float64, device="cuda") if K else None,
               torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda") if s.colors else None)
        args = dict(instances=_dev(inst), instance_colors=_dev(ic) if s.n else None, visible=None if vis is None or not s.n else torch.from_numpy(vis).cuda())
        _sync()
        clip, vary, col, n_out = ctx.instance_stage(vs, u, hd["projection"], mv, mi, face_colors=mfc, device=mesh_device,
                                                    instances_device=True, out=out, **args) if s.n else _empty_device_call(ctx, vs, u, hd, mv, mi, mesh_device, out)
        ctx.sync()
        clip, vary = clip.cpu().numpy(), None if vary is None else vary.cpu().numpy()
        col = None if col is None else col.cpu().numpy().view(np.uint32)
        assert n_out == rows
        assert (_bits(clip[rows:]) == NAN_BITS).all(), "clip rows behind n_out were written"
        assert vary is None or (_bits(vary[rows:]) == NAN_BITS).all(), "varyings behind n_out were written"
        assert col is None or (col[rows:] == np.uint32(SENTINEL)).all(), "colours behind n_out were written"
        clip, vary, col = clip[:rows], None if vary is None else vary[:rows], None if col is None else col[:rows]
    else:
        if mesh_device:
            _sync()
        clip, vary, col, n_out = ctx.instance_stage(vs, u, hd["projection"], mv, mi, instances=inst, face_colors=mfc, instance_colors=ic,
                                                    visible=vis, device=mesh_device)
        assert n_out == rows and clip.shape == (rows, 12) and vary.shape == (rows, K)
    assert np.array_equal(_bits(clip), _bits(want_clip)), "clip rows differ from the model"
    if K:
        assert np.array_equal(_bits(vary), _bits(want_vary)), "varyings differ from the model"
    if want_col is None:
        assert col is None
    else:
        assert np.array_equal(col, want_col), "colours differ from the model"


def _empty_device_call(ctx, vs, u, hd, mv, mi, mesh_device, out):
    """n_instances = 0 in device memory: torch hands out no address for an empty tensor, so the C ABI is called with the pointers
    null and the stride the shape names - nothing may be read or written."""
    n_out = C.c_uint64(77)
    pj = np.ascontiguousarray(hd["projection"], np.float64).reshape(16)
    rc = ctx.L.trgl_instance_stage(ctx.h, vs, C.byref(u), api._dp(pj), api._ptr(mv), mv.shape[1], mv.shape[0], api._ptr(mi), mi.shape[0], None,
                                   api.MEM_DEVICE if mesh_device else api.MEM_HOST, None, 16, 0, None, None, api.MEM_DEVICE,
                                   out[0].data_ptr(), None if out[1] is None else out[1].data_ptr(), None if out[2] is None else out[2].data_ptr(),
                                   C.byref(n_out))
    assert rc == 0, ctx.L.trgl_last_error(ctx.h)
    return out[0], out[1], out[2], int(n_out.value)


# ---- frames: one instanced call against the loop it replaces ----------------------------------------------------------------
W, H = 320, 200
MODES = {"one": {}, "halves": dict(halves=True), "strip": dict(strip=(37, 131)), "bands0": dict(interleave=(32, 0, 2)),
         "bands1": dict(interleave=(32, 1, 2))}
N_FRAME = 40


def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _frame_scene(kind_name):
    hd = scenes.head_standin(1, W, H)
    verts, idx = IC.cube(9, 0.5)
    inst = IC.instances(N_FRAME, 19, seed=77, spread=0.9, scale=(0.15, 0.4))
    vis = IC.visible("random", N_FRAME, seed=8)
    assert 10 <= int((vis & 1).sum()) <= 30
    back = scenes.random_triangles(120, W, H, seed=41, rmin=6, rmax=70, perspective_w=True)
    return hd, verts, idx, inst, vis, back


# kind name -> (stage, fragment kind or (source, K, may_discard, reads_dest), which colours)
FRAME_KINDS = {
    "flat_instance_colors": ("k0", FLAT, "instance"),
    "gouraud_user_vs": ("k3", GOURAUD, "face"),
    "phong_builtin": ("builtin", PHONG, None),
    "blend_reads_dest": ("k0", (B.ALPHA_TEST_SRC, 0, True, True), "instance"),
}


def _draw_frame(kind_name, instanced, strip=None, interleave=None, halves=False, device=False):
    stage, frag, which = FRAME_KINDS[kind_name]
    hd, verts, idx, inst, vis, (bclip, bcol) = _frame_scene(kind_name)
    d, n, sp = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], tex_diffuse=0, tex_normal=1, tex_specular=2)
    fc = IC.colors(12, 7) if which == "face" else None
    ic = IC.colors(N_FRAME, 9, alpha=isinstance(frag, tuple)) if which == "instance" else None
    with Context(W, H, 3) as ctx:
        kind = frag if isinstance(frag, int) else ctx.register_shader(frag[0], frag[1], frag[2], reads_dest=frag[3])
        vs = None if stage == "builtin" else ctx.register_vertex_shader(*IC.STAGES[stage])
        if strip:
            ctx.set_strip(*strip)
        if interleave:
            ctx.set_interleave(*interleave)
        for slot, t in enumerate((d, n, sp)):
            ctx.upload_texture(slot, t)
        ctx.draw(FLAT, bclip, colors=bcol)                       # something underneath, so that order and depth show
        if instanced:
            a = (verts, idx, inst, fc, ic, vis)
            if device:
                import torch
                a = (_dev(verts), _dev(idx), _dev(inst), _dev(fc), _dev(ic), torch.from_numpy(vis).cuda())
                _sync()
            ctx.draw_instanced(kind, u, hd["projection"], a[0], a[1], instances=a[2], vertex_shader=vs, face_colors=a[3],
                               instance_colors=a[4], visible=a[5], device=device, instances_device=device)
        else:
            for i in M.compact(vis, N_FRAME):
                if stage == "builtin":                           # trgl_vertex_stage under MV_i, then trgl_draw under the call's uniforms
                    ui = make_uniforms(M.mat_product(hd["model_view"], inst[i, :16]), hd["key"], hd["fill"], hd["rim"])
                    clip, vary = ctx.vertex_stage(-1, ui, hd["projection"], verts, idx)
                else:                                            # (the plain vertex stage cannot tell a shader its instance: the model's rows)
                    clip, vary = IC.expect_user(stage, hd["model_view"], hd["projection"], hd["key"], verts, idx, inst, [i])
                ctx.draw(kind, clip, vary, M.colors([i], 12, fc, ic), u)
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        return _result(ctx)


@pytest.mark.parametrize("kind_name", sorted(FRAME_KINDS))
def test_instanced_frame_equals_the_loop(kind_name):
    for name, kw in MODES.items():
        got, want = _draw_frame(kind_name, True, **kw), _draw_frame(kind_name, False, **kw)
        same(got, want, what=f"{kind_name} {name}")
        assert got[2][1] > 0
    same(_draw_frame(kind_name, True, device=True), _draw_frame(kind_name, False), what=f"{kind_name} device arrays")


def test_small_instanced_frame_equals_the_oracle():
    hd, verts, idx, inst, vis, (bclip, bcol) = _frame_scene("flat_instance_colors")
    ic = IC.colors(N_FRAME, 9)
    drawn = M.compact(vis, N_FRAME)
    clip, _ = IC.expect_user("k0", hd["model_view"], hd["projection"], hd["key"], verts, idx, inst, drawn)
    case = cases.make_case(W, H, [(FLAT, None, bclip, None, bcol), (FLAT, None, clip, None, M.colors(drawn, 12, None, ic))])
    same(_draw_frame("flat_instance_colors", True), cases.run_oracle(case), what="instanced FLAT against the oracle")


# ---- order, flushes ------------------------------------------------------------------------------------------------------------
def test_submission_order_is_instance_order():
    """Two instances with the same matrix: z ties keep the earlier triangle (our_gl.cpp:165), so the first colour shows - and the second
    once the first is not drawn."""
    hd = scenes.head_standin(1, 64, 64)
    verts, idx = IC.cube(9, 0.5)
    inst = np.repeat(IC.instances(1, 16, seed=5), 2, 0)
    first, second = 0xFF2040F0, 0xFF80C010
    ic = np.array([first, second], np.uint32)

    def shown(vis):
        with Context(64, 64, 3) as ctx:
            vs = ctx.register_vertex_shader(IC.MOVE, 0)
            ctx.draw_instanced(FLAT, make_uniforms(hd["model_view"]), hd["projection"], verts, idx, instances=inst, vertex_shader=vs,
                               instance_colors=ic, visible=vis)
            fb, z = ctx.read_framebuffer(), ctx.read_zbuffer()
        covered = np.isfinite(z)
        assert covered.sum() > 50
        px = fb[covered].astype(np.uint32)
        return set((px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)).tolist())

    assert shown(None) == {first & 0xFFFFFF}
    assert shown(np.array([1, 1], np.uint8)) == {first & 0xFFFFFF}
    assert shown(np.array([0, 1], np.uint8)) == {second & 0xFFFFFF}


def test_200_instances_are_one_flush():
    """One call queues one draw: 200 boxes are one flush of 2400 triangles (a draw call per box would have met TRGL_MAX_DRAWS = 64
    three times on the way)."""
    hd = scenes.head_standin(1, 128, 96)
    verts, idx = IC.cube(8, 0.5)
    inst = IC.instances(200, 16, seed=31)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
    with Context(128, 96, 3) as ctx:
        ctx.set_profiling(True)
        ctx.draw_instanced(PHONG, u, hd["projection"], verts, idx, instances=inst)
        ctx.flush()
        ctx.sync()
        info = ctx.last_flush_info()
        _, flushes = ctx.phase_ms()
        assert info["triangles"] == 200 * 12 and flushes == 1, (info, flushes)
        assert ctx.stats()[0] == 200 * 12
    with Context(128, 96, 3) as ctx:                             # the loop, for comparison: its last flush holds the remainder only
        ctx.set_profiling(True)
        for i in range(200):
            ui = make_uniforms(M.mat_product(hd["model_view"], inst[i]), hd["key"], hd["fill"], hd["rim"])
            ctx.draw_indexed(PHONG, ui, hd["projection"], verts, idx)
        ctx.flush()
        ctx.sync()
        assert ctx.phase_ms()[1] == 4 and ctx.last_flush_info()["triangles"] == (200 - 3 * 64) * 12


# ---- occlusion codes straight into the draw ------------------------------------------------------------------------------------
def _occlusion_scene():
    w, h = 320, 200
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, w / h, 1.0, 30.0)
    # the wall: the left half of the view at z = 0
    wall_v = np.array([[-6.0, -4.0, 0.0], [0.0, -4.0, 0.0], [0.0, 4.0, 0.0], [-6.0, 4.0, 0.0]])
    wall_clip, _ = V.expect_clip(mv, proj, np.concatenate([wall_v, np.zeros((4, 5))], 1), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    # cubes of side 0.3 on a grid at z = -3, three units behind the wall's plane: the left ones far inside its shadow
    xs, ys = np.linspace(-2.6, 2.6, 12), np.linspace(-1.5, 1.5, 6)
    centres = np.array([[x, y, -3.0] for y in ys for x in xs])
    n = len(centres)
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10]] = 0.3                                   # the unit cube (half = 0.5) scaled to side 0.3
    inst[:, [3, 7, 11]] = centres
    inst[:, 15] = 1.0
    half = 0.15 * 1.25                                          # the box: the cube and a quarter more on every side
    boxes = np.concatenate([centres - half, centres + half], 1)
    return dict(w=w, h=h, mv=mv, proj=proj, wall=wall_clip, inst=inst, boxes=boxes, view_proj=M.mat_product(proj, mv).reshape(16))


def test_occlusion_codes_gate_the_instances_on_the_device():
    import torch
    sc = _occlusion_scene()
    verts, idx = IC.cube(8, 0.5)
    u = make_uniforms(sc["mv"])
    wall_col = np.array([0xFF808080, 0xFF808080], np.uint32)
    n = len(sc["inst"])

    def frame(gated):
        with Context(sc["w"], sc["h"], 3) as ctx:
            ctx.draw(FLAT, sc["wall"], colors=wall_col)
            codes = None
            if gated:
                boxes = torch.from_numpy(sc["boxes"]).cuda()
                d_inst = _dev(sc["inst"])
                _sync()
                codes = ctx.occlusion_boxes(sc["view_proj"], boxes, device=True)            # left in device memory, not waited for
                ctx.draw_instanced(PHONG, u, sc["proj"], verts, idx, instances=d_inst, visible=codes, instances_device=True)
            else:
                ctx.draw_instanced(PHONG, u, sc["proj"], verts, idx, instances=sc["inst"])
            res = _result(ctx)
            return res, None if codes is None else codes.cpu().numpy()

    (fb_all, z_all, st_all, _), _ = frame(False)
    # the CPU side: the model's codes against the wall's depths have both kinds in numbers
    with Context(sc["w"], sc["h"], 3) as ctx:
        ctx.draw(FLAT, sc["wall"], colors=wall_col)
        z_wall = ctx.read_zbuffer()
        viewport = scenes.init_viewport(0, 0, sc["w"], sc["h"])
    want = om.codes(z_wall, viewport, sc["view_proj"], sc["boxes"])
    assert (want == om.HIDDEN).sum() >= n // 4 and (want == om.VISIBLE).sum() >= n // 4, np.bincount(want, minlength=4)
    (fb, z, st, _), codes = frame(True)
    assert np.array_equal(codes, want)
    assert np.array_equal(fb, fb_all) and np.array_equal(z.view(np.uint64), z_all.view(np.uint64))
    assert st[1] == st_all[1], "fragments_drawn differs: a skipped instance had a fragment to give"
    assert st[0] == 2 + 12 * int((codes & 1).sum()) and st_all[0] == 2 + 12 * n


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable():
    hd = scenes.head_standin(1, 64, 64)
    verts, idx = IC.cube(8, 0.5)
    inst = IC.instances(3, 16, seed=2)
    vis = np.array([1, 0, 1], np.uint8)
    fc, ic = IC.colors(12, 7), IC.colors(3, 9)
    pj = np.ascontiguousarray(hd["projection"], np.float64).reshape(16)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
    bad_idx = idx.copy(); bad_idx[7, 1] = 8
    dev_inst = _dev(inst)
    _sync()
    with Context(64, 64, 3) as ctx:
        k0 = ctx.register_vertex_shader(IC.MOVE, 0)
        base = dict(vs=-1, kind=PHONG, u=C.byref(u), pj=api._dp(pj), v=verts.ctypes.data, vstride=8, nv=8, i=idx.ctypes.data, nf=12, fc=None,
                    mmem=api.MEM_HOST, inst=inst.ctypes.data, istride=16, n=3, ic=None, vis=vis.ctypes.data, imem=api.MEM_HOST)

        def call(**kw):
            a = dict(base, **kw)
            return ctx.L.trgl_draw_instanced(ctx.h, a["vs"], a["kind"], a["u"], a["pj"], a["v"], a["vstride"], a["nv"], a["i"], a["nf"], a["fc"],
                                             a["mmem"], a["inst"], a["istride"], a["n"], a["ic"], a["vis"], a["imem"])

        invalid = dict(null_vertices=dict(v=None), null_indices=dict(i=None), null_projection=dict(pj=None), unknown_vs=dict(vs=7),
                       unknown_vs_negative=dict(vs=-2), unknown_kind=dict(kind=999), kinds_differ_builtin=dict(kind=FLAT),
                       kinds_differ_user=dict(vs=k0, kind=GOURAUD), bad_mesh_mem=dict(mmem=7), bad_instance_mem=dict(imem=-1),
                       vertex_stride=dict(vstride=7), instance_stride_builtin=dict(istride=15), instance_stride_user=dict(vs=k0, kind=FLAT, istride=-1),
                       null_instances=dict(inst=None), instances_without_stride=dict(vs=k0, kind=FLAT, istride=0),
                       both_colors=dict(fc=fc.ctypes.data, ic=ic.ctypes.data), index_out_of_range=dict(i=bad_idx.ctypes.data),
                       no_uniforms_builtin=dict(u=None))
        for name, kw in invalid.items():
            assert call(**kw) == E_INVALID, name
            assert ctx.L.trgl_last_error(ctx.h), name
        unsupported = dict(too_many_instances=dict(n=1 << 31, vis=None, inst=dev_inst.data_ptr(), imem=api.MEM_DEVICE),
                           too_many_triangles=dict(n=(1 << 31) // 12 + 1, vis=None, inst=dev_inst.data_ptr(), imem=api.MEM_DEVICE))
        for name, kw in unsupported.items():
            assert call(**kw) == E_UNSUPPORTED, name
        # nothing to draw: fine, and nothing is read (the pointers are not even there)
        assert call(n=0, inst=None, vis=None) == 0
        assert call(nf=0, i=bad_idx.ctypes.data) == 0
        n_out = C.c_uint64(5)
        stage = (ctx.h, -1, C.byref(u), api._dp(pj), verts.ctypes.data, 8, 8, idx.ctypes.data, 12, None, api.MEM_HOST, inst.ctypes.data, 16, 3, None,
                 vis.ctypes.data, api.MEM_HOST)
        assert ctx.L.trgl_instance_stage(*stage, None, None, None, C.byref(n_out)) == E_INVALID and n_out.value == 0      # null outputs
        clip = np.zeros((36, 12))
        assert ctx.L.trgl_instance_stage(*stage, clip.ctypes.data, clip.ctypes.data, None, None) == E_INVALID            # null n_out
        assert ctx.stats()[0] == 0
        # and the context draws what a fresh one draws
        ctx.draw_instanced(PHONG, u, hd["projection"], verts, idx, instances=inst, visible=vis)
        got = _result(ctx)
    with Context(64, 64, 3) as ctx:
        ctx.register_vertex_shader(IC.MOVE, 0)
        ctx.draw_instanced(PHONG, u, hd["projection"], verts, idx, instances=inst, visible=vis)
        same(got, _result(ctx), what="after the refused calls")
    clip, vary, _ = M.builtin_rows(hd["model_view"], hd["projection"], verts, idx, inst, vis)
    case = cases.make_case(64, 64, [(PHONG, u, clip, vary, None)])
    same(got, cases.run_oracle(case), what="after the refused calls, against the oracle")
    assert got[2][0] == 24
