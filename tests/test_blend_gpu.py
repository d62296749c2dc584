"""User shaders that blend, on the GPU (include/trgl.h, TRGL_SHADER_READS_DEST and TRGL_SHADER_NO_DEPTH_WRITE): the run-time raster
kernel hands trgl_fragment the pixel it is drawn over and can leave the depth alone.  Kinds that use neither give what they gave
with TRGL_SHADER_MAY_DISCARD alone; kinds that blend equal the immediate-mode model of blend_model.py - frame bytes, z bits and
the print_render_stats() line - over clears, loaded frames, earlier flushes of any kind, strips and bands."""
import numpy as np
import pytest

import blend_model as B
import cases
import discard_shader_sources as D
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

same = cases.assert_same_frame


def kind(src, K=0, flags=5):
    """A user kind in a draw list: (source, K, flag word)."""
    return (src, K, flags)


def render(case, strip=None, interleave=None, flush_after=(), halves=False, split=None, start=None, between=None):
    """cases.run_gpu for draws whose kind may be a (source, K, flag word) tuple; returns (fb, z, stats tuple, stats line).
    flush_after: indices of draws followed by a flush; between = (i, f): f(ctx) runs after draw i."""
    with Context(case["width"], case["height"], case["bpp"]) as ctx:
        user = {}
        for k in dict.fromkeys(d[0] for d in case["draws"] if isinstance(d[0], tuple)):
            user[k] = ctx.register_shader(k[0], k[1], bool(k[2] & 1), reads_dest=bool(k[2] & 4), depth_write=not k[2] & 8)
        ctx.set_viewport(case["viewport"])
        if start is None:
            ctx.clear(case["clear"], case["zclear"])
        else:
            ctx.write_framebuffer(start[0])
            ctx.write_zbuffer(start[1])
        if strip is not None:
            ctx.set_strip(*strip)
        if interleave is not None:
            ctx.set_interleave(*interleave)
        for slot, t in case["textures"].items():
            ctx.upload_texture(slot, t)
        for i, (k, u, clip, vary, col) in enumerate(case["draws"]):
            n = clip.shape[0]
            edges = [n * j // (split or 1) for j in range((split or 1) + 1)]
            for a, b in zip(edges[:-1], edges[1:]):
                ctx.draw(user.get(k, k), clip[a:b], None if vary is None else vary[a:b], None if col is None else col[a:b], u)
                if split:
                    ctx.flush()
            if i in flush_after:
                ctx.flush()
            if between is not None and between[0] == i:
                between[1](ctx)
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def frame_case(name, draws_of):
    """cases.make_case of B.FRAMES[name]; draws_of(clip, col) gives the draws."""
    cfg, clip, col = B.frame(name)
    return cases.make_case(cfg["w"], cfg["h"], draws_of(clip, col), bpp=cfg["bpp"], viewport=cfg["viewport"], clear=cfg["clear"], zclear=cfg["zclear"])


def one(src, flags):
    return lambda clip, col: [(kind(src, 0, flags), None, clip, None, col)]


# ---- kinds that use neither flag's effect: what TRGL_SHADER_MAY_DISCARD alone gives ---------------------------------------------
RESTATED = {"checker_256": (D.CHECKER, 0), "gouraud_256_rgba": (D.GOURAUD, 3), "phong_nomaps_256": (D.PHONG, 24)}


def with_kind(case, src, K, flags):
    return dict(case, draws=[(kind(src, K, flags),) + d[1:] for d in case["draws"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RESTATED))
def test_reads_dest_changes_nothing_for_a_source_that_ignores_dst(name):
    case = cases.CASES[name]()
    same(render(with_kind(case, *RESTATED[name], 5)), render(with_kind(case, *RESTATED[name], 1)), what=name)


def back_to_front(case):
    """The case with triangle i moved to the constant NDC depth 0.9 - i * 1e-4 (clip z = depth * w; x, y and w, and with them the
    barycentrics, stay): every later fragment is nearer than all before it."""
    (k, u, clip, vary, col), = case["draws"]
    clip = clip.copy()
    depth = 0.9 - 1e-4 * np.arange(clip.shape[0])
    for v in range(3):
        clip[:, 4 * v + 2] = depth * clip[:, 4 * v + 3]
    return dict(case, draws=[(k, u, clip, vary, col)])


@pytest.mark.gpu
def test_no_depth_write_checker_equals_depth_writes_and_leaves_the_clear_depth():
    """checker_256 with TRGL_SHADER_NO_DEPTH_WRITE against TRGL_SHADER_MAY_DISCARD alone: the same colours and stats line, the z-buffer
    still at its clear value.  Without depth writes every fragment is tested against the clear depth, so the two can only agree
    where depth writes reject nothing either: the case's triangles are drawn back to front (back_to_front: their x, y, w and so
    the checker cells are the case's).  On the case as it is, where depth writes do reject, the flag must draw more fragments."""
    case = cases.checker_256()
    assert case["zclear"] == np.inf
    sorted_case = back_to_front(case)
    got, want = render(with_kind(sorted_case, D.CHECKER, 0, 9)), render(with_kind(sorted_case, D.CHECKER, 0, 1))
    assert (got[0] == want[0]).all(), "colours differ"
    assert got[2] == want[2] and got[3] == want[3]
    assert (got[1] == np.inf).all() and not (want[1] == np.inf).all()
    got, want = render(with_kind(case, D.CHECKER, 0, 9)), render(with_kind(case, D.CHECKER, 0, 1))
    assert (got[1] == np.inf).all()
    assert got[2][0] == want[2][0] and got[2][2:6] == want[2][2:6] and got[2][1] > want[2][1]


# ---- against the model ----------------------------------------------------------------------------------------------------------
VARIANTS = {"over_5": (B.OVER_SRC, 5, B.f_over, True), "over_13": (B.OVER_SRC, 13, B.f_over, False),
            "alpha_test_5": (B.ALPHA_TEST_SRC, 5, B.f_alpha_test, True), "alpha_test_13": (B.ALPHA_TEST_SRC, 13, B.f_alpha_test, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(B.FRAMES))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_blending_equals_the_model(name, variant):
    src, flags, fn, depth_write = VARIANTS[variant]
    same(render(frame_case(name, one(src, flags))), B.model_frame(name, fn, depth_write), what=f"{name} {variant}")


@pytest.mark.gpu
def test_dst_is_zero_without_the_flag():
    """The additive shader without TRGL_SHADER_READS_DEST adds to 0: the source colour, with or without depth writes."""
    for flags, depth_write in ((1, True), (9, False)):
        same(render(frame_case("96x64_bpp4", one(B.ADD_SRC, flags))), B.model_frame("96x64_bpp4", B.f_source, depth_write), what=f"flags {flags}")


@pytest.mark.gpu
@pytest.mark.parametrize("name, src, fn", [("96x64_bpp3", B.PROBE_BPP3_SRC, B.f_probe_bpp3), ("96x64_bpp1", B.PROBE_BPP1_SRC, B.f_probe_bpp1)],
                         ids=["bpp3", "bpp1"])
@pytest.mark.parametrize("flags", [5, 13])
def test_bytes_above_the_frame_read_back_as_zero(name, src, fn, flags):
    """The shader returns 0xAA in the bytes a 3-byte (1-byte) frame does not have and puts what dst holds there into the blue byte: the
    next fragment at the pixel reads 0 there, not 0xAA, so blue is 0 everywhere (test_blend_model: the scene reaches the case)."""
    got = render(frame_case(name, one(src, flags)))
    assert (got[0][..., 0] == 0).all()
    same(got, B.model_frame(name, fn, not flags & 8), what=name)


# ---- flush boundaries -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [5, 13])
def test_flush_boundaries_do_not_show(flags):
    """Two draws of one kind in one flush, as flush_begin / flush_end, with a flush between them and in four flushes: the later flushes
    read the pixels the earlier ones left, not a clear."""
    two = lambda clip, col: [(kind(B.OVER_SRC, 0, flags), None, clip[:130], None, col[:130]), (kind(B.OVER_SRC, 0, flags), None, clip[130:], None, col[130:])]
    for name in ("96x64_bpp3", "101x67_viewport_zclear"):
        case = frame_case(name, two)
        want = B.model_frame(name, B.f_over, not flags & 8)
        for mode in ({}, dict(halves=True), dict(flush_after=(0,)), dict(split=2)):
            same(render(case, **mode), want, what=f"{name} flags {flags} {mode}")


def model_from(case, start, stats0, draws):
    m = B.Model(case["width"], case["height"], case["bpp"], viewport=case["viewport"], start=start, stats0=stats0)
    for clip, col, fn, depth_write in draws:
        m.draw(clip, col, fn, depth_write)
    return m.result()


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_over_a_frame_put_in_with_write_framebuffer(bpp):
    name = f"96x64_bpp{bpp}"
    start = cases.loaded_buffers(96, 64, bpp)
    for flags in (5, 13):
        case = frame_case(name, one(B.OVER_SRC, flags))
        (_, _, clip, _, col), = case["draws"]
        same(render(case, start=start), model_from(case, start, None, [(clip, col, B.f_over, not flags & 8)]), what=f"{name} flags {flags}")


def phong_then(w, h, draws_of):
    """A small PHONG head, then draws_of(clip, col) over it (120 translucent triangles)."""
    hd = scenes.head_standin(2, w, h)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.5, -1, -1, -1)
    clip, col = B.scene(w, h, 120, 7301)
    return cases.make_case(w, h, [(PHONG, u, hd["clip"], hd["varyings"], None)] + draws_of(clip, col)), clip, col


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [5, 13])
def test_over_a_phong_draw_in_the_same_context(flags):
    """trgl_draw cuts the flush where the blending kind meets PHONG; dst is what k_shade wrote."""
    case, clip, col = phong_then(128, 96, one(B.OVER_SRC, flags))
    base = render(dict(case, draws=case["draws"][:1]))
    assert base[2][1] > 0
    same(render(case), model_from(case, base[:2], base[2], [(clip, col, B.f_over, not flags & 8)]), what=f"flags {flags}")


@pytest.mark.gpu
def test_over_a_blurred_frame():
    """Opaque FLAT triangles, framebuffer_blur, then the blending kind: dst is the blurred pixel."""
    cfg, clip, col = B.frame("96x64_bpp3")
    opaque = cases.make_case(96, 64, [(FLAT, None, clip[:60], None, col[:60])], bpp=3, clear=cfg["clear"])
    with Context(96, 64, 3) as ctx:
        ctx.clear(cfg["clear"], np.inf)
        ctx.draw(FLAT, clip[:60], None, col[:60])
        ctx.framebuffer_blur(2)
        base = ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()
    assert (base[0] != render(opaque)[0]).any()
    case = dict(opaque, draws=opaque["draws"] + [(kind(B.OVER_SRC, 0, 13), None, clip[60:], None, col[60:])])
    got = render(case, between=(0, lambda ctx: ctx.framebuffer_blur(2)))
    same(got, model_from(case, base[:2], base[2], [(clip[60:], col[60:], B.f_over, False)]), what="blur")


# ---- layers, kinds side by side -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["96x64_bpp4", "37x29_partial_blocks"])
def test_opaque_then_two_translucent_layers(name):
    """FLAT, then two draws with flags 13: the model's frame and stats, and bit for bit the z-buffer of the opaque draw alone."""
    cfg, clip, col = B.frame(name)
    a, b = len(clip) // 3, 2 * len(clip) // 3
    glass = kind(B.OVER_SRC, 0, 13)
    case = frame_case(name, lambda clip, col: [(FLAT, None, clip[:a], None, col[:a]), (glass, None, clip[a:b], None, col[a:b]), (glass, None, clip[b:], None, col[b:])])
    got = render(case)
    m = B.Model(**cfg)
    m.draw(clip[:a], col[:a], B.f_source)
    m.draw(clip[a:b], col[a:b], B.f_over, False)
    m.draw(clip[b:], col[b:], B.f_over, False)
    same(got, m.result(), what=name)
    opaque = render(dict(case, draws=case["draws"][:1]))
    assert (got[1].view(np.uint64) == opaque[1].view(np.uint64)).all()
    assert got[2][1] > opaque[2][1]


@pytest.mark.gpu
def test_kinds_back_to_back():
    """Two blending kinds back to back, a blending kind next to a plain discarding kind and next to FLAT: each meeting cuts the flush."""
    name = "96x64_bpp4"
    cfg, clip, col = B.frame(name)
    q = [len(clip) * i // 5 for i in range(6)]
    kinds = [(kind(B.OVER_SRC, 0, 5), B.f_over, True), (kind(B.ADD_SRC, 0, 13), B.f_add, False), (kind(B.ODD_DISCARD_SRC, 0, 1), B.f_odd_discard, True),
             (kind(B.ALPHA_TEST_SRC, 0, 5), B.f_alpha_test, True), (kind(B.OVER_SRC, 0, 13), B.f_over, False)]
    case = frame_case(name, lambda clip, col: [(k, None, clip[q[i]:q[i + 1]], None, col[q[i]:q[i + 1]]) for i, (k, _, _) in enumerate(kinds)])
    m = B.Model(**cfg)
    for i, (_, fn, depth_write) in enumerate(kinds):
        m.draw(clip[q[i]:q[i + 1]], col[q[i]:q[i + 1]], fn, depth_write)
    want = m.result()
    same(render(case), want, what="one flush call")
    same(render(case, halves=True), want, what="halves")


# ---- strips and bands -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [3, 4])
def test_strips_and_bands_equal_whole_frame(bpp):
    w, h = 200, 192             # (the bands' period divides the height)
    clip, col = B.scene(w, h, 900, 7400 + bpp, rmin=3.0, rmax=50.0)
    case = cases.make_case(w, h, [(FLAT, None, clip[:300], None, col[:300]), (kind(B.OVER_SRC, 0, 5), None, clip[300:600], None, col[300:600]),
                                  (kind(B.ALPHA_TEST_SRC, 0, 13), None, clip[600:], None, col[600:])], bpp=bpp, clear=(20, 30, 40, 255))
    whole = render(case)
    assert whole[2][1] > 0
    for strip, il in [((37, 131), None), (None, (32, 0, 2)), (None, (32, 1, 2))]:
        got = render(case, strip=strip, interleave=il)
        rows = strip if strip else cases.band_rows(h, il)
        same(got, whole, rows=rows, stats=False, what=f"bpp {bpp} strip {strip} bands {il}")
