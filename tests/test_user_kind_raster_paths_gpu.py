"""Kinds compiled at run time (include/trgl.h, "User shaders") on the rare raster paths that tests/test_raster_paths.py and
tests/test_gpu_parity.py pin for the built-in kinds, with the scenes of those tests:

  1. triangles that are not "well scaled" (TRGL_DL_LITERAL), 2. the perspective fallback |denom| < 1e-15 of our_gl.cpp:177-185,
  3. frames that start from caller-written buffers at widths 97 - 99 and 1, 3 and 4 bytes per pixel, 4. stored depths of NaN and
  +-inf, subnormal planes and ties, 5. adversarial needles and large triangles with a depth bound in the pair word, 6. short tile
  lists behind stale pair-buffer words.

Two kernels serve such kinds, and both are built by hiprtc from text the library embeds: trgl_shade_user (shade_user.h) shades
kinds of the plain contract behind k_raster<ANY>, trgl_raster_user (raster_user.h) rasterizes every kind registered with
TRGL_SHADER_MAY_DISCARD, the blending ones among them, with a written-out copy of barycentric() and the z-test.  The implementations:

  plain       user_shader_sources GOURAUD, PHONG, EYE - drawn alone, and ("mixed") in one flush between built-in FLAT, PHONG and
              CHECKER draws, where k_raster<ANY>, k_shade<ANY> and trgl_shade_user each have to leave the others' pixels alone;
  discarding  discard_shader_sources GOURAUD, PHONG, CHECKER, CHECKER_B (flag word 1);
  blending    blend_model OVER_SRC and ALPHA_TEST_SRC with the flag words 5 and 13 (READS_DEST, and NO_DEPTH_WRITE on top).

The reference is never the built-in kind on the GPU.  Plain and discarding restatements are held to the CPU oracle of the kind
they restate, blending kinds to blend_model.Model, the immediate-mode model built on that oracle.  Bar (cases.assert_same_frame):
z bits, framebuffer bytes, stats tuple and stats line are equal; the EYE source has EYE's allowance (1 LSB on at most 0.1 % of the
pixels).  The colours of GOURAUD, PHONG, EYE and the predicates of CHECKER / CHECKER_B depend on in.bar, so a wrong literal or
fallback branch in the barycentrics handed to trgl_fragment changes bytes (the tests without the gpu mark, at the end, measure
by how much on the oracle alone); the blending kinds pin in.dst, the separate zmin register and the depths left alone.
"""
import numpy as np
import pytest

import blend_model as B
import cases
import discard_shader_sources as D
import test_gpu_parity as GP
import test_raster_paths as RP
import user_shader_sources as S
from oracle import orc
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, EYE, CHECKER

same = cases.assert_same_frame
UNIT = cases.UNIT_VIEWPORT


# ---- the implementations under test ---------------------------------------------------------------------------------------------
class Impl:
    """A user kind that restates the built-in kind `kind` (what the oracle renders), registered as `shader` = (source, K[, flag
    word]); mixed: drawn in one flush between built-in FLAT, PHONG and CHECKER draws."""

    def __init__(self, name, kind, shader, mixed=False):
        self.name, self.kind, self.shader, self.mixed = name, kind, shader, mixed
        self.eye = kind == EYE

    def case(self, clip, col, w, h, bpp, seed, viewport=None, clear=(30, 20, 10, 200)):
        """(case for the oracle, `shaders` for cases.run_gpu) over the triangles clip / col, with RP._kind_case's inputs."""
        if not self.mixed:
            return RP._kind_case(self.kind, clip, col, w, h, bpp, seed, viewport=viewport, clear=clear), [self.shader]
        e = [clip.shape[0] * i // 4 for i in range(5)]
        parts = [RP._kind_case(k, clip[e[i]:e[i + 1]], col[e[i]:e[i + 1]], w, h, bpp, seed + i, viewport=viewport, clear=clear)
                 for i, k in enumerate((FLAT, self.kind, PHONG, CHECKER))]
        return dict(parts[2], draws=[p["draws"][0] for p in parts]), [None, self.shader, None, None]    # (parts[2]: the textures)


_PLAIN = [("gouraud", GOURAUD, (S.GOURAUD, 3)), ("phong", PHONG, (S.PHONG, 24)), ("eye", EYE, (S.EYE, 24))]
PLAIN = [Impl(f"plain_{n}", k, sh) for n, k, sh in _PLAIN] + [Impl(f"mixed_{n}", k, sh, mixed=True) for n, k, sh in _PLAIN]
DISCARDING = [Impl("discarding_gouraud", GOURAUD, (D.GOURAUD, 3, 1)), Impl("discarding_phong", PHONG, (D.PHONG, 24, 1)),
              Impl("discarding_checker", CHECKER, (D.CHECKER, 0, 1)), Impl("discarding_checker_b", CHECKER, (D.CHECKER_B, 0, 1))]
DISCARDING_FLAT = Impl("discarding_flat", FLAT, (D.FLAT, 0, 1))
OPAQUE = PLAIN + DISCARDING
# name -> (source, flag word, restatement for the model, depth writes)
BLENDING = {"over_5": (B.OVER_SRC, 5, B.f_over, True), "over_13": (B.OVER_SRC, 13, B.f_over, False),
            "alpha_test_5": (B.ALPHA_TEST_SRC, 5, B.f_alpha_test, True), "alpha_test_13": (B.ALPHA_TEST_SRC, 13, B.f_alpha_test, False)}
FAMILIES = {"plain": PLAIN, "discarding": DISCARDING}
by_name = lambda impl: impl.name


# ---- references, computed once and shared (never written to) --------------------------------------------------------------------
_refs = {}


def oracle_frame(key, case, strip=None, start=None):
    """cases.run_oracle plus the stats line, once per key + strip: implementations that restate one kind share the frame."""
    key = key + (strip,)
    if key not in _refs:
        fb, z, st = cases.run_oracle(case, strip=strip, start=start)
        _refs[key] = (fb, z, st, orc.format_stats_line(st))
    return _refs[key]


def opaque_key(tag, impl, *more):
    return (tag, impl.kind, impl.mixed) + more


def random_alphas(n, seed):
    """32-bit colours with random alphas (the generators' own colours are opaque: blending them would show nothing)."""
    return (scenes.SplitMix64(seed).u64(n) >> np.uint64(32)).astype(np.uint32)


def blend_case(clip, w, h, bpp, seed, viewport=None, clear=(30, 20, 10, 200)):
    return cases.make_case(w, h, [(FLAT, None, clip, None, random_alphas(clip.shape[0], seed))], bpp=bpp, viewport=viewport, clear=clear)


def model_frame(case, variant, strip=None, start=None):
    """blend_model.Model's result() for a blend_case drawn by BLENDING[variant]; start = (fb or None, z) as for cases.run_gpu."""
    _, _, fn, depth_write = BLENDING[variant]
    (_, _, clip, _, col), = case["draws"]
    fb0, z0 = start or (None, None)
    m = B.Model(case["width"], case["height"], case["bpp"], viewport=case["viewport"], clear=case["clear"], zclear=case["zclear"],
                start=None if fb0 is None else (fb0, z0))
    if fb0 is None and z0 is not None:
        m.o.z[:] = z0
    if strip is not None:
        m.o.set_strip(*strip)
    m.draw(clip, col, fn, depth_write)
    return m.result()


def blend_shaders(variant):
    return [(BLENDING[variant][0], 0, BLENDING[variant][1])]


def literal_count(seen):
    """An `inspect` for cases.run_gpu: k_setup's own count of the triangles the flush sent down the literal path."""
    return lambda ctx: seen.append(ctx.debug_snapshot()["info"]["literal_tris"])


# =====================================================================================================================
# 1. triangles that are not well scaled
# =====================================================================================================================
LW, LH = RP.LW, RP.LH
STRIPS = ((0, 45), (45, LH))


def _literal_predicted(case):
    predicted = sum(int(RP.setup_literal(d[2], UNIT, LW, LH)[0].sum()) for d in case["draws"])
    assert predicted >= 150, predicted
    return predicted


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [1, 3, 4])
@pytest.mark.parametrize("impl", OPAQUE, ids=by_name)
def test_literal_triangles(impl, bpp):
    """RP.literal_scene(3101): one flush, two flushes, two strip contexts cut at an odd row; k_setup's count of literal triangles
    is at least the number RP.setup_literal predicts by a margin."""
    clip, col, _, _ = RP.literal_scene(3101)
    case, shaders = impl.case(clip, col, LW, LH, bpp, seed=3200 + bpp, viewport=UNIT)
    key = opaque_key("literal", impl, bpp)
    want = oracle_frame(key, case)
    assert want[2][1] > 5000
    seen = []
    same(cases.run_gpu(case, shaders=shaders, inspect=literal_count(seen)), want, eye=impl.eye, what="one flush")
    assert seen[0] >= _literal_predicted(case), seen
    same(cases.run_gpu(case, shaders=shaders, split=2), want, eye=impl.eye, what="two flushes")
    for strip in STRIPS:
        same(cases.run_gpu(case, shaders=shaders, strip=strip), oracle_frame(key, case, strip=strip), rows=strip, eye=impl.eye, what=f"strip {strip}")


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [3, 4])
@pytest.mark.parametrize("variant", sorted(BLENDING))
def test_literal_triangles_blending(variant, bpp):
    """The same scene with random alphas through the blending kinds, against the model; flag word 13 leaves the clear depth."""
    clip, _, _, _ = RP.literal_scene(3101)
    case = blend_case(clip, LW, LH, bpp, seed=3250 + bpp, viewport=UNIT)
    want = model_frame(case, variant)
    assert want[2][1] > 5000
    seen = []
    got = cases.run_gpu(case, shaders=blend_shaders(variant), inspect=literal_count(seen))
    same(got, want, what="one flush")
    assert seen[0] >= _literal_predicted(case), seen
    if not BLENDING[variant][3]:
        assert (got[1] == np.inf).all()
    same(cases.run_gpu(case, shaders=blend_shaders(variant), split=2), want, what="two flushes")
    for strip in STRIPS:
        same(cases.run_gpu(case, shaders=blend_shaders(variant), strip=strip), model_frame(case, variant, strip=strip), rows=strip, what=f"strip {strip}")


# =====================================================================================================================
# 2. the perspective fallback |denom| < 1e-15
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("impl", OPAQUE, ids=by_name)
def test_perspective_fallback(impl):
    """RP.fallback_scene(3300): w of 1e16 - 1e20 on all or on one of the vertices, so that trgl_fragment gets the screen-space
    barycentrics on some pixels of a triangle and the corrected ones on others.  CHECKER's predicate reads them."""
    clip, col, _, _ = RP.fallback_scene(3300)
    for bpp in (3, 4):
        case, shaders = impl.case(clip, col, RP.FW, RP.FH, bpp, seed=3400)
        want = oracle_frame(opaque_key("fallback", impl, bpp), case)
        assert want[2][1] > 5000
        same(cases.run_gpu(case, shaders=shaders), want, eye=impl.eye, what=f"bpp {bpp}, one flush")
        same(cases.run_gpu(case, shaders=shaders, split=2), want, eye=impl.eye, what=f"bpp {bpp}, two flushes")


# =====================================================================================================================
# 3. frames that start from caller-written buffers
# =====================================================================================================================
LOADED_H = 70
LOADED_STRIPS = (None, (13, 51))


def _loaded_scene(W):
    return scenes.random_triangles(700, W, LOADED_H, seed=3500 + W, rmin=2, rmax=14, perspective_w=True)


def _assert_some_pixels_kept(want, fb0):
    kept = (want[0] == fb0).all(-1)
    assert 0.05 < kept.mean() < 0.95, kept.mean()              # both written and untouched pixels in the frame


@pytest.mark.gpu
@pytest.mark.parametrize("W", [97, 98, 99])
@pytest.mark.parametrize("bpp", [1, 3, 4])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_draws_on_caller_written_buffers(family, bpp, W):
    """trgl_write_framebuffer / trgl_write_zbuffer, then the user kind, whole frame and one strip: every row equals the oracle
    started from the same buffers (store_pixel at unaligned 3-byte addresses; pixels without fragments keep the written bytes)."""
    start = cases.loaded_buffers(W, LOADED_H, bpp)
    clip, col = _loaded_scene(W)
    for impl in FAMILIES[family]:
        case, shaders = impl.case(clip, col, W, LOADED_H, bpp, seed=3600 + W)
        for strip in LOADED_STRIPS:
            want = oracle_frame(opaque_key("loaded", impl, bpp, W), case, strip=strip, start=start)
            same(cases.run_gpu(case, shaders=shaders, strip=strip, start=start), want, eye=impl.eye, what=f"{impl.name} strip {strip}")
            _assert_some_pixels_kept(want, start[0])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [97, 98, 99])
@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_blending_over_caller_written_buffers(bpp, W):
    """in.dst is the loaded pixel (the kernel reads 1, 3 or 4 bytes at pix * bpp); the model starts from the same buffers."""
    start = cases.loaded_buffers(W, LOADED_H, bpp)
    clip, _ = _loaded_scene(W)
    case = blend_case(clip, W, LOADED_H, bpp, seed=3650 + W)
    for variant in sorted(BLENDING):
        for strip in LOADED_STRIPS:
            want = model_frame(case, variant, strip=strip, start=start)
            got = cases.run_gpu(case, shaders=blend_shaders(variant), strip=strip, start=start)
            same(got, want, what=f"{variant} strip {strip}")
            _assert_some_pixels_kept(want, start[0])
            if not BLENDING[variant][3]:
                assert (got[1].view(np.uint64) == start[1].view(np.uint64)).all(), f"{variant}: the depths changed"


# =====================================================================================================================
# 4. extreme depths
# =====================================================================================================================
_scenes = {}


def _extreme(seed):
    if seed not in _scenes:
        _scenes[seed] = GP.extreme_depths_scene(seed)
    return _scenes[seed]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("impl", DISCARDING, ids=by_name)
def test_extreme_depths(impl, seed):
    """GP.extreme_depths_scene: vertex depths of +-1e0..1e300, subnormal planes, planes one ulp from flat, ties, on stored depths
    with NaN, -inf, +inf, finite and subnormal patches; two flushes.  The kernel's strict z-test decides alone: it has no cull in
    front of it.  (The depths of this scene stop at 1e300, so no interpolated depth overflows and the finite check of
    our_gl.cpp:160 drops nothing here: test_depths_that_overflow, below, is the one that holds the kernel to it.)"""
    W, H, clip, col, z0 = _extreme(seed)
    case, shaders = impl.case(clip, col, W, H, 3, seed=8400 + seed, clear=(1, 2, 3, 255))
    want = oracle_frame(opaque_key("extreme", impl, seed), case, start=(None, z0))
    assert want[2][1] > 10_000
    same(cases.run_gpu(case, shaders=shaders, start=(None, z0), split=2), want)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("variant", sorted(BLENDING))
def test_extreme_depths_blending(variant, seed):
    """The first 4000 triangles of the scene through the blending kinds.  With flag word 13 every fragment is tested against the
    stored depths themselves, the z range comes from the kernel's own zmin / zmax registers, and the z-buffer stays as written."""
    W, H, clip, _, z0 = _extreme(seed)
    case = blend_case(clip[:4000], W, H, 4 - seed, seed=8450 + seed, clear=(1, 2, 3, 255))
    want = model_frame(case, variant, start=(None, z0))
    assert want[2][1] > 10_000
    got = cases.run_gpu(case, shaders=blend_shaders(variant), start=(None, z0), split=2)
    same(got, want)
    if not BLENDING[variant][3]:
        assert (got[1].view(np.uint64) == z0.view(np.uint64)).all(), "the depths changed"


OW, OH = 128, 96
DBL_MAX = float(np.finfo(np.float64).max)


def overflowing_depths_scene(seed, depth=DBL_MAX):
    """300 ordinary triangles for UNIT_VIEWPORT (w = 1) whose interpolated depth overflows on some pixels: vertex 0 has a depth in
    [-1, 1] (so our_gl.cpp:103-106 keeps the triangle), vertices 1 and 2 the depth +depth (even rows) or -depth (odd rows), and the
    edge between them runs through pixel centres (half-integer end points, a step of (+-1, 0), (0, +-1) or (+-1, +-1) per pixel).
    On such a pixel b0 is 0 and the computed b1 + b2 can be 1 + 2^-52; with depth = DBL_MAX the sum b1 z1 + b2 z2 (:156-158) then
    rounds to +-inf, which :160 drops - and -inf would pass the strict z-test of :165 against anything.  Returns (clip, colours)."""
    n = 300
    u = scenes.SplitMix64(seed).uniform(n * 8).reshape(n, 8)
    steps = [(1, 0), (0, 1), (1, 1), (1, -1), (-1, 0), (0, -1), (-1, -1), (-1, 1)]
    clip = np.zeros((n, 12))
    for i in range(n):
        dx, dy = steps[int(u[i, 0] * 8) % 8]
        k = 6 + int(u[i, 1] * 30)
        bx, by = int(10 + u[i, 2] * (OW - 20)) + 0.5, int(10 + u[i, 3] * (OH - 20)) + 0.5
        b, c = (bx, by), (bx + k * dx, by + k * dy)
        off = (5.0 + 30.0 * u[i, 4]) * (1.0 if u[i, 5] < 0.5 else -1.0)
        nx, ny = -dy / np.hypot(dx, dy), dx / np.hypot(dx, dy)
        a = ((b[0] + c[0]) / 2 + off * nx + 7.0 * (u[i, 6] - 0.5), (b[1] + c[1]) / 2 + off * ny + 7.0 * (u[i, 6] - 0.5))
        if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0:
            b, c = c, b                                        # counter-clockwise, so that the back-face test keeps it
        z = depth if i % 2 == 0 else -depth
        clip[i] = cases.screen_triangle(a, b, c, z=(2.0 * u[i, 7] - 1.0, z, z))
    col = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0xFF000000)
    return clip, col


@pytest.mark.gpu
@pytest.mark.parametrize("impl", DISCARDING, ids=by_name)
def test_depths_that_overflow(impl):
    """our_gl.cpp:160: a fragment whose depth is not finite is dropped.  A depth of -inf would pass the strict z-test, so only the
    kernel's own finite check keeps it out of the z-buffer, the frame, the fragment count and the z range
    (test_overflowing_depths_are_dropped_by_the_finite_check: the scene has such fragments)."""
    clip, col = overflowing_depths_scene(8700)
    case, shaders = impl.case(clip, col, OW, OH, 3, seed=8710, viewport=UNIT)
    want = oracle_frame(opaque_key("overflow", impl), case)
    assert want[2][1] > 5000 and np.isfinite(want[2][6])
    same(cases.run_gpu(case, shaders=shaders), want, what="one flush")
    same(cases.run_gpu(case, shaders=shaders, split=2), want, what="two flushes")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(BLENDING))
def test_depths_that_overflow_blending(variant):
    """The same scene through the blending kinds: with flag word 13 a fragment of depth -inf would be drawn at every stored depth."""
    clip, _ = overflowing_depths_scene(8700)
    case = blend_case(clip, OW, OH, 4, seed=8720, viewport=UNIT)
    want = model_frame(case, variant)
    assert want[2][1] > 5000 and np.isfinite(want[2][6])
    got = cases.run_gpu(case, shaders=blend_shaders(variant))
    same(got, want, what="one flush")
    if not BLENDING[variant][3]:
        assert (got[1] == np.inf).all()
    same(cases.run_gpu(case, shaders=blend_shaders(variant), split=2), want, what="two flushes")


# =====================================================================================================================
# 5. adversarial shapes and large triangles
# =====================================================================================================================
CULL_FREE = [DISCARDING[0], DISCARDING[2]]                 # GOURAUD and CHECKER


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("impl", CULL_FREE, ids=by_name)
def test_adversarial_shapes(impl, seed):
    """GP.adversarial_shapes_scene: needles, tiny triangles, steep depth planes, a vertex far off screen.  trgl_raster_user has no
    cull of its own: it reads the block masks as k_setup and the sort wrote them, and a bit missing there is a missing fragment."""
    W, H, clip, col = GP.adversarial_shapes_scene(seed)
    case, shaders = impl.case(clip, col, W, H, 3, seed=7200 + seed)
    want = oracle_frame(opaque_key("adversarial", impl, seed), case)
    assert want[2][1] > 10_000
    same(cases.run_gpu(case, shaders=shaders), want)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", CULL_FREE, ids=by_name)
def test_large_triangles_with_a_depth_bound_in_the_pair(impl):
    """GP.large_triangles_scene(0): the flush holds triangles of 64 pixels and more, so the pair's triangle word carries a depth bound
    above the index (TRGL_VAL_ZQ) - the kernel must take the index alone.  One flush, then two flushes on the same context."""
    W, H, clip, col = GP.large_triangles_scene(0)
    case, (shader,) = impl.case(clip, col, W, H, 3, seed=8500)
    (_, u, clip, vary, col), = case["draws"]
    want = oracle_frame(opaque_key("large", impl), case)
    assert want[2][1] > 10_000
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]
    with Context(W, H, 3) as ctx:
        kind = cases.register_user_kind(ctx, shader)
        ctx.clear(case["clear"], case["zclear"])
        ctx.draw(kind, clip, vary, col, u)
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()), want, what="one flush")
        ctx.clear(case["clear"], case["zclear"])
        ctx.reset_stats()
        ctx.draw(kind, clip[:5000], cut(vary, 0, 5000), col[:5000], u)
        ctx.flush()
        ctx.draw(kind, clip[5000:], cut(vary, 5000, None), col[5000:], u)
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()), want, what="two flushes")


# =====================================================================================================================
# 6. short tile lists after a large frame
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("impl", [DISCARDING_FLAT, DISCARDING[0]], ids=by_name)
def test_short_tile_lists_after_a_large_frame(impl):
    """trgl_raster_user reads a tile's list in steps of 64 entries, one per lane, and masks the entries past its end.  A first
    frame of many (tile, triangle) pairs leaves the pair buffers full of stale words; the next frames on the same context have
    lists of 1..299 entries, so the last step of every list ends inside those stale words."""
    W = H = 256
    big, bcol = scenes.random_triangles(400, W, H, seed=3800, rmin=80, rmax=300)
    with Context(W, H, 3) as ctx:
        kind = cases.register_user_kind(ctx, impl.shader)
        ctx.draw(FLAT, big, colors=bcol)
        ctx.flush()
        assert ctx.last_flush_info()["pairs"] > 10_000
        for seed in (3801, 3802):
            clip, col = RP._tile_lists_scene(W, H, seed)
            case, _ = impl.case(clip, col, W, H, 3, seed=seed + 10)
            (_, u, clip, vary, col), = case["draws"]
            ctx.clear(case["clear"], case["zclear"])
            ctx.reset_stats()
            ctx.draw(kind, clip, vary, col, u)
            got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
            same(got, oracle_frame(opaque_key("short lists", impl, seed), case), what=f"seed {seed}")


# =====================================================================================================================
# Non-vacuity, on the CPU: bit-equality on a rare path only means something if in.bar matters where the path is taken
# =====================================================================================================================
def _share_changed_by_rolled_intensities(clip, col, rows, w, h, seed, viewport=None):
    """Share of the pixels whose bytes change when GOURAUD's three intensities of the triangles `rows` move on by one vertex: the
    oracle alone, the frame of the scene as it is against the frame with bar's components read in another order on those rows."""
    case = RP._kind_case(GOURAUD, clip, col, w, h, 3, seed, viewport=viewport)
    (kind, u, clip, inten, col), = case["draws"]
    rolled = inten.copy()
    rolled[rows] = np.roll(inten[rows], 1, axis=1)
    a = cases.run_oracle(case)
    b = cases.run_oracle(dict(case, draws=[(kind, u, clip, rolled, col)]))
    assert (a[1].view(np.uint64) == b[1].view(np.uint64)).all() and a[2] == b[2]       # (the intensities colour, nothing else)
    return float((a[0] != b[0]).any(-1).mean())


def test_barycentrics_matter_on_the_literal_triangles():
    """RP.literal_scene(3101), GOURAUD on the oracle: rolling the intensities of the literal rows by one vertex changes 32 % of the
    frame's pixels (measured: 0.3243), so barycentrics from a wrong branch on those rows cannot hide.  Required: at least 0.5 %."""
    clip, col, rows, _ = RP.literal_scene(3101)
    share = _share_changed_by_rolled_intensities(clip, col, rows, LW, LH, 3204, viewport=UNIT)
    print(f"literal rows: share of pixels changed {share:.4f}")
    assert share >= 0.005, share


@pytest.mark.parametrize("which", ["all_huge_w", "one_huge_w"])
def test_barycentrics_matter_on_the_fallback_triangles(which):
    """RP.fallback_scene(3300), GOURAUD on the oracle: rolling the intensities of the rows whose three w are huge (the fallback on
    every pixel) changes 17 % of the pixels (measured: 0.1664), of the rows with one huge w (the denominator crosses 1e-15 inside the
    triangle) 34 % (measured: 0.3393).  Required: at least 0.5 % each."""
    clip, col, all_huge, one_huge = RP.fallback_scene(3300)
    share = _share_changed_by_rolled_intensities(clip, col, all_huge if which == "all_huge_w" else one_huge, RP.FW, RP.FH, 3400)
    print(f"{which}: share of pixels changed {share:.4f}")
    assert share >= 0.005, share



def _fragments_one_at_a_time(clip, col):
    """Fragments the oracle draws when every triangle meets a cleared z-buffer: its covered pixels with a finite depth, nothing else
    (any finite depth passes against the clear's +inf)."""
    o = orc.Oracle(OW, OH, 3, viewport=UNIT)
    for i in range(clip.shape[0]):
        o.clear()
        o.draw(orc.FLAT, clip[i:i + 1], colors=col[i:i + 1])
    return o.stats[1]


def test_overflowing_depths_are_dropped_by_the_finite_check():
    """Non-vacuity of test_depths_that_overflow, on the oracle alone.  The triangles of overflowing_depths_scene(8700) with -DBL_MAX
    on two vertices, each drawn on a cleared z-buffer, give FEWER fragments than the same triangles with -1.7e308 there (5 % of
    headroom: no sum overflows, the coverage is the same): the difference is what our_gl.cpp:160 drops at depth -inf, and what a
    kernel without the finite check would draw.  Measured: 236 fragments of depth -inf and 235 of +inf among the 72 564
    the triangles cover.  Required: at least 50 of depth -inf (a bound set before measuring: about 150 such triangles with some 20
    on-edge pixels each, of which a few per cent overflow)."""
    clip, col = overflowing_depths_scene(8700)
    headroom, _ = overflowing_depths_scene(8700, depth=1.7e308)
    neg, pos = np.arange(1, len(clip), 2), np.arange(0, len(clip), 2)
    covered = _fragments_one_at_a_time(headroom, col)
    dropped_neg = _fragments_one_at_a_time(headroom[neg], col[neg]) - _fragments_one_at_a_time(clip[neg], col[neg])
    dropped_pos = _fragments_one_at_a_time(headroom[pos], col[pos]) - _fragments_one_at_a_time(clip[pos], col[pos])
    print(f"covered {covered}, dropped at -inf {dropped_neg}, at +inf {dropped_pos}")
    assert dropped_neg >= 50, (dropped_neg, dropped_pos)
    # and they lie where the frame can show them: the scene's own frame has no -inf, the frame without :160 would
    want = cases.run_oracle(cases.make_case(OW, OH, [(FLAT, None, clip, None, col)], viewport=UNIT))
    assert want[2][1] > 5000 and not np.isinf(want[1][want[1] != np.inf]).any()
