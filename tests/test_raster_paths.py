"""Code paths of the raster kernels that ordinary scenes do not reach, each against the CPU oracle (and, for the signed-zero
z ranges, the reference's own goldens through cases.CASES):

  A. triangles that are not "well scaled" (k_setup: ruz = 0, TRGL_DL_LITERAL) in every k_raster / k_shade instantiation:
     the literal visit, the literal branch of resolve and of k_shade, at 1, 3 and 4 bytes per pixel;
  B. z ranges that end in a signed zero (first-zero keys, k_fold_stats' lock, trgl_get_stats);
  C. the perspective fallback |denom| < 1e-15 of our_gl.cpp:177-185 (resolve and k_shade);
  D. frames that start from caller-written buffers (no init_from_clear: the block-out stores only pixels with fragments);
  E. the mixed flush at every pixel size, and short tile lists after a large frame on one context.

Bar (cases.assert_same_frame): z bits, framebuffer bytes and the stats tuple equal the oracle's; EYE colours within 1 LSB on at
most 0.1 % of the pixels.  The tests without the gpu mark check that the scenes really reach the paths they are meant for.
"""
import numpy as np
import pytest

import cases
from oracle import orc
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, EYE, CHECKER, make_uniforms

MIXED = "mixed"                       # FLAT + GOURAUD + PHONG + CHECKER draws in one flush: k_raster<ANY>, k_shade<ANY>
KINDS = [FLAT, GOURAUD, PHONG, EYE, CHECKER, MIXED]
KIND_NAMES = {FLAT: "flat", GOURAUD: "gouraud", PHONG: "phong", EYE: "eye", CHECKER: "checker", MIXED: "mixed"}

check, same = cases.check_gpu, cases.assert_same_frame


# ---- scene inputs per kind -----------------------------------------------------------------------------------------
def _kind_case(kind, clip, col, w, h, bpp, seed, viewport=None, clear=(30, 20, 10, 200)):
    """The draws of `kind` for the triangles clip / col (MIXED: four consecutive draws of the four kinds, one flush)."""
    n = clip.shape[0]
    d, nm, sp = scenes.procedural_textures(64)
    tx = {0: d, 1: nm, 2: sp}
    hd = scenes.head_standin(1, w, h)
    u_ph = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.7, 0, 1, 2)
    inten = scenes.SplitMix64(seed).uniform(n * 3, -0.2, 1.3).reshape(n, 3)
    vary = cases.phong_soup_varyings(n, seed + 1)
    u_ck = make_uniforms(cells=5)
    if kind == MIXED:
        e = [n * i // 4 for i in range(5)]
        draws = [(FLAT, None, clip[e[0]:e[1]], None, col[e[0]:e[1]]),
                 (GOURAUD, None, clip[e[1]:e[2]], inten[e[1]:e[2]], col[e[1]:e[2]]),
                 (PHONG, u_ph, clip[e[2]:e[3]], vary[e[2]:e[3]], None),
                 (CHECKER, u_ck, clip[e[3]:e[4]], None, col[e[3]:e[4]])]
    else:
        draws = [(kind, {PHONG: u_ph, EYE: u_ph, CHECKER: u_ck}.get(kind), clip,
                  {GOURAUD: inten, PHONG: vary, EYE: vary}.get(kind), None if kind in (PHONG, EYE) else col)]
    return cases.make_case(w, h, draws, bpp=bpp, viewport=viewport, textures=tx if kind in (PHONG, EYE, MIXED) else {}, clear=clear)


# =====================================================================================================================
# A. triangles that are not well scaled
# =====================================================================================================================
LW, LH = 160, 128


def literal_scene(seed):
    """Dense random scene with perspective w (UNIT_VIEWPORT: screen = NDC), every fifth triangle replaced by one that k_setup
    sends down the literal path, the three reasons in turn:
      0: one vertex at +-1e200..1e250 px - a wedge over the clamped bbox, up to the whole frame;
      1: an edge delta below 2^-250 (a vertex at x or y = 0, the next at a distance 1e-80..1e-300 from that axis);
      2: a sliver 5..60 px long and 1e-12..1e-10 px wide (fails 2^-40 S^2 R < |u.z|), half of them along a row of pixel centres.
    Vertex depths stay those of the generator, so literal and ordinary triangles interleave in depth.
    Returns (clip, colors, literal_rows, class_of_row)."""
    n = 2500
    clip, col = scenes.random_triangles(n, LW, LH, seed=seed, rmin=2, rmax=40, perspective_w=True)
    clip = cases.to_screen_space(clip, LW, LH)
    u = scenes.SplitMix64(seed + 77).uniform(n * 6).reshape(n, 6)
    rows = np.arange(0, n, 5)
    cls = (rows // 5) % 3
    for i, c in zip(rows, cls):
        w = clip[i, [3, 7, 11]].copy()
        p = [[clip[i, 4 * v] / w[v], clip[i, 4 * v + 1] / w[v]] for v in range(3)]
        if c == 0:
            # the far vertex is v1 (finite arithmetic: a wedge), or v0 on every fourth (the products of u.z overflow: inf / NaN)
            # towards -x / -y: a bbox end at +1e200 converts to INT_MIN (our_gl.cpp:130-133 on x86) and culls the triangle
            ang = 3.141592653589793 * (1.02 + 0.46 * u[i, 0])
            far = 10.0 ** (200.0 + 50.0 * u[i, 1])
            k, j = (0, 1) if i % 20 == 0 else (1, 2)
            p[k] = [p[j][0] + far * np.cos(ang), p[j][1] + far * np.sin(ang)]
            q = [np.array(v) for v in p]
            q[k] = q[j] + 1e6 * np.array([np.cos(ang), np.sin(ang)])
            if (q[1][0] - q[0][0]) * (q[2][1] - q[0][1]) - (q[1][1] - q[0][1]) * (q[2][0] - q[0][0]) < 0:
                p[1], p[2] = p[2], p[1]                        # counter-clockwise, so that the back-face test keeps it
        elif c == 1:                                           # (counter-clockwise by construction)
            tiny = 10.0 ** -(80.0 + 220.0 * u[i, 1])
            a = 50.0 + 50.0 * u[i, 2]; L = 8.0 + 40.0 * u[i, 3]; r = 5.0 + 50.0 * u[i, 4]
            if u[i, 0] < 0.5:                                  # x-delta v0 -> v1 tiny, on the frame's left edge
                p = [[0.0, a], [tiny, a - L], [r, a - L / 2]]
            else:                                              # y-delta tiny, on the bottom edge
                p = [[a, 0.0], [a + L, tiny], [a + L / 2, r]]
            w[:] = 1.0 if u[i, 5] < 0.5 else w[0]             # (ndc = clip / w keeps the tiny coordinate tiny and non-zero)
        else:
            L = 5.0 + 55.0 * u[i, 1]
            wd = 10.0 ** (-12.0 + 2.0 * u[i, 2])
            if u[i, 0] < 0.5:                                  # along a row of pixel centres: the long edge passes through them
                x0, y0 = np.floor(p[0][0]) + 0.5, np.floor(p[0][1]) + 0.5
                p = [[x0, y0], [x0 + L, y0], [x0 + L / 2, y0 + wd]]
                w[:] = 1.0
            else:
                ang = 6.283185307179586 * u[i, 3]
                dx, dy = np.cos(ang), np.sin(ang)
                cx, cy = p[0]
                p = [[cx - L * dx, cy - L * dy], [cx + L * dx, cy + L * dy], [cx - wd * dy, cy + wd * dx]]
        if c == 2 and (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]) < 0:
            p[1], p[2] = p[2], p[1]
        for v in range(3):                                     # clip = ndc * w (the depth keeps its NDC value)
            zn = clip[i, 4 * v + 2] / clip[i, 4 * v + 3]
            clip[i, 4 * v], clip[i, 4 * v + 1], clip[i, 4 * v + 2], clip[i, 4 * v + 3] = p[v][0] * w[v], p[v][1] * w[v], zn * w[v], w[v]
    return clip, col, rows, cls


def setup_literal(clip, viewport, W, H, margin=True):
    """numpy restatement of k_setup's culling and "well scaled" predicate (our_gl.cpp:94-135, kernels_bin.hip), with clear margins:
    per triangle, 1 = survives culling and is literal by a margin for one of the three reasons, 0 = anything else."""
    vp = np.asarray(viewport, np.float64).reshape(4, 4)
    w = clip[:, [3, 7, 11]]
    with np.errstate(all="ignore"):
        ndc = [clip[:, 4 * v: 4 * v + 4] / w[:, v:v + 1] for v in range(3)]
        zo = np.stack([(n[:, 2] < -1) | (n[:, 2] > 1) for n in ndc], 1)
        ok = (w > 1e-12).all(1) & ~zo.all(1) & np.all([np.isfinite(n).all(1) for n in ndc], 0)
        sx = np.stack([n @ vp[0] for n in ndc], 1); sy = np.stack([n @ vp[1] for n in ndc], 1)
        e1x, e1y, e2x, e2y = sx[:, 1] - sx[:, 0], sy[:, 1] - sy[:, 0], sx[:, 2] - sx[:, 0], sy[:, 2] - sy[:, 0]
        ok &= ~((e1x * e2y - e1y * e2x) <= 0)                  # (NaN passes, as in the reference)
        cvt = lambda a: np.where((a > -2147483649.0) & (a < 2147483648.0), np.trunc(a), -2147483648.0)    # x86 cvttsd2si
        bx0 = np.maximum(0, cvt(np.floor(sx.min(1)))); bx1 = np.minimum(W - 1, cvt(np.ceil(sx.max(1))))
        by0 = np.maximum(0, cvt(np.floor(sy.min(1)))); by1 = np.minimum(H - 1, cvt(np.ceil(sy.max(1))))
        ok &= (bx0 <= bx1) & (by0 <= by1)
        s0x, s0y, s1x, s1y = e2x, e1x, e2y, e1y
        uz = s0x * s1y - s0y * s1x
        big = (np.abs(sx) >= 2.0 ** 201).any(1) | (np.abs(sy) >= 2.0 ** 201).any(1)
        dl = np.stack([s0x, s0y, s1x, s1y], 1)
        small = ((dl != 0) & (np.abs(dl) < 2.0 ** -251)).any(1)
        S = np.abs(dl).sum(1)
        rx = np.maximum(np.abs(sx[:, 0] - (bx0 + 0.5)), np.abs(sx[:, 0] - (bx1 + 0.5)))
        ry = np.maximum(np.abs(sy[:, 0] - (by0 + 0.5)), np.abs(sy[:, 0] - (by1 + 0.5)))
        sliver = ~big & ~small & (2.0 ** -40 * S * S * (rx + ry + 17 + S) >= 4 * np.abs(uz)) & (np.abs(uz) >= 4e-12)
    return ok & (big | small | sliver), ok & big, ok & small, ok & sliver


@pytest.mark.parametrize("seed", [3100, 3101, 3102])
def test_literal_scenes_reach_the_literal_path(seed):
    """Non-vacuity of A: every literal scene has triangles of all three reasons that survive culling, and they own final pixels
    (the oracle's frame differs in >= 1 % of the pixels without them)."""
    clip, col, rows, cls = literal_scene(seed)
    lit, big, small, sliver = setup_literal(clip, cases.UNIT_VIEWPORT, LW, LH)
    assert big.sum() >= 50 and small.sum() >= 50 and sliver.sum() >= 50, (big.sum(), small.sum(), sliver.sum())
    assert not lit[np.setdiff1d(np.arange(len(clip)), rows)].any()        # the ordinary ones are well scaled
    keep = np.ones(len(clip), bool); keep[rows] = False
    o = orc.Oracle(LW, LH, 3, viewport=cases.UNIT_VIEWPORT); o.draw(orc.FLAT, clip, colors=col)
    o2 = orc.Oracle(LW, LH, 3, viewport=cases.UNIT_VIEWPORT); o2.draw(orc.FLAT, clip[keep], colors=col[keep])
    assert (o.z.view(np.uint64) != o2.z.view(np.uint64)).mean() >= 0.01
    # slivers and tiny-delta triangles own pixels of their own too (not only the wedges)
    keep2 = np.ones(len(clip), bool); keep2[rows[cls != 0]] = False
    o3 = orc.Oracle(LW, LH, 3, viewport=cases.UNIT_VIEWPORT); o3.draw(orc.FLAT, clip[keep2], colors=col[keep2])
    assert (o.z.view(np.uint64) != o3.z.view(np.uint64)).sum() >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [1, 3, 4])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_NAMES.get)
def test_literal_triangles_in_every_kernel_variant(kind, bpp):
    """Literal triangles mixed into a dense scene: one flush, two flushes, two strip contexts cut at an odd row."""
    clip, col, _, _ = literal_scene(3100 + bpp)
    case = _kind_case(kind, clip, col, LW, LH, bpp, seed=3200 + bpp, viewport=cases.UNIT_VIEWPORT)
    assert check(case)[2][1] > 5000
    check(case, split=2)
    for strip in ((0, 45), (45, LH)):
        check(case, strip=strip)
    # observed, not only predicted: k_setup's own count of the triangles it sent down the literal path (every row that
    # setup_literal marks by a margin survives culling with a non-empty bbox and a u.z that is not tiny, so it has pairs)
    with Context(LW, LH, bpp) as ctx:
        ctx.set_viewport(case["viewport"])
        for slot, t in case["textures"].items():
            ctx.upload_texture(slot, t)
        for k, u, c, vary, cl in case["draws"]:
            ctx.draw(k, c, vary, cl, u)
        ctx.flush()
        observed = ctx.debug_snapshot()["info"]["literal_tris"]
    predicted = sum(int(setup_literal(d[2], cases.UNIT_VIEWPORT, LW, LH)[0].sum()) for d in case["draws"])
    assert observed >= predicted >= 150, (observed, predicted)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [FLAT, PHONG], ids=KIND_NAMES.get)
def test_literal_triangles_in_interleaved_bands(kind):
    """trgl_set_interleave over two contexts: every rank's rows equal the oracle's and the fragment counts add up."""
    clip, col, _, _ = literal_scene(3103)
    case = _kind_case(kind, clip, col, LW, LH, 3, seed=3203, viewport=cases.UNIT_VIEWPORT)
    want = cases.run_oracle(case)
    frags = 0
    for rank in range(2):
        il = (32, rank, 2)
        got = cases.run_gpu(case, interleave=il)
        same(got, want, rows=cases.band_rows(LH, il), eye=cases.has_eye(case), stats=False, what=f"rank {rank}")
        st = got[2]
        assert st[0] == want[2][0] and st[2:6] == want[2][2:6]
        frags += st[1]
    assert frags == want[2][1]


# =====================================================================================================================
# B. z ranges that end in a signed zero
# =====================================================================================================================
def _zero_bits(z):
    zb = z.view(np.uint64)
    return int((zb == 0).sum()), int((zb == np.uint64(1 << 63)).sum())


@pytest.mark.parametrize("name", sorted(cases.ZERO_CASES))
def test_zero_cases_end_at_the_intended_signed_zero(name):
    """Non-vacuity of the golden zero cases: the oracle's z-buffer holds both zero bit patterns, and its range ends at the zero
    the case was built for (the goldens pin the same line from the reference itself)."""
    fb, z, st = cases.run_oracle(cases.CASES[name]())
    pos, neg = _zero_bits(z)
    assert pos > 0 and neg > 0, (pos, neg)
    want_min, want_max = cases.ZERO_CASES[name]
    if want_min is not None:
        assert st[6] == 0.0 and st[8] == want_min
    if want_max is not None:
        assert st[7] == 0.0 and st[9] == want_max


def test_zero_sign_in_one_triangle_follows_x_major_order():
    """zero_signs_in_one_triangle_96x64: the zeros in the z-buffer are the pixels of that one triangle; the first of them in the
    reference's x-major order is -0 while the first in y-major order is +0, so the order of the first-zero key matters."""
    fb, z, st = cases.run_oracle(cases.CASES["zero_signs_in_one_triangle_96x64"]())
    zs = np.argwhere(z.T == 0.0)                        # (x, y), x-major
    x, y = zs[0]
    assert np.signbit(z[y, x]) and st[8] == -1.0
    y, x = np.argwhere(z == 0.0)[0]                     # (y, x), y-major
    assert not np.signbit(z[y, x])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cases.ZERO_CASES))
def test_zero_cases_in_strips_and_two_flushes(name):
    """Each strip counts its own first zero; two flushes lock the sign of the first one."""
    case = cases.CASES[name]()
    H = case["height"]
    check(case, split=2)
    for strip in ((0, 19), (19, H)):
        check(case, strip=strip)


def _zero_background(n, W, H, seed, sign=1.0):
    clip, col = scenes.random_triangles(n, W, H, seed=seed, rmin=3, rmax=24)
    return cases.fold_depths(clip, sign), col


@pytest.mark.gpu
def test_zero_sign_lock_over_draws_and_flushes():
    """Zeros spread over two draws of one flush (record order across draws decides) and over later flushes (the lock holds:
    a first zero of the other sign in a later flush changes nothing).  Stats after every flush against the oracle."""
    W, H = 128, 96
    clip, col = _zero_background(1200, W, H, seed=51)
    cases.set_zero_depths(clip, [199], -1.0)                  # last triangle of draw 1
    cases.set_zero_depths(clip, [200, 201], 1.0)              # first triangles of draw 2
    cases.set_zero_depths(clip, range(600, 603), 1.0)         # flush 2
    cases.set_zero_depths(clip, range(900, 903), -1.0)        # flush 3
    parts = [[(0, 200), (200, 400)], [(400, 800)], [(800, 1200)]]
    o = orc.Oracle(W, H, 3)
    with Context(W, H, 3) as ctx:
        for flush in parts:
            for a, b in flush:
                ctx.draw(FLAT, clip[a:b], colors=col[a:b])
                o.draw(orc.FLAT, clip[a:b], colors=col[a:b])
            ctx.flush()
            assert ctx.stats() == o.stats
            assert ctx.stats_line() == orc.format_stats_line(o.stats)
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()), (o.fb, o.z, o.stats))
    assert o.stats[8] == -1.0 and o.stats[6] == 0.0
    # the first zero comes in a later flush than the first fragments
    clip2, col2 = _zero_background(800, W, H, seed=52)
    cases.set_zero_depths(clip2, range(500, 503), 1.0)
    cases.set_zero_depths(clip2, range(700, 703), -1.0)
    o = orc.Oracle(W, H, 3)
    with Context(W, H, 3) as ctx:
        for a, b in ((0, 400), (400, 600), (600, 800)):
            ctx.draw(FLAT, clip2[a:b], colors=col2[a:b]); ctx.flush()
            o.draw(orc.FLAT, clip2[a:b], colors=col2[a:b])
            assert ctx.stats() == o.stats
    assert o.stats[8] == 1.0


@pytest.mark.gpu
def test_reset_stats_clears_the_zero_lock():
    """trgl_reset_stats forgets the sign of the first zero: the next zero written decides again."""
    W, H = 128, 96
    clip, col = _zero_background(600, W, H, seed=53)
    cases.set_zero_depths(clip, range(100, 103), -1.0)
    cases.set_zero_depths(clip, range(400, 403), 1.0)
    cases.set_zero_depths(clip, range(500, 503), -1.0)
    o = orc.Oracle(W, H, 3)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, clip[:300], colors=col[:300])
        o.draw(orc.FLAT, clip[:300], colors=col[:300])
        assert ctx.stats() == o.stats and o.stats[8] == -1.0
        ctx.reset_stats()
        o.L.orc_stats_init(orc.C.byref(o.t.stats))
        ctx.draw(FLAT, clip[300:], colors=col[300:])
        o.draw(orc.FLAT, clip[300:], colors=col[300:])
        assert o.stats[8] == 1.0
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()), (o.fb, o.z, o.stats))


@pytest.mark.gpu
def test_literal_triangles_write_zeros():
    """Wedges (a vertex at 1e220 px) and slivers with vertex depths of both zero signs, on a background folded to >= 0."""
    W, H = LW, LH
    clip, col, rows, cls = literal_scene(3104)
    clip = cases.fold_depths(clip, 1.0)
    wedges = rows[cls == 0]
    cases.set_zero_depths(clip, wedges[10:12], (-1.0, -1.0, 1.0))
    cases.set_zero_depths(clip, wedges[12:14], 1.0)
    cases.set_zero_depths(clip, wedges[14:16], -1.0)
    cases.set_zero_depths(clip, rows[cls == 2][:40], -1.0)
    for kind in (FLAT, PHONG):
        case = _kind_case(kind, clip, col, W, H, 3, seed=3204, viewport=cases.UNIT_VIEWPORT)
        ofb, oz, ost = cases.run_oracle(case)
        assert ost[6] == 0.0 and min(_zero_bits(oz)) > 0
        check(case)
        check(case, split=3)


@pytest.mark.gpu
def test_zero_race_on_a_2048_frame():
    """2048 x 2048, 3000 triangles of 8-120 px with zero depths of random signs among 3000 folded to > 0: zeros are written by
    thousands of workgroups at once, and the atomicMin of the first-zero key has to find the first in the reference's order."""
    W = H = 2048
    n = 6000
    clip, col = scenes.random_triangles(n, W, H, seed=55, rmin=8, rmax=120)
    clip = cases.fold_depths(clip, 1.0)
    sg = scenes.SplitMix64(56).uniform(n)
    zero_rows = np.arange(1, n, 2)
    for i in zero_rows:
        cases.set_zero_depths(clip, [i], -1.0 if sg[i] < 0.5 else 1.0)
    # the first zero triangle in order is +0 and small; the -0 ones after it cover far more pixels
    cases.set_zero_depths(clip, [1], 1.0)
    for i in (1,):
        for v in (1, 2):
            clip[i, 4 * v: 4 * v + 2] = clip[i, 0:2] + (clip[i, 4 * v: 4 * v + 2] - clip[i, 0:2]) * 0.1
    case = cases.make_case(W, H, [(FLAT, None, clip, None, col)])
    want = cases.run_oracle(case)
    pos, neg = _zero_bits(want[1])
    assert pos > 0 and neg > 0 and want[2][6] == 0.0
    same(cases.run_gpu(case), want)


# =====================================================================================================================
# C. the perspective fallback |denom| < 1e-15
# =====================================================================================================================
FW, FH = 160, 112


def fallback_scene(seed):
    """Random triangles; in turn a third of them get
      all three w in 1e16..1e20 (clip = ndc w: ordinary NDC, denom <= 1e-16 at every pixel by construction),
      one w in 1e16..1e20 and two in 3e14..9e14 (denom crosses 1e-15 inside the triangle),
      one w just above the 1e-12 cull (1 / w up to 1e12) next to ordinary ones.
    Returns (clip, colors, rows of the first class, rows of the second)."""
    n = 2400
    clip, col = scenes.random_triangles(n, FW, FH, seed=seed, rmin=3, rmax=48, perspective_w=True)
    u = scenes.SplitMix64(seed + 5).uniform(n * 3).reshape(n, 3)
    for i in range(n):
        k = i % 3
        if k == 0:
            w = 10.0 ** (16.0 + 4.0 * u[i])
        elif k == 1:
            w = np.array([10.0 ** (16.0 + 4.0 * u[i, 0]), 3e14 + 6e14 * u[i, 1], 3e14 + 6e14 * u[i, 2]])
            w = np.roll(w, i % 7 % 3)
        else:
            w = clip[i, [3, 7, 11]].copy()
            w[i % 7 % 3] = 1e-12 * (1.0 + 1e-6 * (1.0 + u[i, 0]))
        for v in range(3):
            cw = clip[i, 4 * v + 3]
            clip[i, 4 * v: 4 * v + 3] = clip[i, 4 * v: 4 * v + 3] / cw * w[v]
            clip[i, 4 * v + 3] = w[v]
    return clip, col, np.arange(0, n, 3), np.arange(1, n, 3)


def test_fallback_scenes_reach_the_fallback():
    """Non-vacuity of C: the triangles with huge w survive culling and own final pixels, and for the second class the
    denominator of our_gl.cpp:172-174 crosses 1e-15 inside the triangle (evaluated at its vertices' barycentrics)."""
    clip, col, all_huge, one_huge = fallback_scene(3300)
    keep = np.ones(len(clip), bool); keep[all_huge] = False; keep[one_huge] = False
    o = orc.Oracle(FW, FH, 3); o.draw(orc.FLAT, clip, colors=col)
    o2 = orc.Oracle(FW, FH, 3); o2.draw(orc.FLAT, clip[keep], colors=col[keep])
    assert (o.z.view(np.uint64) != o2.z.view(np.uint64)).mean() >= 0.2
    iw = 1.0 / clip[one_huge][:, [3, 7, 11]]
    assert ((iw.min(1) < 1e-15) & (iw.max(1) > 1e-15)).all()       # denom = iw at the vertices: below at one, above at another
    assert (1.0 / clip[all_huge][:, [3, 7, 11]] <= 1e-16).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GOURAUD, CHECKER, PHONG, EYE, MIXED], ids=KIND_NAMES.get)
def test_perspective_fallback_against_oracle(kind):
    clip, col, _, _ = fallback_scene(3300)
    for bpp in (3, 4):
        case = _kind_case(kind, clip, col, FW, FH, bpp, seed=3400)
        assert check(case)[2][1] > 5000
    check(case, split=2)


# =====================================================================================================================
# D. frames that start from caller-written buffers
# =====================================================================================================================
_loaded_buffers = cases.loaded_buffers


@pytest.mark.gpu
@pytest.mark.parametrize("W", [97, 98, 99])
@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_draws_on_caller_written_buffers(bpp, W):
    """trgl_write_framebuffer / trgl_write_zbuffer, then draws of every kind, whole frame and one strip: pixels without fragments
    keep the written bytes (also in tiles that have triangles), the rest equals the oracle started from the same buffers."""
    H = 70
    fb0, z0 = _loaded_buffers(W, H, bpp)
    clip, col = scenes.random_triangles(700, W, H, seed=3500 + W, rmin=2, rmax=14, perspective_w=True)
    for kind in KINDS:
        case = _kind_case(kind, clip, col, W, H, bpp, seed=3600 + W)
        for strip in (None, (13, 51)):
            want = cases.run_oracle(case, strip=strip, start=(fb0, z0))
            same(cases.run_gpu(case, strip=strip, start=(fb0, z0)), want, eye=kind == EYE)     # every row: outside the strip too
            kept = (want[0] == fb0).all(-1)
            assert 0.05 < kept.mean() < 0.95, kept.mean()          # both written and untouched pixels in the frame


@pytest.mark.gpu
def test_clear_and_write_order():
    """A pending trgl_clear is applied before a later write_* (the write wins); a clear after a write wins over it."""
    W, H, bpp = 99, 70, 3
    fb0, z0 = _loaded_buffers(W, H, bpp)
    clip, col = scenes.random_triangles(500, W, H, seed=3700, rmin=2, rmax=14)
    with Context(W, H, bpp) as ctx:
        ctx.draw(FLAT, clip[:100], colors=col[:100])
        ctx.clear((9, 8, 7, 6), 0.5)
        ctx.write_framebuffer(fb0)                                # z stays the pending clear's 0.5
        ctx.draw(FLAT, clip[100:], colors=col[100:])
        want = cases.run_oracle(cases.make_case(W, H, [(FLAT, None, clip[100:], None, col[100:])], zclear=0.5), start=(fb0, None))
        same((ctx.read_framebuffer(), ctx.read_zbuffer()), want, stats=False, what="write after clear")
        flat = cases.make_case(W, H, [(FLAT, None, clip, None, col)], clear=(1, 2, 3, 4), zclear=0.25)
        ctx.clear((1, 2, 3, 4), 0.25)
        ctx.write_zbuffer(z0); ctx.write_framebuffer(fb0)         # both written after the clear: they win
        ctx.draw(FLAT, clip, colors=col)
        same((ctx.read_framebuffer(), ctx.read_zbuffer()), cases.run_oracle(flat, start=(fb0, z0)), stats=False, what="writes after clear")
        ctx.write_zbuffer(z0); ctx.write_framebuffer(fb0)
        ctx.clear((1, 2, 3, 4), 0.25)                             # the clear after the writes wins
        ctx.draw(FLAT, clip, colors=col)
        same((ctx.read_framebuffer(), ctx.read_zbuffer()), cases.run_oracle(flat), stats=False, what="clear after writes")


# =====================================================================================================================
# E. short tile lists after a large frame
# =====================================================================================================================
def _tile_lists_scene(W, H, seed):
    """Per 32 x 32 tile t a list of k_t small triangles inside it, k_t in 1..299 and never a multiple of 4."""
    tx, ty = W // 32, H // 32
    rng = scenes.SplitMix64(seed)
    out = []
    for t in range(tx * ty):
        k = 1 + (t * 37) % 299
        k += k % 4 == 0
        u = rng.uniform(k * 4).reshape(k, 4)
        cx = (t % tx) * 32 + 6 + 20 * u[:, 0]; cy = (t // tx) * 32 + 6 + 20 * u[:, 1]
        r = 1.0 + 3.0 * u[:, 2]
        tri = np.zeros((k, 12))
        for v, (dx, dy) in enumerate(((1.0, 0.0), (-0.5, 0.866), (-0.5, -0.866))):
            tri[:, 4 * v] = (cx + r * dx) * (2.0 / W) - 1.0
            tri[:, 4 * v + 1] = (cy + r * dy) * (2.0 / H) - 1.0
            tri[:, 4 * v + 2] = 2.0 * u[:, 3] - 1.0 + 0.01 * v
            tri[:, 4 * v + 3] = 1.0
        out.append(tri)
    clip = np.concatenate(out)
    col = (np.arange(len(clip), dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0xFF000000)
    return clip, col


@pytest.mark.gpu
def test_short_tile_lists_after_a_large_frame():
    """k_raster reads a tile's list in steps of 256 entries, 4 per lane, and masks the entries past its end.  A first frame
    of many (tile, triangle) pairs leaves the pair buffers full of stale words; the next frames on the same context have
    lists of 1..299 entries (never a multiple of 4 or of 256), so every step ends inside those stale words."""
    W = H = 256
    big, bcol = scenes.random_triangles(400, W, H, seed=3800, rmin=80, rmax=300)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, big, colors=bcol)
        ctx.flush()
        assert ctx.last_flush_info()["pairs"] > 10_000
        for seed in (3801, 3802):
            clip, col = _tile_lists_scene(W, H, seed)
            ctx.clear()
            ctx.reset_stats()
            ctx.draw(FLAT, clip, colors=col)
            got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats())
            same(got, cases.run_oracle(cases.make_case(W, H, [(FLAT, None, clip, None, col)])), what=f"seed {seed}")
