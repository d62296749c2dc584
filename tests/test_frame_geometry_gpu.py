"""Tiny, thin and limit-size frames (tests/frame_geometry.py) through every frame kernel, against the CPU oracle.

trgl_create accepts any width and height from 1 to 65535; the kernels work in 32 x 32 tiles and 8 x 8 blocks and choose their stores
by W & 1 and W & 3.  What these tests reach, by the code that branches on the frame's geometry:

  shade_common.h clear_rows     full_x with even W (16-byte z stores) and with odd W; full_x with (W & 3) == 0 at bpp 3 and 4 (colour rows
                                as dwords) and with W & 3 = 1, 2, 3 (per-pixel loops); odd W at bpp 1 and 4; W < 32, where no tile is
                                full_x: the clear-only frames and the sparse scenes of test_flushes_on_a_cleared_frame, every frame
  kernels_raster.hip block-out  whole = init_from_clear && X0 + 7 < W: the RGB row assembly through LDS, its dword stores unaligned
                                where 3 W y is no multiple of 4 (9x9, 33x31, 35x29, 65535x2); blocks cut by the right edge (per-pixel
                                branch); W < 8: every block is cut; not init_from_clear: test_draws_on_loaded_buffers
  k_raster owned, ya..yb        rows beyond H, rows outside a strip: test_strip_contexts, test_interleaved_bands
  k_make_items row mask         tiles of which 1 to 7 rows exist (1x1, 2x3, 7x5, 70x1, 40x5, 65535x2, 33 = 32 + 1 rows of 31x33)
  raster_user.h, shade_user.h   their own copies of all of that: test_user_kinds
  k_shade `mine`                PHONG, EYE and MIXED on every frame
  trgl_api.cpp radix passes     1 and 2 tiles: a sort key of 1 bit; 2048 tiles in one row or column: test_setup_and_binning_outputs
  TriRec / BlockState packing   bx | by << 16 with a coordinate of 65534 in either half: the limit frames, whose last pixel is compared
  kernels_post.hip              k_zrange with n < 2, k_zimage / k_composite with n < 4, k_ssao on images narrower or lower than its
                                32-pixel tile (no interior block, every x sample of a 1-pixel-wide image out of range):
                                test_postprocess_*, test_ssao_*; blur, modulate and snapshot passes on the same frames

That the scenes draw, leave cleared pixels, reach the last column and row, tile 2047 and coordinate 65534 is shown without a GPU by
test_frame_geometry.py; the tile counts are read back from debug_snapshot() here.

Bar: z bits, framebuffer bytes, the stats tuple and the stats line equal the oracle's.  EYE: cases.assert_same_frame(eye=True)
allows 1 LSB on at most 0.1 % of the pixels of a row range, which below 1000 pixels is no pixel at all - whether the device's pow
agrees with the oracle's is not for a tiny frame to decide.  So for an EYE row range of fewer than 1000 pixels, z bits and stats are
exact against the oracle and the colours are exact against [0:H, 0:W] of the GPU's own render of the same draws in a frame of
max(W, 128) x max(H, 128) (the crop identity, held on the oracle by test_frame_geometry.py); that large render is held to the oracle
with eye=True unchanged.  Ranges of 1000 pixels and more use eye=True directly.
"""
import functools

import numpy as np
import pytest

import binning_model as bm
import cases
import discard_shader_sources as D
import frame_geometry as fg
import image_ops_model
import shadow_model
from frame_geometry import BELOW_ONE_BLOCK, BPPS, FRAMES, KINDS, KIND_NAMES, LIMIT_FRAMES, MIXED, SCENES, THIN_FRAMES, frame_id
from oracle import orc
from test_direct_pairs_gpu import BLOCK, CHUNK, both_ways, group_sums, per_block
from test_next_rows import _numpy_ssao
from test_stage_outputs_gpu import flush_and_check
from test_user_shaders_gpu import SOURCES
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import EYE, FLAT, GOURAUD, PHONG, Context, SsaoParams

pytestmark = pytest.mark.gpu

same = cases.assert_same_frame
E_UNSUPPORTED = -5
FIVE_FRAMES = [(1, 1), (7, 5), (35, 29), (1, 70), (70, 1)]
HAS_TWO_ROWS = [f for f in FRAMES if f[1] >= 2]


def combos():
    return [(which, kind, bpp) for which in SCENES for kind in KINDS for bpp in BPPS]


@functools.lru_cache(maxsize=None)
def large_frame_colours(W, H, which, bpp, loaded):
    """The framebuffer of the GPU's render of the EYE case in the large frame of the crop identity, itself held to the oracle
    within the EYE tolerance (the large frame has at least 16384 pixels, so the 0.1 % binds)."""
    big = fg.big_frame(fg.case(W, H, which, EYE, bpp))
    start = cases.loaded_buffers(big["width"], big["height"], bpp) if loaded else None
    got = cases.run_gpu(big, start=start)
    same(got, cases.run_oracle(big, start=start), eye=True, what=f"{W}x{H} {which} bpp {bpp}: EYE in the large frame")
    return got[0]


def held(got, key, rows=None, strip=None, loaded=False, stats=True, what=""):
    """got (run_gpu) against the oracle's frame of key = (W, H, which, kind, bpp) drawn with the same strip / loaded buffers, in
    `rows` (None: every row): z bits, framebuffer bytes, stats tuple and stats line.  EYE as the module's docstring says."""
    W, H, which, kind, bpp = key
    want = fg.oracle(W, H, which, kind, bpp, strip=strip, loaded=loaded)
    what = f"{W}x{H} {which} {KIND_NAMES[kind]} bpp {bpp} {what}"
    if rows is not None and len(rows) == 0:            # a rank that owns no row: nothing of the frame is its own
        assert not stats
        return
    if kind != EYE:
        same(got, want, rows=rows, stats=stats, what=what)
        return
    ranges = [(0, H)] if rows is None else [rows] if np.isscalar(rows[0]) else rows
    for y0, y1 in ranges:
        if (y1 - y0) * W >= 1000:
            same(got, want, rows=(y0, y1), eye=True, stats=False, what=what)
        else:
            crop = large_frame_colours(W, H, which, bpp, loaded)[:H, :W]
            same((got[0], got[1]), (crop, want[1]), rows=(y0, y1), stats=False, what=what + " (colours: crop of the device's large frame)")
    if stats:
        assert got[2] == want[2], f"{what}: stats {got[2]} != {want[2]}"
        assert got[3] == want[3], f"{what}: stats line {got[3]!r} != {want[3]!r}"


# ---- 3. the flush ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_flushes_on_a_cleared_frame(frame):
    """One flush on a frame cleared to a non-default colour and depth (init_from_clear: clear_rows for the tiles without triangles,
    block-out's `whole` rows and its per-pixel branch for blocks the right edge cuts), then the same draws in two flushes each (the
    second stores only pixels with fragments), every kind at every pixel size; and a frame that is only cleared, where every work
    item is TRGL_ITEM_CLEAR."""
    W, H = frame
    for which, kind, bpp in combos():
        c = fg.case(W, H, which, kind, bpp)
        held(cases.run_gpu(c), (W, H, which, kind, bpp), what="one flush")
        held(cases.run_gpu(c, split=2), (W, H, which, kind, bpp), what="two flushes")
    for bpp in BPPS:
        empty = cases.make_case(W, H, [], bpp=bpp, clear=fg.CLEAR, zclear=fg.ZCLEAR)
        got = cases.run_gpu(empty)
        want = cases.run_oracle(empty)
        same(got, want + (orc.format_stats_line(want[2]),), what=f"{W}x{H} bpp {bpp} clear only")
        assert (got[0] == np.array(fg.CLEAR[:bpp], np.uint8)).all() and (got[1] == fg.ZCLEAR).all()


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_draws_on_loaded_buffers(frame):
    """A frame that starts from write_framebuffer / write_zbuffer (not init_from_clear: the block-out stores only pixels with
    fragments, through its per-pixel branches at every bpp), every row compared: pixels without fragments keep the written bytes."""
    W, H = frame
    for which, kind, bpp in combos():
        got = cases.run_gpu(fg.case(W, H, which, kind, bpp), start=cases.loaded_buffers(W, H, bpp))
        held(got, (W, H, which, kind, bpp), loaded=True, what="loaded buffers")


@pytest.mark.parametrize("frame", HAS_TWO_ROWS, ids=frame_id)
def test_strip_contexts(frame):
    """Two strip contexts cut at an odd row (H // 2 | 1), and where H >= 3 a middle strip (1, H - 1): `owned` and the clear items'
    row range ya..yb with strip ends inside a block, k_make_items' masks for the rows of a tile that a strip owns."""
    W, H = frame
    cut = fg.odd_cut(H)
    strips = [(0, cut), (cut, H)] + ([(1, H - 1)] if H >= 3 else [])
    for which, kind, bpp in combos():
        for strip in strips:
            got = cases.run_gpu(fg.case(W, H, which, kind, bpp), strip=strip)
            held(got, (W, H, which, kind, bpp), rows=strip, strip=strip, what=f"strip {strip}")


def band_rows(H, il):
    return [(32 * int(ty), min(32 * int(ty) + 32, H)) for ty in np.flatnonzero(bm.owned_tile_rows(H, interleave=il))]


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_interleaved_bands(frame):
    """set_interleave(32, rank, 2) for both ranks: each rank's rows equal the oracle's, the triangle count and the bbox are the whole
    frame's and the fragment counts add up.  Where H <= 32 rank 1 owns no row: it counts no fragment, and the context can be given
    the whole frame afterwards and draw it."""
    W, H = frame
    for which, kind, bpp in combos():
        c = fg.case(W, H, which, kind, bpp)
        want = fg.oracle(W, H, which, kind, bpp)
        frags = 0
        for rank in range(2):
            il = (32, rank, 2)
            got = cases.run_gpu(c, interleave=il)
            held(got, (W, H, which, kind, bpp), rows=band_rows(H, il), stats=False, what=f"rank {rank} of 2")
            st = got[2]
            assert st[0] == want[2][0] and st[2:6] == want[2][2:6], (st, want[2])
            assert H > 32 or rank == 0 or st[1] == 0, st
            frags += st[1]
        assert frags == want[2][1], (frame, which, kind, bpp, frags, want[2][1])
    if H <= 32:
        for bpp in BPPS:
            c = fg.case(W, H, "dense", FLAT, bpp)
            (kind, u, clip, vary, col), = c["draws"]
            with Context(W, H, bpp) as ctx:
                ctx.clear(c["clear"], c["zclear"])
                ctx.set_interleave(32, 1, 2)
                ctx.draw(kind, clip, vary, col, u)
                ctx.flush()
                assert ctx.stats()[1] == 0 and ctx.debug_snapshot()["info"]["P"] == 0
                ctx.set_strip(0, H)
                ctx.reset_stats()
                ctx.clear(c["clear"], c["zclear"])
                ctx.draw(kind, clip, vary, col, u)
                got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
            held(got, (W, H, "dense", FLAT, bpp), what="the whole frame after a rank without rows")


# ---- user kinds -------------------------------------------------------------------------------------------------------------------
USER_FRAMES = [(1, 1), (7, 5), (9, 9), (35, 29), (1, 70), (65535, 2)]
DISCARDING = {FLAT: (D.FLAT, 0, True), GOURAUD: (D.GOURAUD, 3, True), PHONG: (D.PHONG, 24, True)}


@pytest.fixture(scope="module")
def user_kinds():
    """Compile the user sources once: registrations on the contexts of this module then only load the cached code objects."""
    for src, k, *flag in list(DISCARDING.values()) + [SOURCES["gouraud"]]:
        ok, log = api.shader_compile(src, k, bool(flag))
        assert ok, log
    return DISCARDING


@pytest.mark.parametrize("frame", USER_FRAMES, ids=frame_id)
def test_user_kinds(user_kinds, frame):
    """The never-discarding restatements of FLAT, GOURAUD and PHONG registered with TRGL_SHADER_MAY_DISCARD (raster_user.h: its own
    `owned`, clear rows and block-out) and a plain user GOURAUD among built-in kinds in a mixed flush (shade_user.h: its own
    `mine`), in every mode of the tests above, against the oracle's frame of the built-in kind."""
    W, H = frame
    cut = fg.odd_cut(H)
    strips = ([(0, cut), (cut, H)] if H >= 2 else []) + ([(1, H - 1)] if H >= 3 else [])
    for which in SCENES:
        for bpp in BPPS:
            for kind in (FLAT, GOURAUD, PHONG, MIXED):
                c = fg.case(W, H, which, kind, bpp)
                sh = [None, SOURCES["gouraud"], None, None] if kind == MIXED else [user_kinds[kind]]
                assert len(sh) == len(c["draws"]) and (kind != MIXED or c["draws"][1][0] == GOURAUD)
                key = (W, H, which, kind, bpp)
                held(cases.run_gpu(c, shaders=sh), key, what="user kind, one flush")
                held(cases.run_gpu(c, shaders=sh, split=2), key, what="user kind, two flushes")
                held(cases.run_gpu(c, shaders=sh, start=cases.loaded_buffers(W, H, bpp)), key, loaded=True, what="user kind, loaded buffers")
                for strip in strips:
                    held(cases.run_gpu(c, shaders=sh, strip=strip), key, rows=strip, strip=strip, what=f"user kind, strip {strip}")
                frags = 0
                for rank in range(2):
                    il = (32, rank, 2)
                    got = cases.run_gpu(c, shaders=sh, interleave=il)
                    held(got, key, rows=band_rows(H, il), stats=False, what=f"user kind, rank {rank} of 2")
                    assert H > 32 or rank == 0 or got[2][1] == 0
                    frags += got[2][1]
                assert frags == fg.oracle(*key)[2][1]


# ---- 4. setup and binning outputs on few and on very many thin tiles -------------------------------------------------------------
BINNING_FRAMES = [(7, 5), (33, 31), (31, 33), (65535, 2), (2, 65535)]


@pytest.mark.parametrize("which", SCENES)
@pytest.mark.parametrize("frame", BINNING_FRAMES, ids=frame_id)
def test_setup_and_binning_outputs(frame, which):
    """Records, pair lists, tile bounds and the frame of one flush against binning_model, as the flush chooses its path and with the
    direct path and k_expand's chain forced: 1 tile and 2 tiles (a sort key of 1 bit: one radix pass over 2-bin histograms), and
    2048 tiles in one row or column (tile 2047, packed coordinates up to 65534).  The tile counts are the device's own (INFO)."""
    W, H = frame
    c = fg.case(W, H, which, FLAT, 3)
    s, m = flush_and_check(c, what=f"{frame_id(frame)} {which}")
    T = {(7, 5): 1, (33, 31): 2, (31, 33): 2}.get(frame, 2048)
    assert s["info"]["tiles_x"] * s["info"]["tiles_y"] == m.tiles_x * m.tiles_y == T
    assert s["info"]["P"] == int(m.cnt.sum()) > 0
    last = T - 1
    assert any(t == last for t, _, _ in bm.pairs(m))
    assert s["tile_end"][last] > s["tile_start"][last], "the last tile's list is empty on the device"
    if frame in LIMIT_FRAMES:
        far = s["recs"][:m.N][s["cnt"] > 0]["bx1" if W > H else "by1"]
        assert (far == 65534).any() and (s["tile_end"] <= s["tile_start"]).any()
    pb = [int(v) for v in np.add.reduceat(m.cnt, np.arange(0, m.N, BLOCK))]
    S, G = 4096, 2
    fits = max(pb) <= S and max(group_sums(pb, G)) <= CHUNK
    d = both_ways(c, S, G, not fits, what=f"{frame_id(frame)} {which}", counts=pb)
    assert list(per_block(d)) == pb and d["info"]["tiles_x"] * d["info"]["tiles_y"] == T
    assert d["tile_end"][last] > d["tile_start"][last]


# ---- 5. passes over a resident frame of these sizes -----------------------------------------------------------------------------
def draw_dense_flat(ctx, W, H, bpp):
    c = fg.case(W, H, "dense", FLAT, bpp)
    ctx.clear(c["clear"], c["zclear"])
    for kind, u, clip, vary, col in c["draws"]:
        ctx.draw(kind, clip, vary, col, u)
    return c


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_postprocess_after_a_draw(frame):
    """postprocess() after the dense FLAT scene: the z-buffer image (k_zrange over W H / 2 pairs and an odd tail - no pair at all on
    1x1 - and k_zimage's groups of 4 pixels and tail), SSAO (no interior block on frames narrower or lower than 32) and the composite
    equal the oracle's; at 1 byte per pixel the composite is refused and the other two are still right."""
    W, H = frame
    for bpp in BPPS:
        with Context(W, H, bpp) as ctx:
            draw_dense_flat(ctx, W, H, bpp)
            fb, z = ctx.read_framebuffer(), ctx.read_zbuffer()
            same((fb, z), fg.oracle(W, H, "dense", FLAT, bpp), stats=False, what=f"{W}x{H} bpp {bpp}")
            if bpp == 1:
                out = np.empty((H, W, 3), np.uint8)
                assert ctx.L.trgl_postprocess(ctx.h, None, None, None, out.ctypes.data) == E_UNSUPPORTED
            out = ctx.postprocess(final=bpp != 1)
        ao = orc.ssao(z)
        assert np.array_equal(out["zbuffer_image"], orc.zbuffer_image(z)), (frame, bpp)
        assert np.array_equal(out["ao"], ao), (frame, bpp)
        if bpp != 1:
            assert np.array_equal(out["final"], orc.composite(np.ascontiguousarray(fb[..., :3]), ao)), (frame, bpp)


def hand_made_depths(W, H):
    """name -> [H, W] depths: no finite depth (the range keys stay empty: 1e9 / -1e9), exactly one finite depth (max - min < 1e-7:
    the range is widened), and - with two pixels or more - two depths 1e-9 apart among non-finite ones."""
    n = W * H
    out = {"no finite depth": np.resize(np.array([np.inf, np.nan, -np.inf, np.inf, np.inf]), n)}
    one = np.full(n, np.inf); one[n // 2] = 0.375
    out["one finite depth"] = one
    if n >= 2:
        two = np.resize(np.array([0.25, 0.25 + 1e-9, np.inf]), n).copy(); two[0], two[n - 1] = 0.25, 0.25 + 1e-9
        out["two depths 1e-9 apart"] = two
    return {k: np.ascontiguousarray(v.reshape(H, W)) for k, v in out.items()}


@pytest.mark.parametrize("frame", BELOW_ONE_BLOCK + THIN_FRAMES, ids=frame_id)
def test_postprocess_of_hand_made_depths(frame):
    W, H = frame
    with Context(W, H, 3) as ctx:
        for name, z in hand_made_depths(W, H).items():
            ctx.write_zbuffer(z)
            out = ctx.postprocess(final=False)
            assert np.array_equal(out["zbuffer_image"], orc.zbuffer_image(z)), (frame, name)
            assert np.array_equal(out["ao"], orc.ssao(z)), (frame, name)


SSAO_PARAMS = [(8, 8, 16.0, 1e-3, 0.35), (7, 6, 40.0, 1e-3, 0.35), (16, 20, 12.0, 1e-3, 0.5)]


def ssao_depths(W, H, seed):
    """Few distinct depths (multiples of 1 / 64), a third of them lowered by exactly the threshold 1e-3 - a sample fl(q - 1e-3) seen
    from a centre q is an exact tie of `sample < centre - threshold` - with NaN, +inf and -inf among them."""
    r = scenes.SplitMix64(seed)
    z = np.round(r.uniform(W * H, -1.0, 1.0) * 64) / 64
    z = np.where(r.uniform(W * H) < 0.33, z - 1e-3, z)
    hole = r.uniform(W * H)
    z[hole < 0.04] = np.nan; z[(hole >= 0.04) & (hole < 0.10)] = np.inf; z[(hole >= 0.10) & (hole < 0.14)] = -np.inf
    n = W * H
    z[n // 3], z[n // 2], z[2 * n // 3] = np.nan, np.inf, -np.inf
    return np.ascontiguousarray(z.reshape(H, W))


@pytest.mark.parametrize("frame", [(1, 70), (70, 1), (7, 5), (35, 29)], ids=frame_id)
def test_ssao_paths_against_numpy(frame):
    """k_ssao on images narrower or lower than its 32-pixel tile - no block is interior, the halo is mostly outside the image, every
    sample of 1x70 is out of range in x unless its offset rounds to 0 - with the reference's parameters, a radius of 40 (direct
    z-buffer reads beyond the halo) and 16 x 20 samples (the literal path), against a plain numpy evaluation."""
    W, H = frame
    z = ssao_depths(W, H, 4300 + W)
    with Context(W, H, 3) as ctx:
        ctx.write_zbuffer(z)
        for params in SSAO_PARAMS:
            got = ctx.postprocess(zbuffer_image=False, ao=True, final=False, params=SsaoParams(*params))["ao"]
            want = _numpy_ssao(z, *params)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{frame} {params}: {len(bad)} differing bytes, first at {bad[:5].tolist()}"
            if params == SSAO_PARAMS[0]:
                assert np.array_equal(got, orc.ssao(z))


@pytest.mark.parametrize("frame", FIVE_FRAMES, ids=frame_id)
def test_blur_modulate_and_snapshot_on_the_resident_frame(frame):
    """framebuffer_blur with radius 1, 3 and 40 (larger than the frame) against image_ops_model, framebuffer_modulate with a host
    mask against shadow_model, and zbuffer_snapshot / draw / zbuffer_restore giving back the first z bits, at every pixel size."""
    W, H = frame
    mask = (scenes.SplitMix64(4400 + W).u64(W * H) & np.uint64(0xFF)).astype(np.uint8).reshape(H, W)
    mask.reshape(-1)[0] = 255; mask.reshape(-1)[-1] = 0
    for bpp in BPPS:
        with Context(W, H, bpp) as ctx:
            draw_dense_flat(ctx, W, H, bpp)
            fb, z, st = ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()
            for radius in (1, 3, 40):
                ctx.write_framebuffer(fb)
                ctx.framebuffer_blur(radius)
                got = ctx.read_framebuffer()
                assert np.array_equal(got, image_ops_model.gaussian_blur(fb, api.gaussian_kernel(radius))), (frame, bpp, radius)
            ctx.write_framebuffer(fb)
            ctx.framebuffer_modulate(mask)
            assert np.array_equal(ctx.read_framebuffer(), shadow_model.modulate(fb, mask)), (frame, bpp)
            assert np.array_equal(ctx.read_zbuffer().view(np.uint64), z.view(np.uint64)) and ctx.stats() == st
            ctx.zbuffer_snapshot(0)
            s = fg.case(W, H, "sparse", FLAT, bpp)
            for kind, u, clip, vary, col in s["draws"]:
                shifted = clip.copy(); shifted[:, [2, 6, 10]] = -0.95 * shifted[:, [3, 7, 11]]      # in front of everything
                ctx.draw(kind, shifted, vary, col, u)
            assert not np.array_equal(ctx.read_zbuffer().view(np.uint64), z.view(np.uint64))
            ctx.zbuffer_restore(0)
            assert np.array_equal(ctx.read_zbuffer().view(np.uint64), z.view(np.uint64)), (frame, bpp)
