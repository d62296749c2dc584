"""The radix scatters as loops over chunks: a scatter block takes the chunks b, b + grid, ... of its
pass, with the next chunk's loads in flight while it reorders and writes the current one.  Context.debug_radix_blocks(n) caps the
grids, so that a flush of a few chunks makes every block loop: one block that walks all chunks, two and three that share them
unevenly, as many blocks as chunks, more blocks than chunks, and the automatic grid.

Every flush here is checked twice: its records and lists against binning_model (the set of (tile, triangle, mask), triangle
numbers strictly increasing inside a tile, bounds inside [0, P)) and its frame, z bits and stats against the CPU oracle - all
exact.  Where several grids sort the same flush, vals, bmask, tile_start and tile_end are the same bytes for all of them.
"""
import os

import numpy as np
import pytest

import binning_model as bm
import cases
import test_direct_pairs_gpu as td
from test_stage_outputs_gpu import RADIX_BIG_CAP, ROOT, _flat, check_pairs, check_setup, flush_and_check
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import BIN_DIRECT, BIN_EXPAND, DBG_INFO, DBG_INFO_FIELDS, FLAT, Context, TrglError

pytestmark = pytest.mark.gpu

CHUNK = 4096                      # pairs per chunk while the pair buffers hold fewer than 4 M pairs; 8192 from there on
SORTED = ("vals", "bmask", "tile_start", "tile_end")


def chunks_of(pairs, chunk=CHUNK):
    return (pairs + chunk - 1) // chunk


def sorted_flush(ctx, case, m, want, max_blocks, mode=None, S=0, G=0, what=""):
    """one flush of the case on ctx with the scatter grids capped at max_blocks (and the binning forced to mode): records and lists
    against the model m, the frame against the oracle's `want`; returns the snapshot with the grids and the path taken in it"""
    ctx.debug_radix_blocks(max_blocks)
    if mode is not None:
        ctx.debug_binning(mode, S, G)
    ctx.reset_stats()
    ctx.clear(case["clear"], case["zclear"])
    s = td.flush(ctx, case, m=m, what=what)
    s["grids"], s["took"] = ctx.debug_radix_blocks(), ctx.debug_binning()
    cases.assert_same_frame(s["frame"], want, what=what)
    assert s["grids"]["first"] >= 1 and s["grids"]["last"] >= 1, (what, s["grids"])
    if max_blocks:
        # (the last pass is a dense one: a column of its table per chunk of the capacity)
        assert s["grids"]["last"] == min(max_blocks, chunks_of(s["info"]["capacity"], chunk_of(s))), (what, s["grids"], s["info"])
        assert s["grids"]["first"] <= max_blocks, (what, s["grids"])
    return s


def chunk_of(s):
    return 2 * CHUNK if s["info"]["capacity"] >= RADIX_BIG_CAP else CHUNK


def same_sorted(a, b, what):
    for k in SORTED:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"
    for x, y, name in zip(a["frame"], b["frame"], ("framebuffer", "z-buffer", "stats")):
        assert (x == y) if name == "stats" else (x.tobytes() == y.tobytes()), f"{what}: {name} differs"


# ---- loop edges --------------------------------------------------------------------------------------------------------
_loop = {}


def loop_scene():
    """544 x 544 (289 tiles: two passes of 5 bits), 12 000 triangles of 2-20 px, each followed by two copies wound the other way
    (rejected, our_gl.cpp:127): 141 setup blocks of about 85 live triangles, so that a group of 16 still fits a chunk"""
    if not _loop:
        W = H = 544
        clip, col = scenes.random_triangles(12_000, W, H, seed=6101, rmin=2, rmax=20)
        rows = np.repeat(clip, 3, axis=0)
        rows[1::3] = clip[:, [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7]]
        rows[2::3] = rows[1::3]
        case = _flat(W, H, rows, np.repeat(col, 3))
        _loop.update(case=case, m=bm.model(case), want=cases.run_oracle(case))
    return _loop


@pytest.mark.parametrize("mode,S,G", [(BIN_EXPAND, 0, 0), (BIN_DIRECT, 1024, 2), (BIN_DIRECT, 512, 16)])
def test_every_grid_sorts_the_same_lists(mode, S, G):
    """5-8 chunks per dense pass; the first pass of the direct path has a chunk per group of 2 (71 of them) or 16 (9) setup blocks.
    One block, two, three, one per chunk, five more than chunks, the automatic grid: the same bytes, the first of them kept for
    the other modes to be compared with"""
    sc = loop_scene()
    case, m = sc["case"], sc["m"]
    P = int(m.cnt.sum())
    chunks = chunks_of(P)
    assert 5 <= chunks <= 8 and m.tiles_x * m.tiles_y == 289, (P, chunks)
    blocks = td.per_block(dict(cnt=m.cnt))
    assert len(blocks) == 141 and blocks.max() <= 512 and np.add.reduceat(blocks, np.arange(0, 141, 16)).max() <= CHUNK, blocks
    with Context(case["width"], case["height"], case["bpp"]) as ctx:
        for mb in (1, 2, 3, chunks, chunks + 5, 0):
            what = f"mode {mode} S {S} G {G}, at most {mb} blocks"
            s = sorted_flush(ctx, case, m, sc["want"], mb, mode, S, G, what)
            assert s["info"]["P"] == P and s["info"]["capacity"] < RADIX_BIG_CAP
            assert s["took"] == dict(direct=mode == BIN_DIRECT, fell_back=False), (what, s["took"])
            if mode == BIN_DIRECT and mb:
                assert s["grids"]["first"] == min(mb, (141 + G - 1) // G), (what, s["grids"])
            same_sorted(s, sc.setdefault("first", s), what)


# ---- eight-wave blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(256, 192), (544, 544)])
def test_eight_wave_blocks_loop(W, H):
    """pair buffers of at least 4 M entries (a first flush of 2.1 M rejected triangles sizes them) sort in chunks of 8192: more
    than three chunks, walked by one block and by three - k_expand's chain, and the direct path with groups of four segments"""
    clip, col = scenes.random_triangles(20_000, W, H, seed=6201 + W, rmin=2, rmax=20)
    case = _flat(W, H, clip, col)
    m, want = bm.model(case), cases.run_oracle(case)
    P = int(m.cnt.sum())
    assert P > 3 * 8192 and td.per_block(dict(cnt=m.cnt)).max() <= 2048, P
    first = None
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, np.zeros((2_100_000, 12)))
        ctx.flush()
        assert ctx.debug_snapshot()["info"]["P"] == 0
        for mode, S, G in ((BIN_EXPAND, 0, 0), (BIN_DIRECT, 2048, 4)):
            for mb in (1, 3):
                what = f"8-wave blocks, mode {mode}, at most {mb} blocks"
                s = sorted_flush(ctx, case, m, want, mb, mode, S, G, what)
                assert s["info"]["capacity"] >= RADIX_BIG_CAP and s["info"]["P"] == P, s["info"]
                assert s["took"] == dict(direct=mode == BIN_DIRECT, fell_back=False), (what, s["took"])
                assert s["grids"]["first"] == mb, (what, s["grids"])
                first = first or s
                same_sorted(s, first, what)


# ---- one pair per triangle -------------------------------------------------------------------------------------------------
def tile_triangles(tiles, tiles_x, seed, size=10, z=None):
    """One clip row (UNIT_VIEWPORT) per entry of `tiles`: a triangle of `size` px well inside that tile, at a place of its own, so
    that the triangles of a tile overlap; depth z (0: every overlap is a tie, which the earlier triangle wins, our_gl.cpp:165)"""
    rng = np.random.default_rng(seed)
    tiles = np.asarray(tiles, np.int64)
    n = len(tiles)
    a = 32.0 * (tiles % tiles_x) + 2.25 + rng.integers(0, 27 - size, n)
    b = 32.0 * (tiles // tiles_x) + 2.25 + rng.integers(0, 27 - size, n)
    z = np.zeros(n) if z is None else z
    rows = np.empty((n, 12))
    for i in range(n):
        rows[i] = cases.screen_triangle((a[i], b[i]), (a[i] + size, b[i]), (a[i], b[i] + size), (z[i], z[i], z[i]))
    return rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 8192, 3 * 4096 + 1])
def test_chunk_boundaries(n):
    """N = P pairs: a last chunk of one pair, of a wave's round less or more by one, full chunks only.  k_expand's chain, and the
    direct path with segments of exactly a setup block's 256 pairs and groups of 16 - every full group is exactly one chunk"""
    W = H = 544
    rng = np.random.default_rng(6300 + n)
    case = _flat(W, H, tile_triangles(rng.integers(0, 289, n), 17, 6400 + n, size=3, z=rng.uniform(-0.9, 0.9, n)), viewport=cases.UNIT_VIEWPORT)
    m, want = bm.model(case), cases.run_oracle(case)
    assert int(m.cnt.sum()) == n and (m.cnt == 1).all()
    first = None
    with Context(W, H, 3) as ctx:
        for mode, S, G in ((BIN_EXPAND, 0, 0), (BIN_DIRECT, 256, 16)):
            for mb in (1, 2):
                what = f"{n} pairs, mode {mode}, at most {mb} blocks"
                s = sorted_flush(ctx, case, m, want, mb, mode, S, G, what)
                assert s["info"]["P"] == n and s["took"] == dict(direct=mode == BIN_DIRECT, fell_back=False), (what, s["took"])
                first = first or s
                same_sorted(s, first, what)


PATTERN_N = 5000


def pattern_tiles(name, T):
    """tile ids of the PATTERN_N triangles, in submission order, on a frame of T tiles"""
    i = np.arange(PATTERN_N)
    A, B = T // 3, T - 2
    if name == "one_tile":
        return np.full(PATTERN_N, A)
    if name == "cycle_64":
        return (i % 64) * (T // 64) + 1
    if name == "alternating":
        return np.where(i & 1, B, A)
    if name == "runs_33_31":
        return np.where(i % 64 < 33, A, B)
    if name == "descending":
        return (T - 1 - i) % T
    if name == "skewed":
        return (T * np.random.default_rng(6500).random(PATTERN_N) ** 4).astype(np.int64)
    raise KeyError(name)


FRAMES = {544: 3, 512: 3, 2912: 1}          # side -> bpp: 289 tiles (5 + 5 bits), 256 tiles (one pass of 8), 8281 tiles (7 + 7)


@pytest.fixture(scope="module")
def frame_ctx():
    made = {}

    def get(side):
        if side not in made:
            made[side] = Context(side, side, FRAMES[side])
        return made[side]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("side", list(FRAMES))
@pytest.mark.parametrize("name", ["one_tile", "cycle_64", "alternating", "runs_33_31", "descending", "skewed"])
def test_digit_patterns_keep_submission_order(name, side, frame_ctx):
    """5000 triangles of one pair each, overlapping inside their tiles at equal depth: a rank that is not stable changes which
    triangle a tie leaves in the frame.  Two chunks, sorted by the automatic grid and by one block, from k_expand's pairs and from
    the segments"""
    tiles_x = side // 32
    T = tiles_x * tiles_x
    tiles = pattern_tiles(name, T)
    assert tiles.min() >= 0 and tiles.max() < T
    case = _flat(side, side, tile_triangles(tiles, tiles_x, 6600 + side), viewport=cases.UNIT_VIEWPORT, bpp=FRAMES[side])
    m, want = bm.model(case), cases.run_oracle(case)
    assert int(m.cnt.sum()) == PATTERN_N and (m.cnt == 1).all() and chunks_of(PATTERN_N) == 2
    ctx = frame_ctx(side)
    first = None
    for mode, S, G in ((BIN_EXPAND, 0, 0), (BIN_DIRECT, 256, 8)):
        for mb in (0, 1):
            what = f"{name} on {side}^2, mode {mode}, at most {mb} blocks"
            s = sorted_flush(ctx, case, m, want, mb, mode, S, G, what)
            assert s["took"] == dict(direct=mode == BIN_DIRECT, fell_back=False), (what, s["took"])
            first = first or s
            same_sorted(s, first, what)
    ts, te = first["tile_start"].astype(np.int64), first["tile_end"].astype(np.int64)
    assert np.array_equal(np.flatnonzero(te > ts), np.unique(tiles))


# ---- sequences on one context, two blocks at most ------------------------------------------------------------------------------
def test_fall_back_with_two_blocks():
    """a direct flush whose segments are too small: the scatter of the segments does nothing, k_expand's chain sorts the flush"""
    W = H = 256
    clip, col = scenes.random_triangles(8000, W, H, seed=6701, rmin=2, rmax=40)
    case = _flat(W, H, clip, col)
    m, want = bm.model(case), cases.run_oracle(case)
    assert td.per_block(dict(cnt=m.cnt)).max() > 64 and chunks_of(int(m.cnt.sum())) >= 3
    with Context(W, H, 3) as ctx:
        s = sorted_flush(ctx, case, m, want, 2, BIN_DIRECT, 64, 2, "segments too small")
        assert s["took"] == dict(direct=True, fell_back=True) and s["grids"] == dict(first=2, last=2), (s["took"], s["grids"])
        e = sorted_flush(ctx, case, m, want, 0, BIN_EXPAND, 0, 0, "k_expand, automatic grid")
        same_sorted(s, e, "fallen back against k_expand's chain")


def test_long_short_and_clear_only_flushes_with_two_blocks():
    """a long flush, then short lists (stale words behind P, stale bounds, fewer chunks than blocks), a flush that only clears, a
    few pairs again"""
    W = H = 256
    big, cb = scenes.random_triangles(400, W, H, seed=6711, rmin=80, rmax=300)
    with Context(W, H, 3) as ctx:
        ctx.debug_radix_blocks(2)
        s, _ = flush_and_check(_flat(W, H, big, cb), ctx=ctx, frame=False, what="long")
        long_P = s["info"]["P"]
        assert chunks_of(long_P) >= 3 and ctx.debug_radix_blocks()["last"] == 2
        small, cs = scenes.random_triangles(300, W, H, seed=6712, rmin=1, rmax=6)
        ctx.clear()
        s, _ = flush_and_check(_flat(W, H, small, cs), ctx=ctx, what="short lists")
        assert 0 < s["info"]["P"] < CHUNK < long_P
        ctx.clear()
        ctx.flush()
        e = ctx.debug_snapshot()
        assert e["info"]["P"] == 0 and len(e["vals"]) == 0 and (e["tile_end"] <= e["tile_start"]).all()
        few, cf = scenes.random_triangles(7, W, H, seed=6713, rmin=2, rmax=20)
        s, _ = flush_and_check(_flat(W, H, few, cf), ctx=ctx, what="few after the clear")
        assert 0 < s["info"]["P"] < 100


def test_outgrown_pair_buffers_with_two_blocks():
    """a flush with more pairs than the buffers hold: the scatters queued first do nothing, the buffers grow, the binning runs again"""
    W = H = 256
    small, cs = scenes.random_triangles(300, W, H, seed=6721, rmin=1, rmax=6)
    big, cb = scenes.random_triangles(700, W, H, seed=6722, rmin=40, rmax=300)
    case = _flat(W, H, big, cb)
    m = bm.model(case)
    with Context(W, H, 3) as ctx:
        ctx.debug_radix_blocks(2)
        ctx.draw(FLAT, small, colors=cs)
        ctx.flush()
        cap0 = ctx.debug_snapshot()["info"]["capacity"]
        td.submit(ctx, case)
        ctx.flush_begin()
        info = dict(zip(DBG_INFO_FIELDS, (int(v) for v in ctx._debug_read(DBG_INFO, np.int64))))
        assert info["capacity"] == cap0 < info["P"] == m.cnt.sum(), (info, cap0)
        with pytest.raises(TrglError):
            ctx.debug_snapshot()
        ctx.flush_end()
        s = ctx.debug_snapshot()
        assert s["info"]["capacity"] >= s["info"]["P"] > cap0 and chunks_of(s["info"]["P"]) >= 3
        check_setup(s, m, "grown")
        check_pairs(s, m, "grown")
        assert ctx.debug_radix_blocks()["last"] == 2
        got = (ctx.read_framebuffer(), ctx.read_zbuffer())
    both = cases.make_case(W, H, [(FLAT, None, small, None, cs), (FLAT, None, big, None, cb)])
    cases.assert_same_frame(got, cases.run_oracle(both), stats=False, what="grown")


def test_hook_is_not_part_of_the_public_interface():
    from tinyrenderder_amd import api
    assert "trgl_debug_radix_blocks" not in api.SYMBOLS
    with open(os.path.join(ROOT, "include", "trgl.h")) as f:
        assert "trgl_debug_radix_blocks" not in f.read()
