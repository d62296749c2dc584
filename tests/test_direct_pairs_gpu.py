"""The direct path of the binning: k_setup leaves every setup block's pairs in a segment of S slots and the
first radix pass sorts groups of G segments; a flush that does not fit falls back to k_expand and the dense passes.

Segment and group sizes are set through Context.debug_binning() to small values, so that the edges - a full segment, a full
group, one pair more, empty blocks and groups, a partial last group - are reached with tens to hundreds of triangles on frames
of 64^2 to 256^2 (frames of 544^2 and 1024^2 where two radix passes are the point: more than 256 tiles).  Every case is flushed in halves with a snapshot
in between (test_stage_outputs_gpu.snapshots: the pending and the complete flush agree), its records and lists are compared with
binning_model (the set of (tile, triangle, mask), triangles strictly increasing per tile, bounds inside [0, P)), its frame, z
bits and stats with the CPU oracle - all exact - and, where it can run both ways, the arrays of the forced direct path equal
those of the forced k_expand chain.

Where per-block pair counts are the point they are stated, built with blocks_case() from rectangles of whole tiles, and asserted
from the snapshot (per_block) before the path taken is.  The automatic choice is held against Rule, DESIGN.md's rule restated:
INFO reports the sizes a flush was given (seg_S, seg_G), so every flush of a sequence is compared with the prediction.
tests/test_direct_pairs_big_gpu.py runs the same kind of case over pair buffers of at least 4 M entries (radix blocks of 8 waves).
"""
from fractions import Fraction

import numpy as np
import pytest

import binning_model as bm
import cases
from test_stage_outputs_gpu import RADIX_BIG_CAP, _flat, check_pairs, check_setup, snapshots, submit
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import BIN_AUTO, BIN_DIRECT, BIN_EXPAND, DBG_INFO, DBG_INFO_FIELDS, FLAT, Context, TrglError

pytestmark = pytest.mark.gpu

BLOCK = 256           # triangles per setup block
CHUNK = 4096          # pairs per block of a radix pass while the pair buffers hold fewer than 4 M pairs
LIST_KEYS = ("cnt", "tilebox", "vals", "bmask", "tile_start", "tile_end")


def tri(tx0, ty0, tx1, ty1, z=0.0, accept=True):
    """A clip row for UNIT_VIEWPORT whose clamped bbox touches exactly the tiles tx0..tx1 x ty0..ty1; accept=False: wound the
    other way (our_gl.cpp:127 rejects it)"""
    a, b, c, d = 32 * tx0 + 1.25, 32 * ty0 + 1.25, 32 * tx1 + 20.5, 32 * ty1 + 20.5
    p1, p2 = ((c, b), (a, d)) if accept else ((a, d), (c, b))
    return cases.screen_triangle((a, b), p1, p2, (z, z * 0.5, -z))


def unit_case(W, H, rows, **kw):
    clip = np.array(rows, np.float64).reshape(-1, 12)
    return _flat(W, H, clip, viewport=cases.UNIT_VIEWPORT, **kw)


def depths(n, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, n)


def pending_info(ctx):
    return dict(zip(DBG_INFO_FIELDS, (int(v) for v in ctx._debug_read(DBG_INFO, np.int64))))


def flush(ctx, case, m=None, strip=None, interleave=None, what="", draws=None, while_pending=None):
    """one flush of the case on ctx, in halves; records, lists, frame checked; returns the snapshot with the frame in it.
    while_pending(ctx, info): called between flush_begin and flush_end with the INFO words of the pending flush"""
    m = m or bm.model(case, strip=strip, interleave=interleave, draws=draws)
    submit(ctx, case, strip, interleave, draws=draws)
    if while_pending is not None:
        ctx.flush_begin()
        while_pending(ctx, pending_info(ctx))
    s = snapshots(ctx)
    check_setup(s, m, what)
    check_pairs(s, m, what)
    s["frame"] = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats())
    s["model"] = m
    return s


def check_frame(s, case, strip=None, interleave=None, what=""):
    m = s["model"]
    rows = strip if interleave is None else [(32 * int(ty), min(32 * int(ty) + 32, m.H)) for ty in np.flatnonzero(m.owned_rows)]
    cases.assert_same_frame(s["frame"], cases.run_oracle(case, strip=strip if interleave is None else None), rows=rows,
                            stats=interleave is None, what=what)


def one(case, mode, S=0, G=0, strip=None, interleave=None, what="", ctx=None, while_pending=None):
    """one flush with the binning forced to `mode`, on a context of its own or (ctx) on a shared one, whose stats are reset"""
    own = ctx is None
    ctx = ctx or Context(case["width"], case["height"], case["bpp"])
    try:
        ctx.debug_binning(mode, S, G)
        if not own:
            ctx.reset_stats()
        ctx.clear(case["clear"], case["zclear"])
        s = flush(ctx, case, strip=strip, interleave=interleave, what=what, while_pending=while_pending)
        s["took"] = ctx.debug_binning()
    finally:
        if own:
            ctx.close()
    assert s["took"] == dict(direct=bool(s["info"]["direct"]), fell_back=bool(s["info"]["fell_back"]))
    given = (S, G) if mode == BIN_DIRECT and not s["info"]["wide"] else (0, 0) if mode == BIN_EXPAND else None
    assert given is None or (s["info"]["seg_S"], s["info"]["seg_G"]) == given, (what, s["info"])
    return s


def same_lists_and_frame(d, e, what):
    for k in LIST_KEYS:
        assert np.array_equal(d[k], e[k]), f"{what}: {k} differs between the direct path and k_expand's chain"
    for a, b, name in zip(d["frame"], e["frame"], ("framebuffer", "z-buffer", "stats")):
        assert (a == b) if name == "stats" else (a.tobytes() == b.tobytes()), f"{what}: {name} differs between the two paths"


def both_ways(case, S, G, fell_back, strip=None, interleave=None, what="", ctx=None, counts=None, while_pending=None):
    """forced direct (which falls back or not, as stated) and forced k_expand: each exact against the model and the oracle, and
    the same arrays.  counts: the pairs per setup block the case intends, asserted before the path is"""
    d = one(case, BIN_DIRECT, S, G, strip, interleave, what + " direct", ctx, while_pending)
    assert counts is None or list(per_block(d)) == list(counts), (what, per_block(d), counts)
    assert d["took"] == dict(direct=True, fell_back=fell_back), (what, d["took"], per_block(d))
    e = one(case, BIN_EXPAND, 0, 0, strip, interleave, what + " k_expand", ctx)
    assert e["took"] == dict(direct=False, fell_back=False), (what, e["took"])
    check_frame(d, case, strip, interleave, what + " direct")
    same_lists_and_frame(d, e, what)
    return d


def per_block(s):
    c = s["cnt"]
    return np.add.reduceat(c, np.arange(0, len(c), BLOCK)) if len(c) else np.zeros(0, np.int64)


# ---- setup blocks with stated pair counts -------------------------------------------------------------------------------
def block_rows(c, T, z, big=16, n=BLOCK, shift=0):
    """n clip rows (one setup block) with exactly c pairs on a frame of T x T whole tiles: rectangles of w x h tiles, of at most
    `big` tiles unless c needs larger ones, at varying places; the other rows are wound the other way.  The accepted rows start
    at row `shift` of the block."""
    shapes = {}
    for h in range(1, T + 1):
        for w in range(h, T + 1):
            shapes.setdefault(w * h, (w, h))
    rows = [tri(0, 0, 0, 0, 0.1, accept=False)] * n
    rem, k = c, 0
    while rem:
        assert k < n, f"{c} pairs do not fit {n} triangles on {T} x {T} tiles"
        need = -(-rem // (n - k))
        cap = max(big, min(t for t in shapes if t >= need))
        w, h = shapes[max(t for t in shapes if t <= min(rem, cap))]
        x0, y0 = (5 * k + shift) % (T - w + 1), (3 * k + k // T) % (T - h + 1)
        rows[(k + shift) % n] = tri(x0, y0, x0 + w - 1, y0 + h - 1, z[k])
        rem -= w * h
        k += 1
    return rows


def blocks_case(W, H, counts, seed, big=16, last=BLOCK):
    """one draw of len(counts) setup blocks (the last of `last` triangles) with counts[b] pairs in block b"""
    T = min(W, H) // 32
    clip = np.tile(tri(0, 0, 0, 0, 0.1, accept=False), (len(counts) * BLOCK, 1))
    for b in np.flatnonzero(counts):
        n = last if b == len(counts) - 1 else BLOCK
        clip[b * BLOCK:b * BLOCK + n] = block_rows(int(counts[b]), T, depths(BLOCK, seed + int(b)), big, n, shift=(37 * int(b)) % n)
    return _flat(W, H, clip[:(len(counts) - 1) * BLOCK + last], viewport=cases.UNIT_VIEWPORT)


def group_sums(counts, G):
    return [int(sum(counts[i:i + G])) for i in range(0, len(counts), G)]


# ---- sizes of a flush ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_direct_at_setup_block_edges(n):
    clip, col = scenes.random_triangles(n, 128, 96, seed=900 + n, rmin=2, rmax=12)
    s = both_ways(_flat(128, 96, clip, col), 2048, 2, False, what=f"{n} triangles")
    assert s["info"]["N"] == n and 0 < s["info"]["P"]


def test_direct_three_draws_groups_span_draws():
    """draws of 300, 70 and 523 triangles are 2 + 1 + 3 setup blocks; groups of 4 hold blocks of two or three draws"""
    W, H = 160, 128
    parts = [scenes.random_triangles(n, W, H, seed=910 + i, rmin=2, rmax=12) for i, n in enumerate((300, 70, 523))]
    case = cases.make_case(W, H, [(FLAT, None, clip, None, col) for clip, col in parts])
    s = both_ways(case, 1024, 4, False, what="three draws")
    assert s["info"]["N"] == 893 and s["model"].draw.max() == 2


@pytest.mark.parametrize("blocks,G", [(3, 3), (4, 3), (5, 2), (2, 16)])
def test_direct_block_count_against_group_size(blocks, G):
    """as many setup blocks as a group holds, one more (a last group of one block), a partial last group, one partial group"""
    n = blocks * BLOCK - 7
    clip, col = scenes.random_triangles(n, 128, 128, seed=920 + blocks, rmin=1, rmax=14)
    s = both_ways(_flat(128, 128, clip, col), 1024, G, False, what=f"{blocks} blocks, groups of {G}")
    assert len(per_block(s)) == blocks


@pytest.mark.parametrize("S,fell_back", [(2048, False), (64, True)])
def test_direct_two_radix_passes(S, fell_back):
    """more than 256 tiles (17 x 17): the first pass reads the segments and is not the last; when the flush does not fit, the dense
    last pass queued behind it must leave the tile bounds alone as well"""
    W = H = 544
    clip, col = scenes.random_triangles(1500, W, H, seed=931, rmin=2, rmax=30)
    s = both_ways(_flat(W, H, clip, col), S, 3, fell_back, what="two passes")
    assert s["info"]["tiles_x"] * s["info"]["tiles_y"] > 256 and (per_block(s).max() <= S) == (not fell_back)


def test_second_flush_falls_back_with_two_radix_passes():
    """automatic sizes on a frame of 1024 tiles: a flush of small triangles runs direct, the larger triangles behind it do not fit
    the sizes it leaves and fall back - over pair buffers that still hold the first flush's pairs"""
    W = H = 1024
    first = _flat(W, H, *scenes.random_triangles(12000, W, H, seed=932, rmin=1, rmax=8))
    second = _flat(W, H, *scenes.random_triangles(1200, W, H, seed=933, rmin=20, rmax=60))
    with Context(W, H, 3) as ctx:
        ctx.clear(first["clear"], first["zclear"])
        a = flush(ctx, first, what="first flush")
        assert ctx.debug_binning() == dict(direct=True, fell_back=False)
        ctx.reset_stats()
        ctx.clear(second["clear"], second["zclear"])
        b = flush(ctx, second, what="second flush")
        assert ctx.debug_binning() == dict(direct=True, fell_back=True), per_block(b)
    check_frame(b, second, what="second flush")


# ---- empty blocks and groups --------------------------------------------------------------------------------------------
def test_direct_rejected_blocks_and_groups():
    """5 blocks in groups of 2: block 1 (half of group 0) and blocks 2, 3 (all of group 1) hold rejected triangles only"""
    W = H = 128
    z = depths(5 * BLOCK, 941)
    rows = [tri(i % 4, (i // 4) % 4, i % 4, (i // 4) % 4, z[i], accept=not (BLOCK <= i < 4 * BLOCK)) for i in range(5 * BLOCK - 30)]
    s = both_ways(unit_case(W, H, rows), 256, 2, False, what="rejected blocks")
    assert list(per_block(s)) == [256, 0, 0, 0, 226]


def test_direct_no_pairs_at_all():
    rows = [tri(0, 0, 1, 1, 0.1, accept=False)] * 300
    s = both_ways(unit_case(64, 64, rows), 8, 2, False, what="all rejected")
    assert s["info"]["P"] == 0


# ---- a full segment, a full group, one pair more ------------------------------------------------------------------------
@pytest.mark.parametrize("extra,fell_back", [(0, False), (1, True)])
def test_direct_block_with_S_pairs_and_one_more(extra, fell_back):
    """S = 64: a block of 64 (+ 1) one-tile triangles among rejected ones, and a second block below S"""
    z = depths(400, 951)
    rows = [tri(i % 2, i // 2 % 2, i % 2, i // 2 % 2, z[i], accept=i < 64 + extra or i >= 370) for i in range(400)]
    s = both_ways(unit_case(64, 64, rows), 64, 2, fell_back, what=f"S + {extra} pairs in a block")
    assert list(per_block(s)) == [64 + extra, 30]


@pytest.mark.parametrize("extra,fell_back", [(0, False), (1, True)])
def test_direct_group_at_the_radix_chunk_and_one_above(extra, fell_back):
    """two blocks of 256 triangles of 8 tiles each are 4096 pairs, the chunk of a radix block; one triangle of 9 tiles makes
    4097, which no block of the first pass may hold (S = 2052 holds either block)"""
    W = H = 256
    z = depths(2 * BLOCK, 961)
    rows = [tri(0, i % 8, 7, i % 8, z[i]) for i in range(2 * BLOCK)]
    if extra:
        rows[300] = tri(0, 3, 2, 5, z[300])
    s = both_ways(unit_case(W, H, rows), 2052, 2, fell_back, what=f"group of {CHUNK + extra}")
    assert per_block(s).sum() == CHUNK + extra and s["info"]["capacity"] < (4 << 20)


def test_direct_one_triangle_beyond_the_segment():
    """a single triangle of 16 tiles, segments of 8 slots"""
    s = both_ways(unit_case(128, 128, [tri(0, 0, 3, 3, 0.3)]), 8, 2, True, what="16 tiles, S = 8")
    assert list(s["cnt"]) == [16]


def test_direct_wave_written_triangles():
    """triangles of more than 8 tiles (written by the whole wave) between small ones, all inside the segments"""
    z = depths(300, 971)
    rows = [tri(i % 4, i // 4 % 4, i % 4, i // 4 % 4, z[i]) for i in range(300)]
    for i, box in ((3, (0, 0, 3, 2)), (64, (0, 0, 3, 3)), (65, (1, 0, 3, 3)), (255, (0, 1, 2, 3)), (256, (0, 0, 3, 3)), (299, (0, 0, 2, 2))):
        rows[i] = tri(*box, z[i])
    s = both_ways(unit_case(128, 128, rows), 512, 2, False, what="wave-written triangles")
    assert (s["cnt"] > 8).sum() == 6 and ((s["cnt"] > 0) & (s["cnt"] <= 8)).any()


# ---- contexts that own part of the frame --------------------------------------------------------------------------------
def tight_sizes(case, G, strip=None, interleave=None):
    """S = the largest pair count of a setup block (the model's), rounded up to a multiple of 4: the fullest segment has at most
    3 free slots; asserts that every group of G blocks stays inside the radix chunk"""
    c = bm.model(case, strip=strip, interleave=interleave).cnt
    pb = np.add.reduceat(c, np.arange(0, len(c), BLOCK))
    assert max(pb[i:i + G].sum() for i in range(0, len(pb), G)) <= CHUNK and pb.max() > 0, pb
    return (int(pb.max()) + 3) & ~3


@pytest.mark.parametrize("G", [2, 3])
def test_direct_strip_context(G):
    """a strip of a 4 x 4-tile frame, 5 setup blocks in groups of 2 or 3 (a partial last group), the fullest block fills its segment"""
    clip, col = scenes.random_triangles(5 * BLOCK - 11, 128, 128, seed=981, rmin=2, rmax=36)
    case = _flat(128, 128, clip, col)
    S = tight_sizes(case, G, strip=(40, 100))
    s = both_ways(case, S, G, False, strip=(40, 100), what=f"strip, S = {S}, G = {G}")
    assert 0 < s["info"]["P"] < bm.model(case).cnt.sum() and S - 4 < per_block(s).max() <= S and (s["cnt"] > 8).any()


@pytest.mark.parametrize("G", [2, 3])
def test_direct_interleaved_bands(G):
    """rank 1 of 2 with bands of one tile row: block_pairs walks only owned rows (il_nth_owned_from), the groups hold 2 or 3 segments"""
    clip, col = scenes.random_triangles(5 * BLOCK - 11, 128, 256, seed=982, rmin=2, rmax=70)
    case = _flat(128, 256, clip, col)
    S = tight_sizes(case, G, interleave=(32, 1, 2))
    s = both_ways(case, S, G, False, interleave=(32, 1, 2), what=f"bands, S = {S}, G = {G}")
    assert 0 < s["info"]["P"] and s["info"]["il_tiles"] > 0 and S - 4 < per_block(s).max() <= S and (s["cnt"] > 8).any()


@pytest.mark.parametrize("kw", [dict(strip=(40, 100)), dict(interleave=(32, 1, 2))], ids=["strip", "bands"])
def test_direct_partial_ownership_one_pair_too_many(kw):
    """the same contexts with a segment 4 slots short of the fullest block: the flush falls back, and is exact"""
    clip, col = scenes.random_triangles(3 * BLOCK, 128, 160, seed=984, rmin=2, rmax=40)
    case = _flat(128, 160, clip, col)
    S = tight_sizes(case, 2, **kw)
    s = both_ways(case, S - 4, 2, True, what=f"{list(kw)[0]}, S = {S - 4}", **kw)
    assert per_block(s).max() > S - 4


def test_wide_frame_takes_k_expand():
    """more than 65536 tiles: forced direct or not, k_expand's chain runs, and nothing counts as a fallback"""
    W = H = 8224
    clip, col = scenes.random_triangles(200, W, H, seed=983, rmin=8, rmax=300)
    case = _flat(W, H, clip, col, bpp=1)
    with Context(W, H, 1) as ctx:
        ctx.debug_binning(BIN_DIRECT, 1024, 2)
        ctx.clear(case["clear"], case["zclear"])
        submit(ctx, case)
        s = snapshots(ctx)
        took = ctx.debug_binning()
    m = bm.model(case)
    check_setup(s, m, "wide")
    check_pairs(s, m, "wide")
    assert s["info"]["wide"] == 1 and took == dict(direct=False, fell_back=False)


# ---- one context, several flushes ---------------------------------------------------------------------------------------
def test_direct_small_flush_over_stale_segments():
    """a flush of three full blocks, then one of 40 triangles on the same context: the segments still hold the first one's words"""
    W = H = 128
    big = _flat(W, H, *scenes.random_triangles(3 * BLOCK, W, H, seed=991, rmin=2, rmax=12))
    small = _flat(W, H, *scenes.random_triangles(40, W, H, seed=992, rmin=2, rmax=10))
    with Context(W, H, 3) as ctx:
        ctx.debug_binning(BIN_DIRECT, 1024, 2)
        ctx.clear(big["clear"], big["zclear"])
        a = flush(ctx, big, what="large flush")
        ctx.reset_stats()
        ctx.clear(small["clear"], small["zclear"])
        b = flush(ctx, small, what="small flush")
        assert a["info"]["direct"] == b["info"]["direct"] == 1 and a["info"]["fell_back"] == b["info"]["fell_back"] == 0
    assert a["info"]["P"] > 4 * b["info"]["P"] > 0
    check_frame(b, small, what="small flush")


def test_forced_direct_after_a_fallback_is_direct_again():
    """forced sizes: a flush that does not fit falls back, the next one that fits runs direct; both exact"""
    W = H = 128
    z = depths(300, 993)
    first = unit_case(W, H, [tri(0, 0, 3, 3, z[i]) for i in range(20)])             # 320 pairs in one block, S = 256
    second = unit_case(W, H, [tri(i % 4, i // 4 % 4, i % 4, i // 4 % 4, z[i]) for i in range(300)])
    with Context(W, H, 3) as ctx:
        ctx.debug_binning(BIN_DIRECT, 256, 2)
        ctx.clear(first["clear"], first["zclear"])
        a = flush(ctx, first, what="flush that falls back")
        assert ctx.debug_binning() == dict(direct=True, fell_back=True)
        check_frame(a, first, what="flush that falls back")
        ctx.reset_stats()
        ctx.clear(second["clear"], second["zclear"])
        b = flush(ctx, second, what="flush that fits")
        assert ctx.debug_binning() == dict(direct=True, fell_back=False)
        check_frame(b, second, what="flush that fits")


def test_automatic_choice_after_a_fallback():
    """The written rule, on a fresh context: the first flush is sized for 512 pairs per block (S = 896); one
    block of 1024 pairs falls back; the next flush stays on k_expand's chain while its counts are checked against the sizes its
    predecessor gives (S = 1664, groups of 3); they fit, so the third is direct."""
    W = H = 64
    z = depths(BLOCK, 994)
    case = unit_case(W, H, [tri(0, 0, 1, 1, z[i]) for i in range(BLOCK)])
    took = []
    with Context(W, H, 3) as ctx:
        assert ctx.debug_binning(BIN_AUTO) == dict(direct=False, fell_back=False)
        for k in range(3):
            ctx.reset_stats()
            ctx.clear(case["clear"], case["zclear"])
            s = flush(ctx, case, what=f"flush {k}")
            took.append(ctx.debug_binning())
            assert list(per_block(s)) == [1024]
        check_frame(s, case, what="third flush")
    assert took == [dict(direct=True, fell_back=True), dict(direct=False, fell_back=False), dict(direct=True, fell_back=False)], took


def test_snapshot_of_a_pending_flush_that_fell_back():
    """debug_snapshot() between flush_begin and flush_end of a flush that fell back: k_expand's chain is queued for it, and the
    lists equal those of the complete flush (snapshots() compares them) and of a context that never tried the direct path"""
    clip, col = scenes.random_triangles(600, 128, 128, seed=995, rmin=2, rmax=40)
    case = _flat(128, 128, clip, col)
    with Context(128, 128, 3) as ctx:
        ctx.debug_binning(BIN_DIRECT, 16, 2)
        ctx.clear(case["clear"], case["zclear"])
        submit(ctx, case)
        ctx.flush_begin()
        pend = ctx.debug_snapshot()
        assert pend["info"]["pending"] == 1 and pend["info"]["direct"] == 1 and pend["info"]["fell_back"] == 1
        assert pend["info"]["P"] <= pend["info"]["capacity"]
        m = bm.model(case)
        check_setup(pend, m, "pending")
        check_pairs(pend, m, "pending")
        ctx.flush_end()
        done = ctx.debug_snapshot()
        frame = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats())
    for k in LIST_KEYS:
        assert np.array_equal(pend[k], done[k]), f"{k} changed between the pending and the complete flush"
    e = one(case, BIN_EXPAND, what="k_expand")
    for k in LIST_KEYS:
        assert np.array_equal(done[k], e[k]), k
    cases.assert_same_frame(frame, cases.run_oracle(case), what="fell back while pending")


# ---- more pairs than the pair buffers hold ------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,fell_back", [(0, False), (4, True)])
def test_direct_over_capacity_that_fits_the_segments(extra, fell_back):
    """A first flush of 5 blocks of 2048 pairs (256 triangles of 8 tiles; one block of 2052 with extra) has more pairs than the
    2 per triangle + 4096 (+ headroom) its pair buffers get: the chain queued by flush_begin does nothing.  S = 2048, G = 2: the
    flush fits its segments and groups, so flush_end grows the buffers and queues the direct chain again over the segments
    k_setup has written (over && direct && !fell in settle_binning); with the block of S + 4 it is k_expand's chain instead."""
    counts = [2048, 2048, 2048 + extra, 2048, 2048]
    case = blocks_case(256, 256, counts, 1001, big=8)
    assert max(counts) <= 2048 + extra and max(group_sums(counts, 2)) <= CHUNK + extra
    seen = {}

    def while_pending(ctx, info):
        seen.update(info)
        assert info["P"] == sum(counts) > info["capacity"] and info["direct"] == 1 and info["fell_back"] == int(fell_back), info
        assert (info["seg_S"], info["seg_G"]) == (2048, 2)
        with pytest.raises(TrglError):
            ctx.debug_snapshot()

    d = both_ways(case, 2048, 2, fell_back, what=f"over capacity, fullest block {2048 + extra}", counts=counts, while_pending=while_pending)
    assert d["info"]["capacity"] >= d["info"]["P"] > seen["capacity"] > 0 and d["info"]["capacity"] < RADIX_BIG_CAP


# ---- k_chunk_spine's checks ---------------------------------------------------------------------------------------------
SPINE16 = ([512, 0, 256, 256] * 4, [1024, 0, 0, 0] + [256] * 12, [2048, 1024, 1024])       # 35 blocks: 4096 pairs in each chunk of 16


@pytest.mark.parametrize("chunk", [None, 0, 1, 2])
def test_direct_groups_of_16_checked_in_the_scan_loop(chunk):
    """G = 16: the groups are k_chunk_spine's own chunks of 16 block sums, checked where it scans them - two full chunks through
    the vector loads, the last chunk of 3 blocks through the scalar branch.  Every chunk holds exactly 4096 pairs (direct); one
    pair more in chunk 0, 1 or the partial one falls back.  No block exceeds S = 2048 in any run."""
    parts = [list(c) for c in SPINE16]
    if chunk is not None:
        parts[chunk][-1] += 1
    counts = sum(parts, [])
    assert len(counts) == 35 and max(counts) <= 2048
    assert group_sums(counts, 16) == [CHUNK + (chunk == k) for k in range(3)]
    both_ways(blocks_case(128, 128, counts, 1011, last=200), 2048, 16, chunk is not None, what=f"35 blocks, one pair more in chunk {chunk}", counts=counts)


@pytest.mark.parametrize("extra,fell_back", [(0, False), (4, True)])
def test_direct_more_groups_than_spine_threads(extra, fell_back):
    """G = 2 over 2050 setup blocks (524800 triangles, all but a few wound the other way) are 1025 groups, one per thread of
    k_chunk_spine's 1024: group 1024 (blocks 2048 and 2049) is the second trip of thread 0.  It holds 4096 pairs (direct) or
    4104 in two blocks of 2052 = S (falls back); a few pairs sit in other groups, none of them near a limit."""
    counts = np.zeros(2050, np.int64)
    counts[[0, 1023, 2046, 2047]] = [40, 7, 300, 1]
    counts[2048:] = 2048 + extra
    assert counts.max() <= 2052 and group_sums(counts, 2)[1024] == CHUNK + 2 * extra and max(group_sums(counts, 2)[:1024]) <= 301
    d = both_ways(blocks_case(256, 256, counts, 1021, big=8), 2052, 2, fell_back, what=f"1025 groups, the last of {CHUNK + 2 * extra}", counts=counts)
    assert d["info"]["N"] == 2050 * BLOCK


# ---- segment sizes of the kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 544])
def test_direct_segment_lengths_around_the_histogram_tail(W):
    """k_radix_hist_seg counts the first 512 words of a segment from two loads issued ahead and the rest in a loop of 256 words
    per trip: segments of 511, 512, 513 (no trip, none, one), 767, 768, 769 (one, one, two) and 1024 = S pairs, G = 4, each on
    another wave of its block.  On 544^2 (289 tiles) the first pass is not the last."""
    counts = [513, 767, 511, 1024, 769, 512, 768]
    assert max(group_sums(counts, 4)) <= CHUNK
    d = both_ways(blocks_case(W, W, counts, 1031, big=4), 1024, 4, False, what=f"hist tail, {W}^2", counts=counts)
    assert (d["info"]["tiles_x"] * d["info"]["tiles_y"] > 256) == (W == 544)


# ---- the automatic choice -----------------------------------------------------------------------------------------------
class Rule:
    """The rule of the automatic choice as DESIGN.md section 3 writes it.  a = pairs per setup block of the previous flush that
    had triangles (at least 1; 512 before the first); S = 1.5 a + 128 rounded down to an integer and up to a multiple of 64;
    G = min(16, floor(0.9 chunk / a)), chunk = 8192 pairs while the pair buffers hold at least 4 M pairs, else 4096; no sizes
    when S > 4096 or G < 2.  A flush that is given sizes runs direct unless the context holds: it holds from a flush that fell
    back (did not fit its sizes) until a flush fits the sizes it is checked against, and that flush still takes k_expand."""

    def __init__(self):
        self.a, self.hold = Fraction(512), False

    def sizes(self, capacity):
        chunk = 8192 if capacity >= RADIX_BIG_CAP else CHUNK
        S = -(-(int(self.a * 3 / 2) + 128) // 64) * 64
        G = min(16, int(Fraction(9, 10) * chunk / self.a))
        return (S, G, chunk) if S <= 4096 and G >= 2 else None

    def flush(self, pb, capacity):
        """pb: pairs per setup block of the flush (empty: no triangles); capacity: of the pair buffers when it begins.
        Returns the INFO words it must show."""
        if not len(pb):
            return dict(seg_S=0, seg_G=0, direct=0, fell_back=0)
        sz = self.sizes(capacity)
        out = dict(seg_S=0, seg_G=0, direct=0, fell_back=0)
        if sz is not None:
            S, G, chunk = sz
            fits = max(pb) <= S and max(group_sums(pb, G)) <= chunk
            out.update(seg_S=S, seg_G=G, direct=int(not self.hold), fell_back=int(not self.hold and not fits))
            self.hold = not fits
        self.a = max(Fraction(int(sum(pb)), len(pb)), Fraction(1))
        return out


def model_blocks(m):
    return [int(v) for v in np.add.reduceat(m.cnt, np.arange(0, m.N, BLOCK))] if m.N else []


def auto_flush(ctx, rule, case, capacity, what, interleave=None, counts=None):
    """one flush under the automatic choice (case None: a flush that only clears); its pairs per setup block against the model's
    (and `counts`, the intended ones), then INFO against the rule's prediction, the frame against the oracle.  Returns the snapshot."""
    ctx.reset_stats()
    if case is None:
        ctx.clear()
        ctx.flush()
        s = ctx.debug_snapshot()
        assert s["info"]["N"] == 0
        want = rule.flush([], capacity)
    else:
        ctx.clear(case["clear"], case["zclear"])
        m = bm.model(case, interleave=interleave)
        s = flush(ctx, case, m=m, interleave=interleave, what=what)
        assert list(per_block(s)) == model_blocks(m) and counts in (None, model_blocks(m)), (what, per_block(s), counts)
        want = rule.flush(model_blocks(m), capacity)
        if m.owned_rows.any():              # (a context without rows has no pixels to compare)
            check_frame(s, case, interleave=interleave, what=what)
    got = {k: s["info"][k] for k in want}
    assert got == want, f"{what}: INFO {got}, the rule gives {want}"
    assert ctx.debug_binning() == dict(direct=bool(want["direct"]), fell_back=bool(want["fell_back"])), what
    return s


def auto_sequence(W, H, per_block_counts, what, seed=1100):
    """a fresh context under the automatic choice; flush k holds blocks of per_block_counts[k] pairs (None: only a clear).
    Returns the INFO dicts."""
    rule, capacity, infos = Rule(), 0, []
    with Context(W, H, 3) as ctx:
        assert ctx.debug_binning(BIN_AUTO) == dict(direct=False, fell_back=False)
        for k, counts in enumerate(per_block_counts):
            case = None if counts is None else blocks_case(W, H, counts, seed + 10 * k)
            s = auto_flush(ctx, rule, case, capacity, f"{what}: flush {k} {counts}", counts=counts)
            capacity = s["info"]["capacity"]
            assert capacity < RADIX_BIG_CAP
            infos.append(s["info"])
    return infos


def path(infos):
    return [(i["seg_S"], i["seg_G"], i["direct"], i["fell_back"]) for i in infos]


def test_automatic_sizes_track_the_previous_flush():
    """pairs per block of about 300, 300, 900, 900, 120, 120: every flush is sized by the one before.  The first 900 is offered
    S = 640 and falls back, the second is checked against S = 1536 on k_expand's chain and fits, the flush after it is direct."""
    seq = [[300, 310, 290], [310, 290, 300], [900, 880, 920], [920, 900, 880], [120, 100, 140], [100, 140, 120]]
    infos = auto_sequence(128, 128, seq, "tracking")
    assert path(infos) == [(896, 7, 1, 0), (640, 12, 1, 0), (640, 12, 1, 1), (1536, 4, 0, 0), (1536, 4, 1, 0), (320, 16, 1, 0)], path(infos)


def test_automatic_hold_lasts_until_a_flush_fits():
    """after the fallback (900 into S = 640) a flush of 1600 per block does not fit the S = 1536 it is checked against: the
    context stays on k_expand's chain; the next one fits (S = 2560, G = 2) but still runs there; the one after it is direct"""
    seq = [[300, 300, 300], [900, 900, 900], [1600, 1600, 1600], [1600, 1600, 1600], [1600, 1600, 1600]]
    infos = auto_sequence(128, 128, seq, "hold")
    assert path(infos) == [(896, 7, 1, 0), (640, 12, 1, 1), (1536, 4, 0, 0), (2560, 2, 0, 0), (2560, 2, 1, 0)], path(infos)


def test_automatic_no_sizes_for_large_blocks_at_4_waves():
    """2000 pairs per block: the first flush (S = 896) falls back; a = 2000 gives G = floor(3686.4 / 2000) = 1 at a chunk of
    4096, so the following flushes are given no sizes, take k_expand's chain from the start, and are no fallback"""
    infos = auto_sequence(128, 128, [[2000, 2000]] * 3, "a beyond the limits")
    assert path(infos) == [(896, 7, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)], path(infos)


def test_automatic_rank_that_owns_nothing():
    """rank 3 of 4 with bands of one tile row on a frame of two: no pairs in any flush; after the first one a = 1 (S = 192,
    G = 16), and every flush is direct with P = 0"""
    W = H = 64
    rule, capacity, infos = Rule(), 0, []
    with Context(W, H, 3) as ctx:
        ctx.debug_binning(BIN_AUTO)
        for k in range(3):
            case = blocks_case(W, H, [300, 200], 1150 + k)
            s = auto_flush(ctx, rule, case, capacity, f"rank without rows, flush {k}", interleave=(32, 3, 4))
            assert s["info"]["P"] == 0 and s["info"]["N"] == 2 * BLOCK and not s["model"].owned_rows.any()
            capacity = s["info"]["capacity"]
            infos.append(s["info"])
    assert path(infos) == [(896, 7, 1, 0), (192, 16, 1, 0), (192, 16, 1, 0)], path(infos)


def test_automatic_sizes_after_a_flush_that_only_clears():
    """Two equal frames of 460 pairs per block with a clear-only flush between them: a flush without triangles has no setup
    blocks and no pairs per block, so the second frame is given the sizes it would have had without it (S = 832, G = 8)."""
    seq = [[460, 470, 450], [450, 460, 470], None, [470, 450, 460]]
    infos = auto_sequence(128, 128, seq, "clear-only flush")
    assert path(infos) == [(896, 7, 1, 0), (832, 8, 1, 0), (0, 0, 0, 0), (832, 8, 1, 0)], path(infos)
