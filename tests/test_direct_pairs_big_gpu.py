"""The direct path of the binning where the product runs it: pair buffers of at least 4 M entries (RADIX_BIG_CAP), so that the
radix passes run in blocks of 8 waves over chunks of 8192 pairs - k_radix_scatter<8, false, LAST, true> with wave_part computed
from 512 threads and groups checked against 8192 - and the automatic sizes are derived from that chunk.

tests/test_direct_pairs_gpu.py covers the same path in 4-wave blocks; its helpers are used here.  Two module-scoped contexts
(256^2: 64 tiles, one radix pass; 544^2: 289 tiles, two) get their pair buffers from one flush of 2.1 M rejected triangles each,
as test_pair_lists_in_eight_wave_radix_blocks does.  Every test sets the binning mode itself, resets the stats and clears, so
none depends on another; every flush is exact against binning_model and the CPU oracle, and the forced-direct arrays equal
those of the forced k_expand chain.  Per-block pair counts are stated, built from whole-tile rectangles and asserted from the
snapshot before the path taken is.
"""
from fractions import Fraction

import numpy as np
import pytest

from test_direct_pairs_gpu import Rule, auto_flush, blocks_case, both_ways, group_sums, one, path, per_block, same_lists_and_frame
from test_stage_outputs_gpu import RADIX_BIG_CAP, _flat
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import BIN_AUTO, BIN_EXPAND, FLAT, Context

pytestmark = pytest.mark.gpu

BIG_CHUNK = 8192          # pairs per block of a radix pass over pair buffers of at least RADIX_BIG_CAP entries
SIZING_ROWS = 2_100_000   # rejected triangles (w = 0) of the flush that sizes the pair buffers at 2 pairs per triangle


def _big_context(W, H):
    ctx = Context(W, H, 3)
    ctx.draw(FLAT, np.zeros((SIZING_ROWS, 12)))
    ctx.flush()
    info = ctx.debug_snapshot()["info"]
    assert info["P"] == 0 and info["capacity"] >= RADIX_BIG_CAP, info
    return ctx


@pytest.fixture(scope="module")
def big():
    ctx = _big_context(256, 256)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def big544():
    ctx = _big_context(544, 544)
    yield ctx
    ctx.close()


def big_both_ways(ctx, case, S, G, fell_back, counts, what):
    d = both_ways(case, S, G, fell_back, what=what, ctx=ctx, counts=counts)
    assert d["info"]["capacity"] >= 4 << 20, d["info"]
    return d


# ---- a full group, one pair more ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuller", [None, 0, 7, 15])
def test_group_at_the_eight_wave_chunk_and_one_above(big, fuller):
    """G = 16: 16 blocks of 512 pairs (256 triangles of 2 tiles) are 8192, the chunk of an 8-wave block, every wave's part full
    (wave_part = 1024); one pair more in the block of the first, a middle or the last wave's part (S = 516 holds it) makes 8193,
    which no block of the first pass may hold"""
    counts = [512] * 16
    if fuller is not None:
        counts[fuller] += 1
    S = 512 if fuller is None else 516
    assert max(counts) <= S and group_sums(counts, 16) == [BIG_CHUNK + (fuller is not None)]
    big_both_ways(big, blocks_case(256, 256, counts, 2001, big=2), S, 16, fuller is not None, counts, f"group of 8192, one more in block {fuller}")


@pytest.mark.parametrize("extra,fell_back", [(0, False), (1, True)])
def test_two_segments_of_seg_max(big, extra, fell_back):
    """G = 2, S = 4096 (SEG_MAX): two blocks of exactly 4096 pairs (256 triangles of 16 tiles) fill k_setup's staging buffer to
    its last word and the 8-wave chunk; 4097 in one block is more than any segment holds"""
    counts = [4096, 4096 + extra]
    assert (max(counts) <= 4096) == (not fell_back)
    big_both_ways(big, blocks_case(256, 256, counts, 2011), 4096, 2, fell_back, counts, f"two blocks of 4096 + {extra}")


# ---- pairs per group ----------------------------------------------------------------------------------------------------
def spread(c, n, rng, most=4096):
    """c pairs over n segments, unevenly, about half of the segments empty"""
    out = np.zeros(n, np.int64)
    live = rng.choice(n, size=max(1, min(n // 2, c)), replace=False)
    for k in rng.choice(live, size=min(c, 64)):
        out[k] += 1
    rest = c - int(out.sum())
    for k in live:                                          # the rest to the first live segments that still have room
        put = min(rest, most - out[k])
        out[k] += put
        rest -= put
    assert rest == 0 and out.sum() == c and out.max() <= most
    return [int(v) for v in out]


@pytest.mark.parametrize("groups", [(1, 63, 64), (65, 511, 512), (513, 1024, 8191), (8191, 1, 65)])
def test_pairs_per_group_and_wave_parts(big, groups):
    """G = 16, two full groups and a third of 5 segments in one flush, with c pairs each: wave_part = ceil(c / 512) * 64 takes
    its first value (c <= 512: one round per wave, waves behind ceil(c / 64) idle), interior ones and its last (8191: 1024, the
    last wave one pair short); the pairs sit unevenly in the segments, about half of which are empty"""
    rng = np.random.default_rng(2021 + groups[0])
    counts = spread(groups[0], 16, rng) + spread(groups[1], 16, rng) + spread(groups[2], 5, rng)
    S = (max(counts) + 3) & ~3
    assert group_sums(counts, 16) == list(groups) and max(groups) <= BIG_CHUNK and 0 in counts[:16] and 0 in counts[16:32]
    big_both_ways(big, blocks_case(256, 256, counts, 2031, last=77), S, 16, False, counts, f"groups of {groups}")


# ---- two radix passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,fell_back", [(2048, False), (64, True)])
def test_two_radix_passes_in_eight_wave_blocks(big544, S, fell_back):
    """289 tiles: the first pass reads the segments and is not the last; when the flush does not fit, the dense last pass queued
    behind it must leave the tile bounds alone as well (test_direct_two_radix_passes, in 8-wave blocks)"""
    clip, col = scenes.random_triangles(1500, 544, 544, seed=2041, rmin=2, rmax=30)
    d = big_both_ways(big544, _flat(544, 544, clip, col), S, 3, fell_back, None, "two passes, 8 waves")
    assert d["info"]["tiles_x"] * d["info"]["tiles_y"] > 256 and (per_block(d).max() <= S) == (not fell_back)
    assert max(group_sums(per_block(d), 3)) <= BIG_CHUNK


# ---- the automatic choice -----------------------------------------------------------------------------------------------
def rule_after_an_empty_flush(ctx):
    """the automatic choice on the shared context, its input set by a flush of 300 rejected triangles: a = 1 (0 pairs per block)"""
    ctx.debug_binning(BIN_AUTO)
    ctx.reset_stats()
    ctx.clear()
    ctx.draw(FLAT, np.zeros((300, 12)))
    ctx.flush()
    info = ctx.debug_snapshot()["info"]
    assert info["N"] == 300 and info["P"] == 0 and info["capacity"] >= 4 << 20
    rule = Rule()
    rule.a = Fraction(1)
    return rule, info["capacity"]


@pytest.mark.parametrize("fullest,fell_back", [(192, False), (193, True)])
def test_automatic_sizes_in_eight_wave_blocks(big, fullest, fell_back):
    """after a flush without pairs the rule gives S = 192, G = 16: 40 blocks of at most 192 pairs run direct, one block of 193
    falls back"""
    counts = [int(v) for v in np.random.default_rng(2051).integers(0, 193, 40)]
    counts[3], counts[17], counts[38] = 0, fullest, 192
    rule, capacity = rule_after_an_empty_flush(big)
    case = blocks_case(256, 256, counts, 2052, big=4)
    assert max(counts) == fullest and max(group_sums(counts, 16)) <= BIG_CHUNK
    s = auto_flush(big, rule, case, capacity, f"fullest block {fullest}", counts=counts)
    assert path([s["info"]]) == [(192, 16, 1, int(fell_back))], s["info"]
    assert s["info"]["capacity"] >= 4 << 20
    e = one(case, BIN_EXPAND, ctx=big, what="k_expand")
    same_lists_and_frame(s, e, f"fullest block {fullest}")


def test_automatic_sizes_come_from_the_chunk_in_use(big):
    """2000 pairs per block, as test_automatic_no_sizes_for_large_blocks_at_4_waves: the first flush (offered S = 192) falls
    back; with a chunk of 8192 a = 2000 gives G = floor(7372.8 / 2000) = 3, so the next flush is checked against S = 3136,
    G = 3 on k_expand's chain, fits, and the third runs direct"""
    rule, capacity = rule_after_an_empty_flush(big)
    infos = []
    for k in range(3):
        case = blocks_case(256, 256, [2000, 2000], 2061 + k)
        s = auto_flush(big, rule, case, capacity, f"a = 2000, flush {k}", counts=[2000, 2000])
        capacity = s["info"]["capacity"]
        assert capacity >= 4 << 20
        infos.append(s["info"])
    assert path(infos) == [(192, 16, 1, 1), (3136, 3, 0, 0), (3136, 3, 1, 0)], path(infos)
    e = one(case, BIN_EXPAND, ctx=big, what="k_expand")
    same_lists_and_frame(s, e, "a = 2000, third flush")


# ---- the same edge in 4-wave blocks --------------------------------------------------------------------------------------
def test_one_segment_of_seg_max_in_four_wave_blocks():
    """on a fresh small context: G = 1, S = 4096, one block of 4096 pairs - the segment and the 4-wave chunk both full"""
    d = both_ways(blocks_case(128, 128, [4096], 2071), 4096, 1, False, what="one block of 4096, 4 waves", counts=[4096])
    assert d["info"]["capacity"] < RADIX_BIG_CAP
