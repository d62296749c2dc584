"""k_raster at the edges of its own list loop (steps, candidate ring, cull rounds, survivors, deferred notes), on every kind.

Each scene of tests/raster_schedule.py is drawn through cases.run_gpu and held to the CPU oracle with cases.assert_same_frame (z bits,
framebuffer bytes, stats tuple and stats line; EYE within its usual 1 LSB on at most 0.1 % of the pixels).  Through run_gpu's
`inspect` hook the test reads Context.debug_snapshot() of that very flush and replays raster_schedule's model over the device's own
vals / bmask / tile_start / tile_end: raster_schedule.assert_reach makes there the same assertions as tests/test_raster_schedule.py
makes on binning_model's lists, and info["zq_cull"] == 0 says that candidacy depended on the masks alone, as the model assumes.
That is the proof that the edges were reached on the lists the kernel walked; nothing here uses the diagnostic build.

What the snapshot cannot show: the words behind the last tile's end lie outside the P entries it returns.  The steps scenes are
drawn behind a flush of raster_schedule.stale_words_draw on the same context (more pairs, every mask 0xFFFF), as the issue asks,
but that part of the test cannot fail: the stale words name triangles 0..499, valid in the flush that follows and nowhere near the
reading block, so a missing end mask on the last tile would change neither frame nor stats.  The same holds for every masked
neighbour (it lies in another tile): for the entries outside [beg, end) the reach assertions are the evidence, not the frame.
"""
import numpy as np
import pytest

import cases
import raster_schedule as RS
import test_raster_paths as RP
import test_user_kind_raster_paths_gpu as UK
from oracle import orc
from tinyrenderder_amd.api import FLAT, GOURAUD, PHONG, EYE, CHECKER

UNIT = cases.UNIT_VIEWPORT
same = cases.assert_same_frame

# id -> (kind, bytes per pixel, one literal triangle elsewhere in the flush)
VARIANTS = {"flat_1": (FLAT, 1, False), "flat_3": (FLAT, 3, False), "flat_4": (FLAT, 4, False), "flat_3_literal": (FLAT, 3, True),
            "gouraud": (GOURAUD, 3, False), "checker": (CHECKER, 3, False), "phong": (PHONG, 3, False), "eye": (EYE, 3, False),
            "mixed": (RP.MIXED, 3, False)}

_frames = {}


def oracle_frame(key, case, **kw):
    """cases.run_oracle plus the stats line, once per key (never written to)"""
    if key not in _frames:
        fb, z, st = cases.run_oracle(case, **kw)
        _frames[key] = (fb, z, st, orc.format_stats_line(st))
    return _frames[key]


def kind_case(s, kind, bpp, clip=None, col=None):
    return RP._kind_case(kind, s.clip if clip is None else clip, s.col if col is None else col, s.W, s.H, bpp, seed=9600, viewport=UNIT)


def draw(s, case, key, zq=0, reach=True, literal=0, eye=False, rows=None, oracle_kw=None, **run):
    """run_gpu against the oracle; zq_cull and k_setup's count of literal triangles of the flush as expected; the scene's edges
    reached on the device's lists"""
    snaps = []
    got = cases.run_gpu(case, inspect=lambda ctx: snaps.append(ctx.debug_snapshot()), **run)
    same(got, oracle_frame(key, case, **(oracle_kw or {})), rows=rows, eye=eye, what=str(key))
    assert snaps[0]["info"]["zq_cull"] == zq and snaps[0]["info"]["literal_tris"] == literal, snaps[0]["info"]
    if reach:
        RS.assert_reach(s, RS.lists_from_snapshot(snaps[0]))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(RS.SCENES))
def test_scene_on_every_kind(name, variant):
    s = RS.scene(name)
    kind, bpp, literal = VARIANTS[variant]
    clip, col = RS.with_sliver(s) if literal else (s.clip, s.col)
    got = draw(s, kind_case(s, kind, bpp, clip, col), (name, variant), literal=int(literal), eye=kind == EYE)
    assert got[2][1] > 300                                   # fragments drawn (the sparsest, rounds under CHECKER, has 313)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flat_3", "mixed"])
@pytest.mark.parametrize("a", range(4))
def test_steps_scene_behind_a_larger_flush(a, variant):
    """list lengths 255 .. 1025 at beg & 3 = a + ..., every list's neighbours carrying the bit of the wave that has candidates"""
    s = RS.scene(f"steps_{a}")
    kind, bpp, _ = VARIANTS[variant]
    case = kind_case(s, kind, bpp)
    stale, scol = RS.stale_words_draw(s.W, s.H)
    case = dict(case, draws=[(FLAT, None, stale, None, scol)] + case["draws"])
    draw(s, case, (s.name, variant), flush_after=0)


@pytest.mark.gpu
def test_ring_scene_in_a_strip_that_owns_blocks_in_part():
    s = RS.scene("ring")
    draw(s, kind_case(s, FLAT, 3), ("ring", "strip"), rows=RS.RING_STRIP, strip=RS.RING_STRIP, oracle_kw=dict(strip=RS.RING_STRIP))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring", "rounds"])
def test_scene_with_depth_bounds_in_the_pair_words(name):
    """one triangle of 64 pixels and more behind everything: the flush drops list entries by their depth bound before they become
    candidates (the model does not cover that: the frame alone is compared)"""
    s = RS.scene(name)
    clip, col = RS.with_large_triangle(s)
    draw(s, kind_case(s, FLAT, 3, clip, col), (name, "large"), zq=1, reach=False)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flat_3", "mixed"])
def test_odd_survivors_on_a_zbuffer_with_nan(variant):
    """a round with one survivor in a block whose caller-written depths hold NaN: the partner record's plane passes the first test
    of its visit on those lanes"""
    s = RS.scene("survivors")
    kind, bpp, _ = VARIANTS[variant]
    z0 = RS.survivors_nan_zbuffer(s)
    got = draw(s, kind_case(s, kind, bpp), ("survivors", variant, "nan"), start=(None, z0), oracle_kw=dict(start=(None, z0)))
    assert np.isnan(got[1]).sum() == np.isnan(z0).sum() == 11


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring", "notes"])
def test_scene_through_a_discarding_user_kind(name):
    """trgl_raster_user has a list loop of its own (64 entries per step): the same lists, frames only"""
    s = RS.scene(name)
    case, shaders = UK.DISCARDING_FLAT.case(s.clip, s.col, s.W, s.H, 3, seed=9600, viewport=UNIT)
    same(cases.run_gpu(case, shaders=shaders), oracle_frame((name, "flat_3"), case), what=name)
