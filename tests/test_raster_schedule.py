"""No GPU: (1) raster_schedule.replay on hand-made lists reports each event it claims to; (2) every scene of raster_schedule,
binned by binning_model, reaches the edges of k_raster's list loop it was built for (raster_schedule.assert_reach - the GPU
tests make the same assertions on the device's own lists); (3) what the model cannot know about a scene - that a "front"
triangle wins all 64 pixels of its block, that equal depths keep the first, that CHECKER lets a farther fragment through -
is shown on the CPU oracle."""
import numpy as np
import pytest

import binning_model as BM
import cases
import raster_schedule as RS
import test_raster_paths as RP
from oracle import orc
from tinyrenderder_amd.api import FLAT, CHECKER

UNIT = cases.UNIT_VIEWPORT
ALL = np.full(4096, 0xFFFF, np.uint16)


def flat_case(s, clip=None, col=None, bpp=3):
    return RP._kind_case(FLAT, s.clip if clip is None else clip, s.col if col is None else col, s.W, s.H, bpp, seed=9000, viewport=UNIT)


def model_lists(s, strip=None, clip=None):
    return RS.lists_from_model(BM.model(flat_case(s, clip=clip), strip=strip))


# ---- 1. the model on hand-made lists -----------------------------------------------------------------------------------------
def test_one_short_list_between_two_others():
    w = RS.replay(5, 9, ALL[:12], 3)
    (st,) = w.steps
    assert st["p0"] == 4 and st["last"] and st["before"] == 1 and st["before_bit"] == 1
    assert st["after"] == 251 and w.tail_bit == 3 and st["tail_bit"] == 3
    assert st["added"] == 4 and st["positions"] == [0, 1, 2, 3] and (st["cnt_before"], st["cnt_after"]) == (0, 4)
    assert [(r["n"], r["members"], r["on_last"], r["tested_in_step"]) for r in w.rounds] == [(4, [5, 6, 7, 8], True, 0)]
    assert w.iters == [dict(step=0, last=True, waiting=4, tested=0, started=4), dict(step=0, last=True, waiting=0, tested=4, started=0)]
    assert RS.edges(w) >= {"bit_before_beg", "bit_after_end"}


def test_lanes_past_the_end_hold_the_last_group():
    """the load address is clamped to the list's last group of four: lanes 2..63 of a six-entry list all hold words 4..7"""
    w = RS.replay(0, 6, ALL[:8], 0)
    assert w.steps[0]["after"] == 250 and w.steps[0]["after_bit"] == 2 + 62 * 4 and w.tail_bit == 2 and w.total == 6


def test_words_behind_the_buffer_count_as_set():
    assert RS.replay(0, 6, ALL[:6], 0).tail_bit == 2
    assert RS.replay(0, 6, ALL[:6], 0, beyond=0).tail_bit == 0
    assert RS.replay(0, 8, ALL[:8], 0).tail_bit == 0 and "bit_after_end" not in RS.edges(RS.replay(0, 8, ALL[:8], 0))


def test_only_the_blocks_bit_counts_and_order_is_kept():
    m = np.zeros(40, np.uint16)
    m[[3, 4, 9, 17, 18, 19, 30]] = 1 << 6
    m[[5, 6]] = 1 << 7
    w = RS.replay(4, 31, m, 6)
    assert w.total == 6 and w.rounds[0]["members"] == [4, 9, 17, 18, 19, 30] and w.steps[0]["before_bit"] == 0
    assert RS.replay(4, 31, m, 7).rounds[0]["members"] == [5, 6]
    w = RS.replay(4, 31, m, 2)
    assert w.total == 0 and w.rounds == [] and w.iters == []


@pytest.mark.parametrize("n, rounds", [(1, [1]), (63, [63]), (64, [64]), (65, [64, 1]), (127, [64, 63]), (128, [64, 64]), (129, [64, 64, 1])])
def test_rounds_of_a_single_step(n, rounds):
    w = RS.replay(0, n, ALL, 0)
    assert [r["n"] for r in w.rounds] == rounds and w.total == n
    e = RS.edges(w)
    assert f"total_{n}" in e
    assert ("start_64_on_last_step" in e) == (n % 64 == 0)           # (of 128, the second round starts with exactly 64 waiting)
    assert ("final_round_1" in e) == (rounds[-1] == 1) and ("final_round_63" in e) == (rounds[-1] == 63)


def test_span_residues():
    for beg, end, r in ((0, 256, 0), (2, 257, 1), (3, 255, 255), (4, 516, 0)):
        assert f"span_mod256_{r}" in RS.edges(RS.replay(beg, end, ALL, 0))
    assert len(RS.replay(4, 516, ALL, 0).steps) == 2 and len(RS.replay(4, 517, ALL, 0).steps) == 3


def _in_flight_list(idle_steps, tail):
    """70 candidates in step 0, none in the next idle_steps steps, `tail` in the last"""
    m = np.zeros(256 * (idle_steps + 2), np.uint16)
    m[:70] = 1
    if tail:
        m[-tail:] = 1
    return m


@pytest.mark.parametrize("idle", [1, 2])
def test_a_request_in_flight_over_idle_steps(idle):
    m = _in_flight_list(idle, 5)
    w = RS.replay(0, len(m), m, 0)
    assert [s["left_in_flight"] for s in w.steps] == [True] * (idle + 1) + [False]
    assert [s["in_flight_in"] for s in w.steps] == [0] + [64] * (idle + 1)
    assert [(r["n"], r["started_in_step"], r["tested_in_step"], r["idle_steps"]) for r in w.rounds] == [(64, 0, idle + 1, idle), (11, idle + 1, idle + 1, 0)]
    e = RS.edges(w)
    assert (f"in_flight_over_{idle}_idle_step" + ("s" if idle == 2 else "")) in e and "last_step_adds_nothing_in_flight" not in e
    # a block without any candidate walks the same steps and does nothing
    z = RS.replay(0, len(m), m, 1)
    assert len(z.steps) == idle + 2 and z.iters == [] and "no_candidate_3_steps" in RS.edges(z)


def test_a_last_step_that_adds_nothing_under_a_request():
    m = _in_flight_list(0, 0)
    w = RS.replay(0, len(m), m, 0)
    assert "last_step_adds_nothing_in_flight" in RS.edges(w)
    assert [(i["step"], i["tested"], i["started"]) for i in w.iters] == [(0, 0, 64), (1, 64, 6), (1, 6, 0)]


def test_the_ring_wraps_and_keeps_list_order():
    w = RS.replay(1, 1105, ALL, 9)
    assert w.total == 1104 and w.max_occupancy == 319 and w.max_position == 1103
    assert [(s["cnt_before"], s["added"], s["cnt_after"]) for s in w.steps[:3]] == [(0, 255, 255), (63, 256, 319), (63, 256, 319)]
    assert [s["straddle"] for s in w.steps] == [False, False, True, False, True]       # 511 .. 514 in lane 0 of step 2, 1023 .. 1026 of step 4
    assert w.steps[2]["positions"][:4] == [511, 512, 513, 514] and w.steps[2]["ring_positions"][:4] == [511, 0, 1, 2]
    assert [q for r in w.rounds for q in r["members"]] == list(range(1, 1105))
    assert {"ring_wraps_twice", "lane_straddles_wrap", "occupancy_319", "left_in_flight"} <= RS.edges(w)
    # an aligned list never has a lane across the wrap
    assert not any(s["straddle"] for s in RS.replay(0, 1104, ALL, 9).steps)


def _assert_rounds_follow_from_the_counts(w):
    got = [(r["n"], r["started_in_step"], r["tested_in_step"], r["idle_steps"]) for r in w.rounds]
    assert got == RS.round_schedule([s["added"] for s in w.steps]), (w.beg, w.end, w.kblk)


def test_rounds_agree_with_queue_arithmetic():
    """replay()'s loop against round_schedule(), which derives sizes, start and test steps and idle steps from the cumulative
    counts alone: on random lists of every density, and on every wave of every scene"""
    rng = RS.scenes.SplitMix64(77)
    for k in range(60):
        n = 1 + int(rng.uniform(1)[0] * 1500)
        density = (0.02, 0.1, 0.26, 0.5, 1.0)[k % 5]
        u = rng.uniform(n + 8)
        m = (u < density).astype(np.uint16)
        m[(n // 3):(n // 3) + 400 * (k % 3)] = 0                  # a stretch without candidates: requests stay in flight
        beg = k % 7
        _assert_rounds_follow_from_the_counts(RS.replay(beg, min(beg + n, len(m)), m, 0))
    for name in [f"steps_{a}" for a in range(4)] + sorted(RS.SCENES):
        for w in RS.waves(model_lists(RS.scene(name))).values():
            _assert_rounds_follow_from_the_counts(w)


# ---- 2. the scenes reach their edges on binning_model's lists -------------------------------------------------------------------
def test_steps_scenes_reach_every_length_at_every_alignment():
    seen, spans = set(), set()
    for a in range(4):
        s = RS.scene(f"steps_{a}")
        assert len(s.clip) < 8000
        L = model_lists(s)
        got = RS.assert_reach(s, L)
        seen |= set(RS.step_alignments(L).items())
        spans |= {e for e in got if e.startswith("span_mod256_")}
        print(s.name, got)
    assert seen == {(n, b) for n in RS.STEP_LENGTHS for b in range(4)}
    assert spans == {"span_mod256_0", "span_mod256_1", "span_mod256_255"}


def test_stale_words_draw_leaves_more_pairs_than_a_steps_scene():
    clip, col = RS.stale_words_draw(256, 64)
    m = BM.model(cases.make_case(256, 64, [(FLAT, None, clip, None, col)], viewport=UNIT))
    L = RS.lists_from_model(m)
    assert len(L.bmask) == 16 * len(clip) > len(RS.scene("steps_3").clip) + 4 and (L.bmask == 0xFFFF).all()


@pytest.mark.parametrize("name", sorted(RS.SCENES))
def test_scene_reaches_its_edges(name):
    s = RS.scene(name)
    assert len(s.clip) < 4000 and s.W <= 256 and s.H <= 64
    m = BM.model(flat_case(s))
    assert m.has_pairs.all() and m.well_scaled.all() and not m.large.any()
    print(name, RS.assert_reach(s, RS.lists_from_model(m)))


def test_ring_scene_in_a_strip_keeps_its_lists():
    s = RS.scene("ring")
    whole, part = model_lists(s), model_lists(s, strip=RS.RING_STRIP)
    assert (whole.tri == part.tri).all() and (whole.tile_start == part.tile_start).all()
    RS.assert_reach(s, part)
    assert all(k // 4 in (1, 2, 3) for _, k in RS.waves(part))           # block row 0 lies outside the strip


def test_sliver_is_literal_and_leaves_the_lists_alone():
    for name in RS.SCENES:
        s = RS.scene(name)
        clip, col = RS.with_sliver(s)
        assert RP.setup_literal(clip, UNIT, s.W, s.H)[0].tolist() == [False] * len(s.clip) + [True]
        m = BM.model(flat_case(s, clip, col))
        assert m.literal[-1] and m.has_pairs[-1]
        RS.assert_reach(s, RS.lists_from_model(m))


def test_large_triangle_makes_the_flush_compare_depth_bounds():
    for name in ("ring", "rounds"):
        s = RS.scene(name)
        clip, col = RS.with_large_triangle(s)
        m = BM.model(flat_case(s, clip, col))
        assert m.large.tolist() == [True] + [False] * len(s.clip) and (clip[0, 2] > s.z).all()


# ---- 3. what the scenes claim about depth, on the oracle ---------------------------------------------------------------------------
def _block(s, tile, block=RS.MAIN):
    X0, Y0 = s._origin(tile, block)
    return slice(Y0, Y0 + 8), slice(X0, X0 + 8)


def test_survivor_fronts_win_their_whole_block():
    """every "front" is strictly in front of everything submitted before it in its tile, and drawn in order it writes all 64 pixels
    of its block (53 where the z-buffer started with NaN): 64 fragments per front, which the GPU's count has to match"""
    s = RS.scene("survivors")
    for start, lost in ((None, 0), (RS.survivors_nan_zbuffer(s), 11)):
        o = orc.Oracle(s.W, s.H, 3, viewport=UNIT)
        if start is not None:
            o.z[:] = start
        for i in range(len(s.clip)):
            before = o.stats[1]
            o.draw(orc.FLAT, s.clip[i:i + 1], colors=s.col[i:i + 1])
            if s.role[i] == "front":
                t = int(s.tile[i])
                assert (s.z[i] < s.z[:i][s.tile[:i] == t]).all()
                ys, xs = _block(s, t)
                want = 64 - (lost if t == RS.NAN_TILE else 0)
                assert (np.abs(o.z[ys, xs] - s.z[i]) < 1e-12).sum() == want and o.stats[1] - before >= want, (i, t)


def test_notes_scene_depth_cases():
    s = RS.scene("notes")
    fb, z, st = cases.run_oracle(flat_case(s))
    stack = lambda t: np.flatnonzero((s.tile == t) & (s.role == "stack"))
    bgr = lambda c: [c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF]
    for t, winner in ((1, -1), (2, 0), (3, 0)):                    # falling depth: the last wins; equal and rising: the first
        ys, xs = _block(s, t)
        i = stack(t)[winner]
        assert (np.abs(z[ys, xs] - s.z[i]) < 1e-12).all() and (fb[ys, xs] == bgr(int(s.col[i]))).all(), t
    ys, xs = _block(s, 0)
    assert np.isfinite(z[ys, xs]).all()                              # (a): 64 disjoint triangles, one pixel each
    ys, xs = _block(s, 0, 7)
    assert len(np.unique(z[ys, xs][np.isfinite(z[ys, xs])])) >= 5   # (e): several of the overlapping ones own pixels
    # CHECKER on the rising stack: nearer triangles discard fragments, farther later ones pass there
    ck = RP._kind_case(CHECKER, s.clip, s.col, s.W, s.H, 3, seed=9000, viewport=UNIT)
    zc = cases.run_oracle(ck)[1]
    ys, xs = _block(s, 3)
    first, second = s.z[stack(3)[:2]]
    assert (np.abs(zc[ys, xs] - first) < 1e-12).any() and (np.abs(zc[ys, xs] - second) < 1e-12).any()
