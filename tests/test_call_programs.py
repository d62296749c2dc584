"""The programs of tests/call_programs.py, on the model alone (no GPU): that the committed seed list contains the hazards the GPU test
is meant for, that the final frame of a program depends on them, that the immediate interpreter agrees with the harness the goldens pin
(cases.run_oracle), and that a printed program parses back.

A hazard is a point of a program where one host rule of csrc/trgl_api.cpp (end_pending_raster, flush_queued, flush_sync, the copy of
host arrays, the kind cut) is what keeps a deferred implementation equal to the immediate reference.  Sensitivity: the model runs once
more with one operation where an implementation without that rule would apply it - a state change at the next flush point (state
latched at the flush) or right behind the previous one (queued draws rendered under the new state), a scribble before its draw - and
the final frame must differ, or the occurrence would pin nothing."""
import collections

import pytest

import call_programs as cp
import cases
from oracle import orc

ALL = [(f, s) for f in cp.FAMILIES for s in cp.SEEDS[f]]
_programs, _truth = {}, {}


def program(f, s):
    if (f, s) not in _programs:
        _programs[f, s] = cp.generate(f, s)
    return _programs[f, s]


def truth(f, s):
    """(observations, hazards) of the model's run of a program, computed once."""
    if (f, s) not in _truth:
        sh = cp._Shadow()
        _truth[f, s] = (cp.run_model(program(f, s), shadow=sh), sh.events)
    return _truth[f, s]


def test_printing():
    for f, s in ALL:
        p = program(f, s)
        text = p.text()
        assert cp.Program.parse(text) == p, text
        assert cp.Program.parse(text).text() == text
        assert len(text.splitlines()) == len(p.ops) + 1 and p.text(3).splitlines() == text.splitlines()[:4]
    assert cp.generate("B", 3) == program("B", 3) and cp.generate("B", 3) != program("B", 4)


def test_program_shape():
    seen = collections.Counter()
    for f, s in ALL:
        p = program(f, s)
        names = [n for n, _ in p.ops]
        assert 25 <= len(names) <= 60, (f, s, len(names))
        assert names[-1] == "observe" and p.w <= 160 and p.h <= 128
        seen.update(names)
        kinds = [a["kind"] for n, a in p.ops if n in ("draw", "draw_indexed", "draw_burst")]
        for n, a in p.ops:
            if n in ("draw", "draw_burst"):
                assert 0 <= a.get("n", 1) <= 300
                assert not (a.get("mem") == "dev" and a.get("scr")), "device arrays are never scribbled"
        if f == "A":
            assert "upload_texture" not in names and "EYE" not in kinds
        if f == "S":
            assert names[:2] == ["write_framebuffer", "write_zbuffer"] and "clear" not in names and "framebuffer_blur" not in names
        if f == "E":
            assert "EYE" in kinds and "framebuffer_blur" not in names and not any(a["final"] for n, a in p.ops if n == "postprocess")
        if f != "E":
            assert "EYE" not in kinds
        if f == "D":
            assert "UCHECKER" in kinds
    for name in ("draw", "draw_indexed", "draw_burst", "set_viewport", "init_viewport", "upload_texture", "clear", "write_framebuffer",
                 "write_zbuffer", "reset_stats", "flush", "flush_begin", "flush_end", "sync", "zbuffer_snapshot", "zbuffer_restore",
                 "framebuffer_blur", "postprocess", "mesh_bounds", "register_shader", "set_stream", "refused", "set_strip", "set_interleave",
                 "read_fb", "read_z", "stats", "observe"):
        assert seen[name] >= 3, name
    family_a = [program("A", s) for s in cp.SEEDS["A"]]
    assert {p.bpp for p in family_a} == {1, 3, 4} and {(p.w, p.h) for p in family_a} == set(cp.FRAMES)
    blur_radii = {a["r"] for f, s in ALL for n, a in program(f, s).ops if n == "framebuffer_blur"}
    assert min(blur_radii) == 1 and max(blur_radii) == cp.BLUR_LDS_RADIUS + 1 and cp.BLUR_LDS_RADIUS in blur_radii, blur_radii
    refused = {a["what"] for f, s in ALL for n, a in program(f, s).ops if n == "refused"}
    assert refused == {"unknown_kind", "bad_strip", "blur_in_strip", "restore_empty"}
    kinds = {a["kind"] for f, s in ALL for n, a in program(f, s).ops if n == "draw"}
    assert kinds == set(cp.KINDS)
    mems = {(n, a["mem"]) for f, s in ALL for n, a in program(f, s).ops if n in ("draw", "draw_indexed")}
    assert len(mems) == 4


HAZARDS = ["vp_diff_queued", "vp_same_queued", "init_vp_queued", "tex_replace_queued", "tex_replace_sampled", "clear_queued",
           "clear_only_flush", "write_over_clear", "write_queued", "reset_stats_queued"] + ["mid_" + m for m in cp.MID_OPS] + \
          ["scribble_draw", "scribble_indexed", "phong_flat_phong", "kind_cut", "snapshot_queued", "restore_queued", "blur_queued",
           "postprocess_queued", "refused_queued", "strip_queued", "zero_draw"]


def test_hazards():
    """Each hazard occurs at least 3 times over the seed list, each time with a queued (or begun) draw that put fragments into the
    model's frame; the draws of one flush pass TRGL_MAX_DRAWS at least once."""
    count = collections.Counter()
    for f, s in ALL:
        count.update(name for name, _ in truth(f, s)[1])
    short = {h: count[h] for h in HAZARDS if count[h] < 3}
    assert not short, (short, dict(count))
    assert count["max_draws"] >= 1, dict(count)


def _final(obs):
    return [o for o in obs if o[0] == "frame"][-1]


def _occurrences(p):
    """(hazard class, operation index) of every state change and scribble of a program."""
    rect, loaded = (0, 0, p.w, p.h), set()
    for i, (n, a) in enumerate(p.ops):
        if n in ("set_viewport", "init_viewport"):
            if tuple(a["rect"]) != rect:
                yield "viewport", i
            rect = tuple(a["rect"])
        elif n == "upload_texture":
            if a["slot"] in loaded:
                yield "texture", i
            loaded.add(a["slot"])
        elif n in ("set_strip", "set_interleave"):
            yield "strip", i
        elif n == "reset_stats":
            yield "reset_stats", i
        elif n in ("draw", "draw_indexed") and a.get("scr"):
            yield "scribble", i


def _has_draw(ops):
    return any(n in ("draw", "draw_indexed", "draw_burst") for n, _ in ops)


def test_sensitivity():
    late, early = collections.defaultdict(set), collections.defaultdict(set)
    for f, s in ALL:
        p = program(f, s)
        want = _final(truth(f, s)[0])
        for what, i in _occurrences(p):
            if what == "scribble":
                if cp.differs(_final(cp.run_model(p, lazy_scribble=i)), want):
                    late[what].add((f, s))
                continue
            j = next(k for k in range(i + 1, len(p.ops)) if p.ops[k][0] in cp.FLUSH_POINTS)      # (the last operation is one)
            if (f, s) not in late[what] and _has_draw(p.ops[i + 1:j]) and cp.differs(_final(cp.run_model(p.moved(i, j))), want):
                late[what].add((f, s))
            j = max([k + 1 for k in range(i) if p.ops[k][0] in cp.FLUSH_POINTS], default=0)
            if (f, s) not in early[what] and _has_draw(p.ops[j:i]) and cp.differs(_final(cp.run_model(p.moved(i, j))), want):
                early[what].add((f, s))
    for what in ("viewport", "texture", "strip", "reset_stats", "scribble"):
        assert len(late[what]) >= 3, (what, sorted(late[what]))
    for what in ("viewport", "texture", "strip", "reset_stats"):
        assert len(early[what]) >= 3, (what, sorted(early[what]))


@pytest.mark.parametrize("family,bpp", [("A", 1), ("B", 3), ("E", 4), ("S", 3)])
def test_model_equals_the_harness(family, bpp):
    """run_model on a program that is only state, draws and one observation equals cases.run_oracle on the same case."""
    g = cp._Gen(family, 2)
    g.bpp = bpp
    g.set_viewport()
    if family in "BE":
        for slot, b in enumerate((3, 3, 1, 1, 4, 4)):
            g.upload(slot, b)
    g.clear()
    for kind in g.kinds:
        if cp.KINDS[kind][1] is None:
            g.draw(kind=kind, mem="host", scr=0)
            g.draw(kind=kind, mem="host", scr=0, r=2)
    g.op("observe")
    p = cp.Program(family, 2, g.w, g.h, g.bpp, g.ops)
    (obs,) = cp.run_model(p)
    fb, z, stats = cases.run_oracle(cp.simple_case(p))
    assert stats[1] > 500, stats
    cases.assert_same_frame(obs[3:6], (fb, z, stats))
    assert obs[6] == orc.format_stats_line(stats)


def test_moved():
    p = program("A", 0)
    names = [n for n, _ in p.ops]
    q = p.moved(2, 5)
    assert [n for n, _ in q.ops] == names[:2] + names[3:5] + [names[2]] + names[5:]
    q = p.moved(5, 2)
    assert [n for n, _ in q.ops] == names[:2] + [names[5]] + names[2:5] + names[6:]
