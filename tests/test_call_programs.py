"""The programs of tests/call_programs.py, on the model alone (no GPU): that the committed seed list contains the hazards the GPU test
is meant for, that the final frame of a program depends on them, that the immediate interpreter agrees with the harness the goldens pin
(cases.run_oracle), and that a printed program parses back.

A hazard is a point of a program where one host rule of csrc/trgl_api.cpp (end_pending_raster, flush_queued, flush_sync, the copy of
host arrays, the kind cut) is what keeps a deferred implementation equal to the immediate reference.  Sensitivity: the model runs once
more with one operation where an implementation without that rule would apply it - a state change at the next flush point (state
latched at the flush) or right behind the previous one (queued draws rendered under the new state), a scribble before its draw - and
the final frame must differ, or the occurrence would pin nothing.

Families T, P and I (translucent kinds, passes over the resident frame, instances and clipping) add the rules of csrc/trgl_passes.cpp and
the stage entry points (csrc/trgl_stage_*.cpp).  Their sensitivity removes a rule in one of five ways: a call is moved in front of the draws it must wait for, or
behind the next flush point; a scribble or an overwrite is applied before the call; an order list is reversed; queued draws read the
arrays of a later draw (the staging arena reset under them).  Where none of the five fits, the rule's own opposite is run: the draws
queued in front of a refused call do not land, a register is read as it was before the pass that fills it, visibility bytes that draw
nothing or a plane that drops everything are ignored, a query reads the resident depths in place of a freed snapshot's.  Only the
quiet calls inside a begun flush have no observable opposite and are held by their occurrences alone."""
import collections

import numpy as np
import pytest

import blend_model as B
import call_programs as cp
import cases
import instance_model as IM
import instanced_cases as IC
import occlusion_model
import shadow_model
from oracle import orc
from tinyrenderder_amd import scenes

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
        if f == "T":
            assert set(cp.BLEND) <= set(kinds) and "draw_instanced" not in names
        if f in "TPI":                                  # (whole frames, but for the strip a refused pass of family P stands in)
            assert all(p.ops[k + 2][0] == "refused" and p.ops[k + 3][0] == "set_interleave" for k, n in enumerate(names) if n == "set_strip")
            assert f == "P" or "set_strip" not in names
            assert len(set(cp.KINDS[a["src"]][1] for n, a in p.ops if n == "register_shader" and a["src"] in cp.KINDS) |
                       set(a["src"] for n, a in p.ops if n == "register_shader" and a["src"] not in cp.KINDS) |
                       set(a["src"] for n, a in p.ops if n == "register_vertex_shader")) <= 3, "at most three user sources"
        for n, a in p.ops:
            if n in ("draw_instanced", "instance_stage"):
                assert a["n"] <= (cp.INST_BLOCK + 40 if a["mesh"] == "quad" and a["vis"] != "none" else 40)
                visited = a["n"] + 3 if a["ord"] != "none" else (a["n"] + 1) // 2 if a["n"] > 40 else a["n"]      # (the large calls draw every other instance)
                assert visited * (12 if a["mesh"] == "cube" else 2) <= 300, (f, s, a)
                if a["n"] > 40:
                    vis = next(b for m, c in p.ops for b in cp.arrays_of(m, c) if b["reg"] == a["vis"])
                    assert vis["pattern"] == "alternating"
    for name in ("draw", "draw_indexed", "draw_burst", "set_viewport", "init_viewport", "upload_texture", "clear", "write_framebuffer",
                 "write_zbuffer", "reset_stats", "flush", "flush_begin", "flush_end", "sync", "zbuffer_snapshot", "zbuffer_restore",
                 "framebuffer_blur", "postprocess", "mesh_bounds", "register_shader", "set_stream", "refused", "set_strip", "set_interleave",
                 "read_fb", "read_z", "stats", "observe",
                 "array", "instances", "read_reg", "occlusion_boxes", "shadow_mask", "framebuffer_modulate", "image_blur", "zbuffer_snapshot_free",
                 "instance_boxes", "frustum_boxes", "instance_depths", "depth_order", "draw_instanced", "instance_stage", "clip_stage",
                 "dev_copy", "register_vertex_shader"):
        assert seen[name] >= 3, name
    new = [(n, a, program(f, s)) for f, s in ALL for n, a in program(f, s).ops]
    mem_of = {(id(q), b["reg"]): b["mem"] for n, a, q in new for b in cp.arrays_of(n, a)}
    for n, a, q in new:                                 # (registers that calls wrote are where their inputs were)
        if n in ("instance_boxes", "instance_depths"):
            mem_of[id(q), a["out"]] = mem_of[id(q), a["inst"]]
        elif n == "depth_order":
            mem_of[id(q), a["out"]] = mem_of[id(q), a["depths"]]
        elif n == "frustum_boxes":
            mem_of[id(q), a["codes"]] = mem_of[id(q), a["boxes"]]
        elif n == "occlusion_boxes":
            mem_of[id(q), a["out"]] = a["cmem"]
        elif n == "shadow_mask":
            mem_of[id(q), a["out"]] = a["mem"]
    m = lambda q, reg: "none" if reg == "none" else mem_of[id(q), reg]
    calls = {call: {(a["mmem"], m(q, a["inst"]), m(q, a["vis"]), m(q, a["ord"])) for n, a, q in new if n == call} for call in ("draw_instanced", "instance_stage")}
    for call, combos in calls.items():                  # each call sees each of its arrays in both memories and every vertex stage
        for k, kinds in enumerate((("host", "dev"), ("host", "dev"), ("host", "dev", "none"), ("host", "dev", "none"))):
            assert {c[k] for c in combos} == set(kinds), (call, k, combos)
        assert {a["vs"] for n, a, q in new if n == call} == set(cp.VERTEX_STAGES), call
    # every combination include/trgl.h allows an instanced call (visibility bytes are where the instances are) occurs
    allowed = {(t[0], t[1], t[1] if t[2] else "none", t[3] or "none") for t in cp.MEMORY_COMBOS}
    both = calls["draw_instanced"] | calls["instance_stage"]
    assert len(allowed) == 24 and both == allowed, sorted(allowed - both)
    scribbled = {(a["mmem"], m(q, a["vis"])) for n, a, q in new if n == "draw_instanced" and a["scr"] and m(q, a["inst"]) == "host"}
    assert ("host", "host") in scribbled and ("dev", "host") in scribbled, scribbled     # the host mesh is scribbled next to host bytes too
    assert {(m(q, a["boxes"]), a["cmem"]) for n, a, q in new if n == "occlusion_boxes"} == {(x, y) for x in ("host", "dev") for y in ("host", "dev")}
    assert {a["slot"] >= 0 for n, a, q in new if n == "occlusion_boxes"} == {True, False}
    assert {a["mem"] for n, a, q in new if n == "shadow_mask"} == {"host", "dev"}
    assert {(m(q, a["mask"]), a["scr"]) for n, a, q in new if n == "framebuffer_modulate"} >= {("host", 1), ("dev", 0), ("none", 1)}
    assert {(a["merge"], m(q, a["boxes"])) for n, a, q in new if n == "frustum_boxes"} >= {(0, "dev"), (1, "dev"), (0, "host")}
    assert {(a["dir"], m(q, a["depths"])) for n, a, q in new if n == "depth_order"} == {(x, y) for x in (0, 1) for y in ("host", "dev")}
    assert {m(q, a["inst"]) for n, a, q in new if n == "instance_boxes"} == {m(q, a["inst"]) for n, a, q in new if n == "instance_depths"} == {"host", "dev"}
    assert {a["mem"] for n, a, q in new if n == "clip_stage"} == {"host", "dev"}
    assert {(n, a["mem"]) for n, a, q in new if n in ("draw", "draw_indexed") and a.get("plane")} >= {("draw", "dev"), ("draw_indexed", "host")}
    family_t = [program("T", s) for s in cp.SEEDS["T"]]
    assert {p.bpp for p in family_t} == {1, 3, 4} and {(p.w, p.h) for p in family_t} == set(cp.FRAMES)
    family_a = [program("A", s) for s in cp.SEEDS["A"]]
    assert {p.bpp for p in family_a} == {1, 3, 4} and {(p.w, p.h) for p in family_a} == set(cp.FRAMES)
    blur_radii = {a["r"] for f, s in ALL for n, a in program(f, s).ops if n == "framebuffer_blur"}
    assert min(blur_radii) == 1 and max(blur_radii) == cp.BLUR_LDS_RADIUS + 1 and cp.BLUR_LDS_RADIUS in blur_radii, blur_radii
    refused = {a["what"] for f, s in ALL for n, a in program(f, s).ops if n == "refused"}
    assert refused == {"unknown_kind", "bad_strip", "blur_in_strip", "restore_empty", "occl_empty_slot", "shadow_empty_slot", "occl_in_strip",
                       "shadow_in_strip", "inst_bad_order", "inst_k_differs"}
    kinds = {a["kind"] for f, s in ALL for n, a in program(f, s).ops if n == "draw"}
    assert kinds == set(cp.KINDS)
    mems = {(n, a["mem"]) for f, s in ALL for n, a in program(f, s).ops if n in ("draw", "draw_indexed")}
    assert len(mems) == 4


HAZARDS = ["vp_diff_queued", "vp_same_queued", "init_vp_queued", "tex_replace_queued", "tex_replace_sampled", "clear_queued",
           "clear_only_flush", "write_over_clear", "write_queued", "reset_stats_queued"] + ["mid_" + m for m in cp.MID_OPS] + \
          ["scribble_draw", "scribble_indexed", "phong_flat_phong", "kind_cut", "snapshot_queued", "restore_queued", "blur_queued",
           "postprocess_queued", "refused_queued", "strip_queued", "zero_draw"]
HAZARDS_T = ["blend_kind_cut", "blend_same_kind_twice", "blend_over_clear", "blend_over_written", "blend_over_pass", "nodepth_then_opaque",
             "blend_begun", "blend_restore"] + ["blend_mid_" + m for m in cp.MID_OPS]
HAZARDS_P = ["occl_queued", "shadow_queued", "modulate_queued", "occl_clear_pending", "occl_snapshot_stale", "shadow_chain", "modulate_scribbled",
             "pass_then_stream", "pass_refused_queued", "snapshot_free_queued"]
HAZARDS_I = ["chain_device", "inst_host_scribbled", "inst_dev_overwritten", "inst_two_calls", "inst_begun", "inst_zero", "clip_drops_all_queued",
             "clip_drops_all_idle", "clip_wait_queued", "quiet_begun", "inst_refused_queued"]


def test_hazards():
    """Each hazard occurs at least 3 times over the seed list, each time with a queued (or begun) draw that put fragments into the
    model's frame; the draws of one flush pass TRGL_MAX_DRAWS at least once."""
    count = collections.Counter()
    for f, s in ALL:
        count.update(name for name, _ in truth(f, s)[1])
    short = {h: count[h] for h in HAZARDS + HAZARDS_T + HAZARDS_P + HAZARDS_I if count[h] < 3}
    assert not short, (short, dict(count))
    assert count["max_draws"] >= 1, dict(count)
    for family, names in (("T", HAZARDS_T), ("P", HAZARDS_P), ("I", HAZARDS_I)):       # each family holds its own hazards three times
        own = collections.Counter(name for s in cp.SEEDS[family] for name, _ in truth(family, s)[1])
        assert not {h: own[h] for h in names if own[h] < 3}, (family, dict(own))


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


# ---- families T, P and I ---------------------------------------------------------------------------------------------------------
_SETUP = ("register_shader", "register_vertex_shader")
_DRAWS = ("draw", "draw_indexed", "draw_burst", "draw_instanced")


def _before_the_draws(p, i):
    """The index of the first of the draws (and flush_begin) that stand directly in front of operation i."""
    k = i
    while k > 0 and p.ops[k - 1][0] in _DRAWS + _SETUP + ("flush_begin",):
        k -= 1
    return k


def _previous(p, i):
    """The operation in front of i that is not a registration."""
    k = i - 1
    while p.ops[k][0] in _SETUP:
        k -= 1
    return k


def _tagged(obs, tag):
    return [o[3] for o in obs if o[0] == tag]


def _arrays_differ(a, b, distinct=1):
    """Whether two lists of arrays differ in an array that holds at least `distinct` values in the second, the true one."""
    return len(a) != len(b) or any(not np.array_equal(x, y) and len(set(y.reshape(-1).tolist())) >= distinct for x, y in zip(a, b))


def _frames_differ(got, want):
    """Whether two runs of the model that make the same observations in the same order differ in one of the frame, its bytes, depths
    or counters (the operation numbers may differ: an operation was moved)."""
    kinds = ("fb", "z", "stats", "frame", "post")
    got, want = [o for o in got if o[0] in kinds], [o for o in want if o[0] in kinds]
    assert [o[0] for o in got] == [o[0] for o in want]
    return any(cp.differs(g[:1] + w[1:2] + g[2:], w) for g, w in zip(got, want))


def _removed(p, name, i):
    """(the model's run of program p with the rule of hazard `name` at operation i removed, what to compare) or None when the five
    removals do not apply to this hazard."""
    a = p.ops[i][1]
    if name == "inst_begun":                            # (likewise: the draws of the begun flush move behind the call)
        j = _before_the_draws(p, i)
        q = p
        for _ in range(j, max(k for k in range(i) if p.ops[k][0] == "flush_begin")):
            q = q.moved(j, i + 1)
        return cp.run_model(q), "frame"
    if name in ("occl_queued", "shadow_queued", "modulate_queued", "clip_wait_queued"):
        return cp.run_model(p.moved(i, _before_the_draws(p, i))), {"occl_queued": "codes", "shadow_queued": "mask"}.get(name, "frame")
    if name == "occl_clear_pending":                    # in front of the clear it must wait for
        j = max(k for k in range(i) if p.ops[k][0] == "clear")
        return cp.run_model(p.moved(i, j)), "codes"
    if name in ("blend_kind_cut", "blend_same_kind_twice", "blend_over_clear", "blend_over_written", "blend_over_pass", "blend_begun",
                "nodepth_then_opaque", "inst_two_calls"):   # in front of what it must be drawn over
        if p.ops[i][0] == "draw_instanced":             # (its registers are written in between: what it is drawn over moves behind it)
            j = max(k for k in range(i) if p.ops[k][0] in _DRAWS)
            return cp.run_model(p.moved(j, i + 1)), "frame"
        j = _previous(p, i)
        if p.ops[j][0] == "flush_begin":
            j = _before_the_draws(p, j)
        return cp.run_model(p.moved(i, j)), "frame"
    if name == "blend_restore":                         # the restore in front of the translucent layers
        j = max(k for k in range(i) if p.ops[k][0] == "zbuffer_snapshot" and p.ops[k][1]["slot"] == a["slot"])
        return cp.run_model(p.moved(i, j + 1)), "frame"
    if name == "shadow_chain":                          # behind the next flush point: the draws on top are darkened too
        j = next(k for k in range(i + 1, len(p.ops)) if p.ops[k][0] in cp.FLUSH_POINTS)
        return cp.run_model(p.moved(i, j + 1 if p.ops[j][0] in ("flush", "flush_end") else j)), "frame"
    if name in ("modulate_scribbled", "inst_host_scribbled"):
        return cp.run_model(p, lazy_scribble=i), "frame"
    if name == "chain_device":
        return cp.run_model(p, reverse_order=i), "frame"
    if name == "inst_dev_overwritten":                  # the overwrite in front of the call that named the register
        reg = a["codes"] if "codes" in a else a["reg"] if "reg" in a else a["out"]
        j = max(k for k in range(i) if p.ops[k][0] == "draw_instanced" and reg in p.ops[k][1].values())
        return cp.run_model(p.moved(i, j)), "frame"
    if name == "clip_drops_all_queued":                 # the arena reset with draws queued: the staged draw reads the next draw's arrays
        k = max(k for k in range(i) if p.ops[k][0] == "draw" and p.ops[k][1]["mem"] == "host")
        j = next(j for j in range(i + 1, len(p.ops)) if p.ops[j][0] == "draw")
        return cp.run_model(p, swap_arrays={k: j}), "frame"
    if name in ("pass_refused_queued", "inst_refused_queued"):      # the queued draws do not land: the program without them
        gone = [k for k in range(_before_the_draws(p, i), i) if p.ops[k][0] in _DRAWS]
        return cp.run_model(cp.Program(p.family, p.seed, p.w, p.h, p.bpp, [op for k, op in enumerate(p.ops) if k not in gone])), "frame"
    if name == "pass_then_stream":                      # the pass behind its consumer: the register as it was before the pass
        return cp.run_model(p, alter={i: "stale"}), "codes" if p.ops[i][0] == "read_reg" else "frame"
    if name == "inst_zero":                             # the bytes that draw nothing are not looked at
        return cp.run_model(p, alter={i: "all_visible"}), "frame"
    if name == "clip_drops_all_idle":                   # the plane that drops everything is not applied
        return cp.run_model(p, alter={i: "no_plane"}), "frame"
    if name == "snapshot_free_queued":                  # the free in front of the query: the slot's depths are gone, it reads the resident ones
        return cp.run_model(p, alter={i - 1: "resident"}), "codes"
    return None


# trgl_instance_boxes, trgl_frustum_boxes, trgl_instance_depths and trgl_depth_order inside a begun flush: whether they complete it or
# not, every observation of the model is the same (the second half of a flush runs before anything reads the frame either way), so no
# removal of the rule gives another result; the hazard is held by its occurrences, each with fragments in the begun flush
NOT_REMOVABLE = {"quiet_begun"}


def test_sensitivity_of_the_new_families():
    sensitive = collections.defaultdict(set)
    for f in "TPI":
        for s in cp.SEEDS[f]:
            p = program(f, s)
            obs, events = truth(f, s)
            for name, i in events:
                if name not in HAZARDS_T + HAZARDS_P + HAZARDS_I or name.startswith("blend_mid_") or name in NOT_REMOVABLE or (f, s) in sensitive[name]:
                    continue
                if name == "occl_snapshot_stale":       # the hazard is the difference of the two arrays itself
                    mine = [o[3] for o in obs if o[0] == "codes" and o[1] in (i - 1, i)]
                    if all(len(set(c.tolist())) >= 2 for c in mine):
                        sensitive[name].add((f, s))
                    continue
                got, what = _removed(p, name, i)
                if what == "frame":                     # (any observation of the frame, not the last alone: a later clear hides nothing)
                    hit = _frames_differ(got, obs)
                else:
                    hit = _arrays_differ(_tagged(got, what), _tagged(obs, what), distinct=2 if what == "codes" else 1)
                if hit:
                    sensitive[name].add((f, s))
    names = [h for h in HAZARDS_T + HAZARDS_P + HAZARDS_I if not h.startswith("blend_mid_") and h not in NOT_REMOVABLE]
    short = {h: sorted(sensitive[h]) for h in names if len(sensitive[h]) < 3}
    assert not short, short


def test_reversed_chain_differs():
    """The device chain of family I ends in an ordered translucent draw: visited backwards, the frame read behind it is another one."""
    found = 0
    for s in cp.SEEDS["I"]:
        obs, events = truth("I", s)
        for name, i in events:
            if name == "chain_device":
                found += _frames_differ(cp.run_model(program("I", s), reverse_order=i), obs)     # (the chain ends in a read_fb)
    assert found >= 3, found


def test_translucent_model_equals_blend_model():
    """A T program of clear, draws, observe equals blend_model.model_frame: the per-triangle scheme on the program's oracle is the
    scheme of blend_model.Model, counters and depth range included."""
    for name, kind in (("96x64_bpp1", "TOVER"), ("96x64_bpp3", "TOVER_ND"), ("96x64_bpp4", "TADD"), ("101x67_viewport_zclear", "TOVER")):
        cfg, clip, col = B.frame(name)
        f = B.FRAMES[name]
        p = cp.Program("T", 0, cfg["w"], cfg["h"], cfg["bpp"], [
            ("set_viewport", dict(rect=(f.get("vx", 0), f.get("vy", 0), f.get("vw", f["w"]), f.get("vh", f["h"])))),
            ("clear", dict(bgra=tuple(cfg["clear"]), z=cfg["zclear"])), ("observe", {})])
        # (the draw's arrays are blend_model's own scene, handed to the interpreter's draw in place of a seeded one)
        real = cp.draw_arrays
        try:
            cp.draw_arrays = lambda prog, a: (clip, None, col, None)
            p.ops.insert(2, ("draw", dict(kind=kind, n=len(col), seed=0, r=1, mem="host", scr=0)))
            (obs,) = cp.run_model(p)
        finally:
            cp.draw_arrays = real
        fn, depth_write = cp.BLEND[kind]
        want = B.model_frame(name, fn, depth_write)
        assert want[2][1] > 500
        cases.assert_same_frame(obs[3:6], want[:3])
        assert obs[6] == want[3]


def _plain(family, ops, w=96, h=64, bpp=3):
    return cp.Program(family, 0, w, h, bpp, ops)


def test_instanced_model_equals_the_harness():
    """An I program equals cases.run_oracle on the expanded loop: vertex stage per drawn instance, then a draw of its rows."""
    p = _plain("I", [("array", dict(reg="i0", what="inst", mem="host", n=9, seed=5, stride=19)),
                     ("array", dict(reg="v1", what="vis", mem="host", n=9, seed=6, pattern="alternating")),
                     ("array", dict(reg="o2", what="order", mem="host", n=9, seed=7)),
                     ("draw_instanced", dict(kind="PHONG", vs="builtin", mesh="cube", mmem="host", n=9, inst="i0", icol="none", fcol=0, vis="v1",
                                             ord="o2", scr=0)),
                     ("draw_instanced", dict(kind="FLAT", vs="k0", mesh="quad", mmem="host", n=9, inst="i0", icol="none", fcol=1, vis="none",
                                             ord="none", scr=0)),
                     ("observe", {})])
    (obs,) = cp.run_model(p)
    cam = cp.camera(p)
    mv, proj, key, u = cam.model_view, cam.projection, cam.key, cp.call_uniforms(p, {})
    inst, vis, order = (cp.array_of(p, a) for n, a in p.ops[:3])
    draws = []
    verts, idx, _ = cp.mesh_of("cube")
    for j in order:                                     # the loop include/trgl.h defines, one instance at a time
        if vis[j] & 1:
            clip, vary = orc.vertex_stage(IM.mat_product(mv, inst[j, :16]), proj, verts, idx)
            draws.append((cp.PHONG, u, clip, vary, None))
    verts, idx, fc = cp.mesh_of("quad")
    for j in range(9):
        clip, _ = IC.expect_user("k0", mv, proj, key, verts, idx, inst, np.array([j]))
        draws.append((cp.FLAT, None, clip, None, fc))
    fb, z, stats = cases.run_oracle(cases.make_case(p.w, p.h, draws, bpp=p.bpp))
    assert stats[1] > 300, stats
    cases.assert_same_frame(obs[3:6], (fb, z, stats))


def test_pass_models_equal_the_models_on_the_harness_depths():
    """A P program's codes and mask equal occlusion_model and shadow_model applied to cases.run_oracle's depths."""
    clear = dict(bgra=(10, 20, 30, 255), z=0.6)
    d1, d2 = dict(kind="FLAT", n=10, seed=11, r=2, mem="host", scr=0), dict(kind="GOURAUD", n=10, seed=12, r=2, mem="host", scr=0)
    p = _plain("P", [("array", dict(reg="b0", what="boxes", mem="host", n=30, seed=3)), ("clear", clear), ("draw", d1), ("zbuffer_snapshot", dict(slot=1)),
                     ("clear", clear), ("draw", d2), ("occlusion_boxes", dict(slot=-1, boxes="b0", out="c1", cmem="host", vp="ndc")),
                     ("occlusion_boxes", dict(slot=1, boxes="b0", out="c2", cmem="host", vp="ndc")),
                     ("shadow_mask", dict(slot=1, out="m3", mem="host", dx=2, dy=-1, r=1)), ("observe", {})])
    obs = cp.run_model(p)
    z = []
    for d in (d1, d2):
        q = _plain("P", [("clear", clear), ("draw", d), ("observe", {})])
        z.append(cases.run_oracle(cp.simple_case(q))[1])
    boxes, vp = cp.array_of(p, p.ops[0][1]), scenes.init_viewport(0, 0, p.w, p.h)
    assert np.array_equal(obs[0][3], occlusion_model.codes(z[1], vp, np.eye(4), boxes)) and len(set(obs[0][3].tolist())) >= 2
    assert np.array_equal(obs[1][3], occlusion_model.codes(z[0], vp, np.eye(4), boxes)) and not np.array_equal(obs[0][3], obs[1][3])
    m, r = cp.shadow_params_of(p.ops[8][1])
    want = shadow_model.shadow_mask(z[1], m, z[0], cp.SHADOW_BIAS, cp.SHADOW_DARKNESS, r)
    assert np.array_equal(obs[2][3], want) and (want < 255).any() and (want == 255).any()
