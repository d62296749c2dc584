"""The programs of tests/shim_programs.py on the model alone (no GPU): that the committed list contains every hazard the GPU test
(tests/test_shim_programs_gpu.py) is meant for, and that the observations of a program depend on it.

A hazard is a place in a program where one rule of tinyrenderder_amd/shim/trgl_gl.h - a cut of rasterize()'s batch, the proxy completing
pending work, bind() and the context, a call that submits the batch first - is what keeps the deferred shim equal to the immediate
reference.  For each one the model runs once more as a deferred implementation WITHOUT that rule at that place (run_model's lazy=...),
and its observations must differ from the model's own; otherwise a shim without the rule would pass the GPU test and the occurrence
would pin nothing.  Taking a hazard's operations out of the committed programs fails its test here: no occurrence is left.

 1 uniform change inside one kind (PHONG's ModelView and normal_map_strength, CHECKER's cells)      late_state
 2 Viewport change inside one kind                                                                late_state
 3 kind change, into and out of CHECKER and a user kind that may discard                          by_kind
 4 element read between runs                                                                      read_before, read_dirty
 5 element write between runs                                                                     write_before
 6 saved = zbuffer ... zbuffer = saved with runs of one kind on both sides                        save_before
 7 init_zbuffer in mid-frame                                                                      init_before
 8 texture upload between two PHONG runs on one slot                                              upload_before
 9 clip plane switched on and off between runs of one kind                                        late_plane
10 gl_draw_indexed between two rasterize runs of one kind and uniforms                            indexed_first
11 the cut at TRGL_SHIM_BATCH_TRIS, three coincident triangles across it                          tail_first
12 print_render_stats() in mid-sequence                                                           stats_before
13 a framebuffer of another size after gl_flush(old): a user kind keeps its number                user_lost
14 a framebuffer of another size with work pending                                                into_bound
15 a second image of the same size: gl_flush(A), gl_framebuffer_modified(B), draws into B         no_modified"""
import collections

import numpy as np
import pytest

import call_programs as cp
import cases
import shim_programs as sp

_truth = {}


def truth(name):
    if name not in _truth:
        _truth[name] = sp.run_model(sp.PROGRAMS[name])
    return _truth[name]


def where(hazard, pick=lambda p, i: True):
    """[(program name, operation index)] of a hazard over the committed programs."""
    return [(name, i) for name, p in sp.PROGRAMS.items() for h, i in sp.occurrences(p) if h == hazard and pick(p, i)]


def lazy_differs(name, rule, i):
    return sp.differs(sp.run_model(sp.PROGRAMS[name], lazy=(rule, i)), truth(name))


def assert_each_noticed(found, rule, at_least=1, everywhere=False):
    """Every occurrence in `found` changes the observations of its program when `rule` is missing there (everywhere: in the whole program)."""
    assert len(found) >= at_least, (rule, found)
    blind = [(name, i) for name, i in found if not lazy_differs(name, rule, None if everywhere else i)]
    assert not blind, (rule, blind)


def test_printing_and_shape():
    assert len(sp.PROGRAMS) <= 24
    registering = 0
    for name, p in sp.PROGRAMS.items():
        text = p.text()
        assert cp.Program.parse(text) == p and cp.Program.parse(text).text() == text, name
        assert sp.encode(p) == sp.encode(cp.Program.parse(text)), name
        names = [n for n, _ in p.ops]
        assert names[0] == "image" and names[-1] == "flush", name
        registering += "register_shader" in names
        dims = {a["fb"]: (a["w"], a["h"], a["bpp"]) for n, a in p.ops if n == "image"}
        assert set(dims.values()) <= {sp.MAIN, sp.SMALL1, sp.SMALL4}, name
        for n, a in p.ops:
            if n == "rasterize":
                assert 20 <= a["n"] <= 300 and a["kind"] != "EYE", (name, a)
    assert registering <= 2
    used = collections.Counter(n for p in sp.PROGRAMS.values() for n, _ in p.ops)
    assert set(used) == set(sp.OPCODES) - {"end"}, set(sp.OPCODES) - set(used)
    kinds = {a["kind"] for p in sp.PROGRAMS.values() for n, a in p.ops if n == "rasterize"}
    assert kinds == {"FLAT", "GOURAUD", "CHECKER", "PHONG", "UCHECKER"}
    first = {(p.w, p.h, p.bpp) for p in sp.PROGRAMS.values()}
    assert first == {sp.MAIN, sp.SMALL1, sp.SMALL4}
    assert set(sp.B64) <= set(sp.PROGRAMS)


def test_every_draw_lands():
    """Each run of each program puts fragments into the model's frame (the counters grow), and no program ends in an error."""
    for name, p in sp.PROGRAMS.items():
        m = sp._Model(p, None)
        for i, (n, a) in enumerate(p.ops):
            before = m.o.stats[1] if m.o is not None and n == "rasterize" and (m.o.w, m.o.h, m.o.bpp) == m.dims[a["fb"]] else 0
            m.step(i, n, a)
            if n == "rasterize":
                assert (m.o.stats[1] > before) != bool(a.get("hidden")), (name, i, a)
        assert truth(name)[-1] == ("error", len(p.ops), 0, "")


@pytest.mark.parametrize("dims", [sp.MAIN, sp.SMALL1, sp.SMALL4])
def test_model_equals_the_harness(dims):
    """A program that is only runs and one gl_flush equals cases.run_oracle on the same draws."""
    w, h, bpp = dims
    runs = [dict(fb=0, kind=k, n=25, seed=900 + j, r=2, **({"cells": 5} if k == "CHECKER" else {})) for j, k in enumerate(("FLAT", "GOURAUD", "CHECKER", "FLAT"))]
    ops = [("image", dict(fb=0, w=w, h=h, bpp=bpp, fill=cases.DEFAULT_CLEAR)), ("init_zbuffer", dict(w=w, h=h)), ("init_viewport", dict(rect=(3, 2, w - 5, h - 3)))]
    ops += [("rasterize", a) for a in runs] + [("stats", {}), ("flush", dict(fb=0)), ("z_ref", {})]
    obs = sp.run_model(cp.Program("plain", 0, w, h, bpp, ops))
    q = cp.Program("A", 0, w, h, bpp, [("set_viewport", dict(rect=(3, 2, w - 5, h - 3)))] + [("draw", a) for a in runs] + [("observe", {})])
    fb, z, stats = cases.run_oracle(cp.simple_case(q))
    assert stats[1] > 300, stats
    from oracle import orc
    assert obs[0] == ("stats", len(ops) - 3, orc.format_stats_line(stats))
    assert obs[1][:4] == ("image", len(ops) - 2, 1, 0) and np.array_equal(obs[1][4], fb)
    assert np.array_equal(obs[2][2].view(np.uint64), z.reshape(-1).view(np.uint64))


def test_the_driver_format_names_every_operation():
    """The opcodes of shim_programs.py are the enum of tests/host/shim_program.cpp, in order; the record tags likewise."""
    import os
    import re
    src = open(os.path.join(cp.ROOT, "tests", "host", "shim_program.cpp")).read()
    ops = re.search(r"enum Op \{(.*?)\};", src, re.S).group(1)
    names = [n.split("=")[0].strip().lower() for n in ops.replace("\n", " ").split(",")]
    assert names == sorted(sp.OPCODES, key=sp.OPCODES.get), names
    tags = re.search(r"enum Tag \{(.*?)\};", src, re.S).group(1)
    assert [t.split("=")[0].strip()[2:].lower() for t in tags.split(",")] == [sp.TAGS[k] for k in sorted(sp.TAGS)]
    assert f"-DTRGL_SHIM_BATCH_TRIS={sp.BATCH} " in open(os.path.join(cp.ROOT, "examples", "Makefile")).read()


# ---- one test per hazard ---------------------------------------------------------------------------------------------------------------
def _run(p, i):
    return p.ops[i][1]


def _previous_run(p, i):
    return next(p.ops[k][1] for k in range(i - 1, -1, -1) if p.ops[k][0] == "rasterize")


def test_hazard_01_uniform_change():
    between = lambda p, i: [n for n, _ in p.ops[max(k for k in range(i) if p.ops[k][0] == "rasterize"):i]]
    model_view = where(1, lambda p, i: _run(p, i)["kind"] == "PHONG" and "modelview" in between(p, i) and _run(p, i)["s"] == _previous_run(p, i)["s"])
    strength = where(1, lambda p, i: _run(p, i)["kind"] == "PHONG" and "modelview" not in between(p, i) and _run(p, i)["s"] != _previous_run(p, i)["s"])
    cells = where(1, lambda p, i: _run(p, i)["kind"] == "CHECKER" and _run(p, i)["cells"] != _previous_run(p, i)["cells"])
    for found in (model_view, strength, cells):
        assert_each_noticed(found, "late_state")


def test_hazard_02_viewport_change():
    assert_each_noticed(where(2), "late_state", at_least=3)


def test_hazard_03_kind_change():
    found = where(3)
    pairs = {(_previous_run(sp.PROGRAMS[name], i)["kind"], _run(sp.PROGRAMS[name], i)["kind"]) for name, i in found}
    for discarding in sp.DISCARDING:
        assert {a for a, b in pairs if b == discarding} - set(sp.DISCARDING), (discarding, pairs)      # into it, from a kind that cannot discard
        assert {b for a, b in pairs if a == discarding} - set(sp.DISCARDING), (discarding, pairs)      # and out of it
    assert ("CHECKER", "UCHECKER") in pairs and ("UCHECKER", "CHECKER") in pairs
    # (grouping by kind needs a kind that comes back: the programs made of kind changes alone)
    assert_each_noticed([(name, None) for name in ("kinds", "kinds_small")], "by_kind", everywhere=True)
    assert {name for name, _ in found} >= {"kinds", "kinds_small"}


def test_hazard_04_element_read():
    reads = where(4, lambda p, i: p.ops[i][0] == "z_read")
    # (a read of a pixel the pending run leaves alone sees the same either way: two that see another depth)
    assert sum(lazy_differs(name, "read_before", i) for name, i in reads) >= 2, reads
    # a read that marks the host copy modified: with pull() as it is, the copy it marks is the one it has just fetched, and nothing is
    # lost; it costs a frame when the copy is an older one - here the one the last whole access fetched, which a run has changed since
    assert_each_noticed(reads, "read_dirty", at_least=2)
    assert_each_noticed(where(4, lambda p, i: p.ops[i][0] == "z_copy"), "read_before")


def test_hazard_05_element_write():
    writes = where(5, lambda p, i: p.ops[i][0] == "z_write")
    assert len(writes) >= 4 and {sp.PROGRAMS[name].ops[i][1]["v"] for name, i in writes} == {-9.0, float("inf")}
    # (a single write may land on a pixel the next run does not cover: the writes of one place together are what a caller makes)
    for name in {name for name, _ in writes}:
        assert lazy_differs(name, "write_before", None), name
    noticed = [(name, i) for name, i in writes if lazy_differs(name, "write_before", i)]
    assert {sp.PROGRAMS[name].ops[i][1]["v"] for name, i in noticed} == {-9.0, float("inf")}, noticed
    assert_each_noticed(where(5, lambda p, i: p.ops[i][0] == "z_copy"), "write_before")


def test_hazard_06_save_and_restore():
    assert_each_noticed(where(6, lambda p, i: p.ops[i][0] == "z_save"), "save_before", at_least=2)
    assert_each_noticed(where(6, lambda p, i: p.ops[i][0] == "z_load"), "save_before", at_least=2)


def test_hazard_07_init_zbuffer_in_mid_frame():
    assert_each_noticed(where(7), "init_before")


def test_hazard_08_texture_upload():
    assert_each_noticed(where(8), "upload_before")


def test_hazard_09_clip_plane():
    found = where(9)
    planes = {sp.PROGRAMS[name].ops[i][1]["plane"] for name, i in found}
    assert "off" in planes and len(planes) >= 3, planes
    assert_each_noticed(found, "late_plane", at_least=4)


def test_hazard_10_draw_indexed():
    assert_each_noticed(where(10), "indexed_first")


def test_hazard_11_batch_bound():
    found = where(11)
    assert {name for name, _ in found} <= set(sp.B64), "the driver with the small batch bound runs them"
    assert {_run(sp.PROGRAMS[name], i)["n"] // sp.BATCH for name, i in found} >= {1, 2}      # the first cut of a run, and a later one
    assert_each_noticed(found, "tail_first", at_least=2)


def test_hazard_12_stats_in_mid_sequence():
    found = where(12)
    assert_each_noticed(found, "stats_before", at_least=3)
    # ... and changes nothing that follows: the program without the call makes the other observations unchanged
    for name, i in found[:3]:
        p = sp.PROGRAMS[name]
        q = cp.Program(p.family, p.seed, p.w, p.h, p.bpp, p.ops[:i] + p.ops[i + 1:])
        want = [o[:1] + (o[1] - (o[1] > i),) + o[2:] for o in truth(name) if o[1] != i]
        assert not sp.differs(sp.run_model(q), want), (name, i)


def test_hazard_13_user_kind_on_another_size():
    found = where(13)
    assert_each_noticed(found, "user_lost", everywhere=True)
    for name, i in found:                               # registered once, in front of the first framebuffer's draws
        p = sp.PROGRAMS[name]
        assert [n for n, _ in p.ops].count("register_shader") == 1 and any(n == "rasterize" and a["kind"] == "UCHECKER" for n, a in p.ops[:i - 1])


def test_hazard_14_another_size_with_work_pending():
    found = where(14)
    assert_each_noticed(found, "into_bound", at_least=3)
    calls = {sp.PROGRAMS[name].ops[i][0] for name, i in found}
    assert calls == {"rasterize", "flush"}, calls     # the new framebuffer first met by a draw, and by gl_flush alone
    # with Viewport changed in between and unchanged; with the kind unchanged
    def viewport_moved(p, i):
        k = max(k for k in range(i) if p.ops[k][0] == "rasterize")
        return "init_viewport" in [n for n, _ in p.ops[k:i]]
    assert {viewport_moved(sp.PROGRAMS[name], i) for name, i in found if sp.PROGRAMS[name].ops[i][0] == "rasterize"} == {True, False}
    # the old image's bytes are observed behind the switch, as its last gl_flush left them
    for name, i in found:
        p = sp.PROGRAMS[name]
        old = _previous_run(p, i)["fb"]
        assert any(n == "dump" and a["fb"] == old for n, a in p.ops[i:]) or p.ops[i][0] == "flush", (name, i)


def test_hazard_15_second_image_of_the_same_size():
    found = where(15)
    assert_each_noticed(found, "no_modified")
    for name, i in found:                               # depths persist: a read of them behind the first draws into the second image
        p = sp.PROGRAMS[name]
        assert any(n in ("z_read", "z_ref", "z_iter") for n, _ in p.ops[i:])
    # and without gl_flush(old): gl_framebuffer_modified(B) with a run pending for A
    assert any(p.ops[i][0] == "fb_modified" and p.ops[i - 1][0] == "rasterize" and p.ops[i - 1][1]["fb"] != p.ops[i][1]["fb"]
               for p in sp.PROGRAMS.values() for i in range(1, len(p.ops)))
