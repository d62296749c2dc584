"""Programs of a main.cpp-shaped caller over the shim (tinyrenderder_amd/shim/trgl_gl.h) against an immediate-mode model.

The shim's rasterize() only batches; a batch is cut when the kind, the uniforms or Viewport change, the `zbuffer` proxy completes pending
work before every access, bind() creates and re-creates the context, and every other entry point submits the batch first.  A *program*
is a list of what a caller writes - runs of rasterize() calls, assignments to the globals, uses of zbuffer, gl_flush(), pixel writes -
in the text form of tests/call_programs.py (Program.text() / Program.parse()); tests/host/shim_program.cpp executes its binary form
(encode) through the shim's public names, run_model executes it at once on the CPU oracle, and both give the observations the program
asks for, which must be equal bit for bit.

  PROGRAMS                    the committed list: name -> Program
  run_model(program)          -> [observation]; with lazy=(rule, i) the model without one rule of the shim at operation i (None: everywhere)
  encode(program)             -> the bytes shim_program reads
  decode(program, out, err)   -> [observation] of a driver run (its output file and its stderr)
  occurrences(program)        -> [(hazard number, operation index)]: where a rule of the shim is what keeps it equal to the model

The model is the reference: one image per TGAImage, drawn into where rasterize() names it, one global depth vector, every operation
in effect where it stands.  Two rules follow the shim and are stated in INTEGRATION.md: the counters are the context's, so they restart
when a framebuffer of another size or bpp is first used; and such a framebuffer starts from the depths of `zbuffer` when it holds
width x height of them, from +inf otherwise.

An observation is (tag, operation index, payload...): 'image' (gl_flush's result, gl_last_error(), the bytes; for `dump` the TGAImage
as the caller holds it), 'depths', 'double', 'size', 'kind', 'stats' (the line on stderr), 'error' (gl_last_error() and its message)."""
import struct

import numpy as np

import call_programs as cp
import clip_model
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import GOURAUD, PHONG, SHADER_USER_FIRST

BATCH = 64                                              # TRGL_SHIM_BATCH_TRIS of the second driver binary (examples/Makefile)
MAIN, SMALL1, SMALL4 = (96, 64, 3), (37, 29, 1), (37, 29, 4)
KIND_CODES = {"FLAT": 0, "GOURAUD": 1, "PHONG": 2, "CHECKER": 4, "UCHECKER": 100}      # shim_program.cpp: enum Kind (user kinds from 100, in order)
OPCODES = {n: k for k, n in enumerate(("end", "image", "register_shader", "rasterize", "modelview", "init_viewport", "z_read", "z_write", "z_copy",
                                       "z_save", "z_load", "z_iter", "z_size", "z_ref", "init_zbuffer", "flush", "fb_set", "fb_modified",
                                       "upload_texture", "clip_plane", "draw_indexed", "stats", "dump"))}
TAGS = {1: "image", 2: "depths", 3: "double", 4: "size", 5: "kind", 6: "error"}
STATE_OPS = ("modelview", "init_viewport", "image")    # assignments to globals and constructors: no call into the shim
DISCARDING = ("CHECKER", "UCHECKER")
TEX = (0, 1, 2)


class _Dims:
    def __init__(self, w, h):
        self.w, self.h = w, h


def model_view(seed):
    """A ModelView of a `modelview` operation: a turn about the y axis and a shift, other ones for every seed."""
    c, t = np.cos(0.4 * seed), np.sin(0.4 * seed)
    return np.array([[c, 0.0, t, 0.1 * seed], [0.0, 1.0, 0.0, -0.05 * seed], [-t, 0.0, c, -2.0], [0.0, 0.0, 0.0, 1.0]], np.float64)


def run_arrays(dims, a):
    """(clip, varyings, colours, uniforms) of a rasterize run: call_programs.draw_arrays, with the three triangles from `tie` on made
    one triangle in three colours (equal depths everywhere: the first one submitted owns every pixel), and the colours changed by
    `tint` (runs that share a seed are the same triangles: where two of them keep a fragment, the first one submitted owns it)."""
    clip, vary, col, u = cp.draw_arrays(_Dims(*dims[:2]), a)
    if "tint" in a and col is not None:
        col ^= np.uint32(a["tint"] * 0x01030507 & 0x00FFFFFF)
    if "tie" in a:
        t = a["tie"]
        clip[t + 1], clip[t + 2] = clip[t], clip[t]
        if vary is not None and cp.KINDS[a["kind"]][0] == GOURAUD:
            vary[t + 1], vary[t + 2] = vary[t], vary[t]
    return clip, vary, col, u


# ---- the committed programs ----------------------------------------------------------------------------------------------------------
class _Build:
    def __init__(self, name, dims=MAIN, fill=(40, 30, 20, 255)):
        self.name, self.ops, self.dims, self.runs = name, [], {}, 0
        self.next_seed = 52000 + 700 * len(_built)
        self.image(0, dims, fill)
        self.op("init_zbuffer", w=dims[0], h=dims[1])
        self.op("init_viewport", rect=(0, 0, dims[0], dims[1]))

    def op(self, name, **a):
        self.ops.append((name, a))

    def seed(self):
        self.next_seed += 13
        return self.next_seed

    def image(self, fb, dims, fill=(40, 30, 20, 255)):
        self.dims[fb] = dims
        self.op("image", fb=fb, w=dims[0], h=dims[1], bpp=dims[2], fill=tuple(fill))

    def run(self, kind, fb=0, n=None, r=1, seed=None, **kw):
        n = n or (60 if self.dims[fb][0] > 40 else 30)
        a = dict(fb=fb, kind=kind, n=n, seed=seed or self.seed(), r=r)
        self.runs += 1
        kw.setdefault("zoff", 1 - self.runs)     # each run a little nearer than the one before: all of them stay in sight
        if kind == "PHONG":
            a.update(tex=kw.pop("tex", TEX), s=kw.pop("s", 10))
        if kind in DISCARDING:
            a.update(cells=kw.pop("cells", 4))
        a.update(kw)
        self.op("rasterize", **a)
        return a

    def textures(self, fb=0):
        for slot, bpp in zip(TEX, (3, 3, 1)):
            self.op("upload_texture", fb=fb, slot=slot, w=9 + 2 * slot, h=7, bpp=bpp, seed=self.seed())

    def viewport(self, rect):
        self.op("init_viewport", rect=tuple(rect))

    def covered(self, fb=0):
        """An index of the depth vector in the middle of the frame, where large triangles are."""
        w, h, _ = self.dims[fb]
        return (h // 2) * w + w // 2

    def changed(self, k=0):
        """An index of the depth vector where the last operation, a run, changed the model's depths: the k-th such place, counted from the
        middle one of them (found once, when the list is built: the programs are their text)."""
        m = _Model(cp.Program(self.name, 0, 0, 0, 0, self.ops), None)
        for i, (name, a) in enumerate(self.ops[:-1]):
            m.step(i, name, a)
        before = m.z.copy()
        m.step(len(self.ops) - 1, *self.ops[-1])
        places = np.flatnonzero(before.view(np.uint64) != m.z.view(np.uint64))
        return int(places[len(places) // 2 + k])

    def done(self, fb=0):
        self.op("flush", fb=fb)
        d = self.dims[0]
        p = cp.Program(self.name, len(_built), d[0], d[1], d[2], self.ops)
        _built[self.name] = p
        return p


_built = {}


def _programs():
    b = _Build("phong_uniforms")                        # hazard 1: ModelView and normal_map_strength between PHONG runs
    b.textures()
    b.op("modelview", seed=3); b.run("PHONG", r=2, n=20); b.op("modelview", seed=4); b.run("PHONG", r=2, n=20)
    b.run("PHONG", r=2, n=20, s=3); b.run("PHONG", n=40, s=3)
    b.op("stats"); b.done()

    b = _Build("checker_cells_viewport")                # hazards 1 and 2: cells between CHECKER runs, Viewport between runs of one kind
    b.run("CHECKER", r=2, n=20, cells=3); b.run("CHECKER", r=2, n=20, cells=6)
    b.viewport((8, 4, 80, 52)); b.run("CHECKER", r=2, n=20, cells=6)
    b.run("FLAT", r=2, n=20); b.viewport((-10, -6, 116, 76)); b.run("FLAT", r=2, n=20); b.viewport((0, 0, 48, 64)); b.run("FLAT", n=50)
    b.op("flush", fb=0); b.op("z_iter"); b.done()

    b = _Build("viewport_small", SMALL4)                # hazard 2 on the small frame
    b.run("GOURAUD", r=2, n=20); b.viewport((4, 2, 30, 24)); b.run("GOURAUD", r=2, n=20); b.viewport((0, 0, 37, 29)); b.run("GOURAUD")
    b.op("stats"); b.done()

    # hazard 3: kind changes into and out of the kinds that may discard.  Submission order shows only where depths tie, so the runs of a
    # group are the same triangles in other colours: a fragment belongs to the first run of its group that keeps it
    b = _Build("kinds")
    b.op("register_shader", src="UCHECKER")
    for g, group in enumerate(((("CHECKER", 4), ("UCHECKER", 3), ("CHECKER", 2), ("FLAT", 0)),
                               (("UCHECKER", 4), ("CHECKER", 3), ("UCHECKER", 5), ("GOURAUD", 0)),
                               (("CHECKER", 3), ("FLAT", 0)))):
        seed = b.seed()
        for k, (kind, cells) in enumerate(group):
            b.run(kind, r=2, n=20, seed=seed, zoff=-3 * g, tint=4 * g + k + 1, **({"cells": cells} if cells else {}))
    b.op("stats"); b.op("flush", fb=0); b.op("z_ref"); b.done()

    b = _Build("kinds_small", SMALL1)                   # hazard 3 on one byte per pixel (hidden: behind the run in front of it, all of it)
    for g, group in enumerate(((("CHECKER", 4), ("GOURAUD", 0), ("CHECKER", 3)), (("GOURAUD", 0),), (("CHECKER", 5), ("FLAT", 0), ("CHECKER", 2)))):
        seed = b.seed()
        for k, (kind, cells) in enumerate(group):
            b.run(kind, r=2, n=20, seed=seed, zoff=-3 * g, tint=4 * g + k + 1, **({"cells": cells} if cells else {}), **({"hidden": 1} if k == 2 else {}))
    b.done()

    b = _Build("z_reads")                               # hazards 4 and 5: elements read, written and copied between runs of one kind
    b.run("FLAT", r=2, n=20); b.op("z_iter"); b.run("FLAT", n=60, zoff=-4); b.op("z_read", i=b.changed()); b.run("FLAT", n=60, zoff=-8); b.op("z_read", i=b.changed())
    b.run("FLAT", n=60, zoff=-10); i, j = b.changed(), b.changed(5); b.op("z_copy", i=i, j=j); b.run("FLAT", r=0, n=30, zoff=-12)
    b.op("z_copy", i=3, j=b.changed()); b.run("FLAT", r=0, n=30, zoff=-13)
    b.op("z_size"); b.op("z_ref"); b.done()

    b = _Build("z_writes", SMALL4)                      # hazard 5 on the small frame: writes that block and that open pixels
    i = b.covered(0)
    b.run("GOURAUD", r=2, n=20)
    for k in range(-3, 4):
        b.op("z_write", i=i + k, v=-9.0)                # nearer than anything: the next run cannot pass
    b.run("GOURAUD", r=2, n=20, zoff=-5)
    for k in range(-3, 4):
        b.op("z_write", i=i + 37 + k, v=float("inf"))   # open again: the next run passes wherever it covers
    b.run("GOURAUD", r=0, n=30, zoff=-7); b.op("z_read", i=i); b.op("z_read", i=i + 37); b.run("GOURAUD", r=0, n=30, zoff=-9)     # (small: most opened pixels stay open)
    b.op("z_iter"); b.done()

    b = _Build("save_restore")                          # hazard 6: saved = zbuffer ... zbuffer = saved inside runs of one kind
    b.run("FLAT", r=2, n=20); b.op("z_save"); b.run("FLAT", r=2, n=20, zoff=-6); b.op("z_load"); b.run("FLAT", r=2, n=20, zoff=-3)
    b.op("z_ref"); b.op("stats"); b.done()

    b = _Build("save_restore_small", SMALL1)
    b.run("CHECKER", r=2, n=20); b.op("z_save"); b.run("CHECKER", r=2, n=20, zoff=-6); b.op("z_load"); b.run("CHECKER", r=2, n=20, zoff=-3)
    b.op("z_iter"); b.done()

    b = _Build("init_zbuffer_mid")                      # hazard 7: init_zbuffer between runs of one kind
    b.run("GOURAUD", r=2, n=20, zoff=-6); b.op("init_zbuffer", w=96, h=64); b.run("GOURAUD", r=2, n=20); b.op("z_size")
    b.op("flush", fb=0); b.op("z_iter"); b.done()

    b = _Build("texture_replaced")                      # hazard 8: a sampled slot replaced between two PHONG runs
    b.textures(); b.op("modelview", seed=5)
    b.run("PHONG", r=2, n=20); b.op("upload_texture", fb=0, slot=0, w=5, h=11, bpp=4, seed=b.seed()); b.run("PHONG", r=2, n=20, zoff=4)
    b.done()

    b = _Build("clip_planes")                           # hazard 9: the plane switched on, changed and off between runs of one kind
    b.run("FLAT", r=2, n=20); b.op("clip_plane", plane="slant"); b.run("FLAT", r=2, n=20); b.op("clip_plane", plane="off"); b.run("FLAT", r=2, n=20)
    b.run("GOURAUD", r=2, n=20); b.op("clip_plane", plane="near"); b.run("GOURAUD", r=2, n=20); b.op("clip_plane", plane="slant")
    b.run("GOURAUD", r=2, n=20); b.op("clip_plane", plane="off"); b.run("GOURAUD", r=2, n=20)
    b.op("stats"); b.done()

    b = _Build("indexed_between")                       # hazard 10: gl_draw_indexed between two runs of one kind and uniforms
    b.textures(); b.op("modelview", seed=6)
    b.run("PHONG", r=2, n=20); b.op("draw_indexed", fb=0, seed=b.seed(), s=10, tex=TEX); b.run("PHONG", r=2, n=20)
    b.op("stats"); b.done()

    b = _Build("batch_bound")                           # hazard 11: three coincident triangles across the batch bound
    b.run("FLAT", r=2, n=BATCH + 3, tie=BATCH - 1); b.run("GOURAUD", r=2, n=2 * BATCH + 2, tie=2 * BATCH - 2)
    b.op("stats"); b.op("flush", fb=0); b.op("z_ref"); b.done()

    b = _Build("stats_mid", SMALL4)                     # hazard 12: print_render_stats() with a run batched, and at the ends
    b.run("FLAT"); b.op("stats"); b.run("FLAT"); b.op("stats"); b.op("stats"); b.run("CHECKER"); b.op("flush", fb=0); b.op("stats")
    b.done()

    b = _Build("flushes")                               # host pixel writes; gl_flush twice in a row and with nothing pending
    b.op("flush", fb=0); b.run("FLAT", r=2, n=20); b.op("flush", fb=0); b.op("flush", fb=0)
    for k in range(6):
        b.op("fb_set", fb=0, x=40 + 3 * k, y=30 + k, c=(250 - k, 3 * k, 77, 255))
    b.op("fb_modified", fb=0); b.run("FLAT", r=1, n=60, zoff=5); b.op("flush", fb=0)
    b.op("fb_set", fb=0, x=0, y=0, c=(1, 2, 3, 4)); b.op("fb_modified", fb=0); b.op("dump", fb=0)
    b.done()

    b = _Build("other_size_flushed")                    # hazard 13: gl_flush(old), then a framebuffer of another size and bpp; a user kind on both
    b.op("register_shader", src="UCHECKER")
    b.run("UCHECKER", r=2, n=20); b.run("FLAT", r=2, n=20); b.op("stats"); b.op("flush", fb=0)
    b.image(1, SMALL4, (9, 8, 7, 6)); b.op("init_zbuffer", w=37, h=29); b.viewport((0, 0, 37, 29))
    b.run("UCHECKER", fb=1, r=2, n=20); b.run("GOURAUD", fb=1, r=2, n=20); b.op("stats"); b.op("flush", fb=1); b.op("z_iter")
    b.op("init_zbuffer", w=96, h=64); b.viewport((0, 0, 96, 64)); b.run("UCHECKER", r=2, n=20); b.op("stats"); b.op("dump", fb=1)
    b.done()

    b = _Build("other_size_pending")                    # hazard 14: triangles pending for the old framebuffer when the new one is first drawn into
    b.run("FLAT", r=2, n=20); b.op("flush", fb=0); b.run("FLAT", r=2, n=20)
    b.image(1, SMALL1, (200, 0, 0, 0)); b.viewport((0, 0, 37, 29))
    b.run("FLAT", fb=1, r=2, n=20); b.op("stats"); b.op("flush", fb=1); b.op("z_ref"); b.op("dump", fb=0)
    b.op("init_zbuffer", w=96, h=64); b.viewport((0, 0, 96, 64)); b.run("GOURAUD", r=2, n=20)           # ... and back, with the small one's work flushed
    b.op("stats"); b.done()

    b = _Build("other_size_pending_same_viewport", SMALL4)      # hazard 14 with Viewport and kind unchanged, and through gl_flush(new) alone
    b.run("GOURAUD", r=2, n=20); b.op("flush", fb=0); b.run("GOURAUD", r=2, n=20)
    b.image(1, MAIN, (1, 2, 3, 4))
    b.run("GOURAUD", fb=1, r=2, n=20); b.op("stats"); b.op("flush", fb=1); b.op("z_size"); b.op("z_iter"); b.op("dump", fb=0)
    b.run("GOURAUD", fb=1, r=2, n=20)
    b.image(2, SMALL1, (5, 0, 0, 0)); b.op("flush", fb=2); b.op("stats"); b.op("z_size")
    b.done(fb=2)

    b = _Build("same_size_images")                      # hazard 15: a second image of the frame's size, with and without gl_flush(old)
    b.image(1, MAIN, (0, 90, 180, 255))
    b.run("FLAT", r=2, n=20); b.op("flush", fb=0); b.op("fb_modified", fb=1); b.run("FLAT", fb=1, r=2, n=20, zoff=3); b.op("z_read", i=b.covered())
    b.op("flush", fb=1); b.op("dump", fb=0)
    b.op("fb_modified", fb=0); b.run("FLAT", r=1, zoff=-4); b.op("fb_modified", fb=1); b.run("FLAT", fb=1, r=1, zoff=-6)       # (A's pixels stay on the device)
    b.op("stats"); b.op("flush", fb=1); b.op("z_ref"); b.op("dump", fb=0)
    b.done(fb=1)

    b = _Build("same_size_other_bpp", SMALL4)           # hazard 14 where the depths fit the new framebuffer: they persist, the pending run's too
    b.run("FLAT", r=2, n=20); b.op("flush", fb=0); b.run("FLAT", r=2, n=20)
    b.image(1, SMALL1, (90, 0, 0, 0)); b.run("FLAT", fb=1, r=2, n=20); b.op("stats"); b.op("flush", fb=1); b.op("z_iter"); b.op("dump", fb=0)
    b.op("fb_set", fb=0, x=5, y=6, c=(9, 99, 199, 29)); b.op("fb_modified", fb=0)       # back, the first image named by gl_framebuffer_modified alone
    b.run("FLAT", r=0, n=30, zoff=-9); b.op("z_read", i=b.changed()); b.op("stats")
    b.done()
    return dict(_built)


# ---- where a rule of the shim is at work -----------------------------------------------------------------------------------------------
ELEMENT_OPS = ("z_read", "z_write", "z_copy")


def _neighbour(ops, i, step):
    """The index of the nearest operation before / behind i that is a call into the shim, or None; for a use of one element of zbuffer,
    the nearest that is not such a use either (a caller reads and writes several between two runs)."""
    skip = STATE_OPS + (ELEMENT_OPS if ops[i][0] in ELEMENT_OPS else ())
    k = i + step
    while 0 <= k < len(ops) and ops[k][0] in skip:
        k += step
    return k if 0 <= k < len(ops) else None


def _run_at(ops, k, fb=None):
    return k is not None and ops[k][0] == "rasterize" and (fb is None or ops[k][1]["fb"] == fb)


def occurrences(p):
    """[(hazard, operation index)] of a program, hazards numbered as in tests/test_shim_programs.py."""
    out, ops = [], p.ops
    dims = {a["fb"]: (a["w"], a["h"], a["bpp"]) for n, a in ops if n == "image"}
    registered = set()
    for i, (n, a) in enumerate(ops):
        before, behind = _neighbour(ops, i, -1), _neighbour(ops, i, +1)
        between = _run_at(ops, before) and _run_at(ops, behind) and ops[before][1]["fb"] == ops[behind][1]["fb"]
        same_kind = between and ops[before][1]["kind"] == ops[behind][1]["kind"]
        if n == "register_shader":
            registered.add(a["src"])
        elif n == "rasterize" and _run_at(ops, before, a["fb"]):
            b = ops[before][1]
            state = [m for m, _ in ops[before + 1:i]]
            rects = [tuple(c["rect"]) for m, c in ops[:i] if m == "init_viewport"]
            if b["kind"] == a["kind"]:
                uniforms = lambda x: (x.get("cells"), x.get("s"), x.get("tex"))
                if uniforms(a) != uniforms(b) or (a["kind"] == "PHONG" and "modelview" in state):
                    out.append((1, i))
                if "init_viewport" in state and rects[-1] != rects[-1 - state.count("init_viewport")]:
                    out.append((2, i))
            else:
                out.append((3, i))
        elif n == "rasterize" and a["kind"] == "UCHECKER" and "UCHECKER" in registered:
            last = [(m, c) for m, c in ops[:i] if "fb" in c and m != "image"][-1:]      # the last call that named a framebuffer
            if last and last[0][0] == "flush" and dims[last[0][1]["fb"]] != dims[a["fb"]]:
                out.append((13, i))
        if n in ("rasterize", "flush") and _run_at(ops, before) and dims[ops[before][1]["fb"]] != dims[a["fb"]]:
            out.append((14, i))
        if n == "rasterize" and "tie" in a and a["tie"] // BATCH != (a["tie"] + 2) // BATCH:       # (the three triangles are in two batches)
            out.append((11, i))
        if n in ("z_read", "z_copy") and between:
            out.append((4, i))
        if n in ("z_write", "z_copy") and same_kind:
            out.append((5, i))
        if n in ("z_save", "z_load") and same_kind:
            out.append((6, i))
        if n == "init_zbuffer" and same_kind:
            out.append((7, i))
        if n == "upload_texture" and same_kind and ops[before][1]["kind"] == "PHONG" and a["slot"] in ops[before][1]["tex"]:
            out.append((8, i))
        if n == "clip_plane" and same_kind:
            out.append((9, i))
        if n == "draw_indexed" and same_kind and ops[before][1]["kind"] == "PHONG" and \
                all(ops[before][1][k] == ops[behind][1][k] for k in ("s", "tex")) and "modelview" not in [m for m, _ in ops[before:behind]]:
            out.append((10, i))
        if n == "stats" and _run_at(ops, before) and behind is not None:
            out.append((12, i))
        if n == "fb_modified" and before is not None and ops[before][0] == "flush" and ops[before][1]["fb"] != a["fb"] and \
                dims[ops[before][1]["fb"]] == dims[a["fb"]] and _run_at(ops, behind, a["fb"]):
            out.append((15, i))
    return out


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class _Model:
    """The reference's state, and - for the lazy variants - the triangles a deferred implementation holds back."""

    def __init__(self, p, lazy):
        self.p, self.lazy = p, lazy
        self.pixels, self.host, self.dims = {}, {}, {}  # per image: what the reference has drawn; what the caller's TGAImage holds
        self.z, self.saved = np.zeros(0), np.zeros(0)   # the global depth vector
        self.fetched = self.z                           # lazy 'read_dirty': the host copy as it was last fetched in full
        self.o, self.bound = None, None                 # the counters and textures of the context; the image it serves
        self.mv, self.vp, self.plane = np.eye(4), np.eye(4), None
        self.pending, self.obs, self.user = [], [], []
        self.lost_kinds = False

    def off(self, rule, i):
        return self.lazy is not None and self.lazy[0] == rule and self.lazy[1] in (None, i)

    # -- the context: counters restart with a framebuffer of another size or bpp, depths persist when they fit; the shim serves one
    #    framebuffer at a time, so pixels drawn into an image and not fetched by gl_flush() before another takes its place are gone --
    def switch(self, fb, keep=False):
        if self.bound is not None and self.bound != fb:
            if keep:                                    # lazy 'no_modified': the device's frame still holds the other image
                self.pixels[fb][:] = self.pixels[self.bound]
            self.pixels[self.bound][:] = self.host[self.bound]
        self.bound = fb

    def bind(self, fb, i):
        from oracle import orc
        d = self.dims[fb]
        if self.o is None or (self.o.w, self.o.h, self.o.bpp) != d:
            if not self.off("into_bound", i):
                self.submit()                           # what is pending belongs to the old framebuffer
            if self.o is not None and self.off("user_lost", None):
                self.lost_kinds = True
            self.o = orc.Oracle(*d)
            if self.z.size != d[0] * d[1]:
                self.z = np.full(d[0] * d[1], np.inf)
            self.switch(fb)
        assert self.bound == fb, "an image of the frame's size takes its place through gl_framebuffer_modified()"

    def point_at(self, fb):
        o = self.o
        o.fb, o.z = self.pixels[fb], self.z.reshape(o.h, o.w)
        o.t.fb, o.t.zbuf = o.fb.ctypes.data, o.z.ctypes.data

    # -- draws --
    def draw(self, run):
        a, fb = run["a"], run["fb"]
        base = cp.KINDS[a["kind"]][0]
        if self.lost_kinds and a["kind"] == "UCHECKER":
            return
        clip, vary, col, u = run_arrays(self.dims[a["fb"]], a)
        if base == PHONG:
            u.model_view[:] = run["mv"].reshape(16).tolist()
        parts = [slice(None)]
        if self.off("tail_first", run["i"]) and a["n"] > BATCH:
            cut = a["n"] - a["n"] % BATCH
            parts = [slice(cut, None), slice(0, cut)]
        for part in parts:
            c, v, k = clip[part], None if vary is None else vary[part], None if col is None else col[part]
            if run["plane"] is not None:
                c, v, k = clip_model.clip_model(cp.PLANES[run["plane"]], c, v, k, attrs=clip_model.LAYOUTS[base])
            if c.shape[0]:
                self.point_at(fb)
                self.o.set_viewport(run["vp"])
                self.o.draw(base, c, v, k, cp._orc_uniforms(u))

    def submit(self):
        runs, self.pending = self.pending, []
        if self.off("by_kind", None):                   # one batch per kind, in the order the kinds first came
            order = []
            for r in runs:
                if r["a"]["kind"] not in order:
                    order.append(r["a"]["kind"])
            runs.sort(key=lambda r: order.index(r["a"]["kind"]))
        for r in runs:
            if self.lazy and self.lazy[0] == "into_bound" and self.dims[r["fb"]] != self.dims[self.bound]:
                r = dict(r, fb=self.bound)              # (its arrays stay those made for the old frame)
            self.draw(r)

    def rasterize(self, i, a):
        self.bind(a["fb"], i)
        run = dict(i=i, a=a, fb=a["fb"], mv=self.mv.copy(), vp=self.vp.copy(), plane=self.plane)
        if self.lazy is None:
            self.draw(run)
            return
        if self.off("late_state", i):                   # no cut: the batch goes out under the uniforms and Viewport of its last triangle
            for r in reversed(self.pending):
                if r["a"]["kind"] != a["kind"] or r["fb"] != a["fb"]:
                    break
                r["mv"], r["vp"] = run["mv"], run["vp"]
                r["a"] = dict(r["a"], **{k: a[k] for k in ("cells", "s", "tex") if k in a})
        self.pending.append(run)

    def step(self, i, name, a):
        from oracle import orc
        rule = {"z_read": "read_before", "z_write": "write_before", "z_save": "save_before", "z_load": "save_before",
                "init_zbuffer": "init_before", "upload_texture": "upload_before", "clip_plane": "late_plane", "draw_indexed": "indexed_first",
                "stats": "stats_before"}.get(name)
        if name == "z_copy":
            rule = "read_before" if self.off("read_before", i) else "write_before"
        if name not in STATE_OPS + ("rasterize", "register_shader") and not (rule and self.off(rule, i)):
            if not (name in ("flush", "upload_texture", "draw_indexed") and self.off("into_bound", i)):
                self.submit()
        if name == "image":
            d = (a["w"], a["h"], a["bpp"])
            self.dims[a["fb"]] = d
            self.pixels[a["fb"]] = np.empty((d[1], d[0], d[2]), np.uint8)
            self.pixels[a["fb"]][:] = np.array(a["fill"][:d[2]], np.uint8)
            self.host[a["fb"]] = self.pixels[a["fb"]].copy()
        elif name == "register_shader":
            self.user.append(a["src"])
            self.obs.append(("kind", i, SHADER_USER_FIRST + len(self.user) - 1))
        elif name == "rasterize":
            self.rasterize(i, a)
        elif name == "modelview":
            self.mv = model_view(a["seed"])
        elif name == "init_viewport":
            self.vp = scenes.init_viewport(*a["rect"])
        elif name == "z_read":
            self.obs.append(("double", i, float(self.z[a["i"]])))
            if self.off("read_dirty", i):               # the copy fetched earlier goes back to the device in front of the next run
                self.z = self.fetched.copy()
        elif name == "z_write":
            self.z[a["i"]] = a["v"]
        elif name == "z_copy":
            self.z[a["i"]] = self.z[a["j"]]
        elif name == "z_save":
            self.saved = self.z.copy()
        elif name == "z_load":
            self.z = self.saved.copy()
        elif name in ("z_iter", "z_ref"):
            self.obs.append(("depths", i, self.z.copy()))
        elif name == "z_size":
            self.obs.append(("size", i, int(self.z.size)))
        elif name == "init_zbuffer":
            self.z = np.full(a["w"] * a["h"], np.inf)
        elif name == "flush":
            self.bind(a["fb"], i)
            if self.off("into_bound", i):
                self.submit()
            self.host[a["fb"]] = self.pixels[a["fb"]].copy()
            self.obs.append(("image", i, 1, 0, self.host[a["fb"]].copy()))
        elif name == "fb_set":
            bpp = self.dims[a["fb"]][2]
            for img in (self.pixels[a["fb"]], self.host[a["fb"]]):
                img[a["y"], a["x"]] = np.array(a["c"][:bpp], np.uint8)
        elif name == "fb_modified":
            if self.o is not None and (self.o.w, self.o.h, self.o.bpp) != self.dims[a["fb"]]:
                self.bind(a["fb"], i)                   # an image of another size: the call is the first that names it
            elif self.o is not None:
                self.switch(a["fb"], keep=self.off("no_modified", i))
        elif name == "upload_texture":
            self.bind(a["fb"], i)
            self.o.upload_texture(a["slot"], cp.texels(a))
        elif name == "clip_plane":
            self.plane = None if a["plane"] == "off" else a["plane"]
            if self.off("late_plane", i):
                for r in self.pending:
                    r["plane"] = self.plane
        elif name == "draw_indexed":
            self.bind(a["fb"], i)
            assert self.plane is None
            verts, idx, u, proj = cp.mesh_arrays(_Dims(*self.dims[a["fb"]][:2]), a)
            u.model_view[:] = self.mv.reshape(16).tolist()
            clip, vary = orc.vertex_stage(self.mv, proj, verts, idx)
            self.point_at(a["fb"])
            self.o.set_viewport(self.vp)
            self.o.draw(PHONG, clip, vary, None, cp._orc_uniforms(u))
        elif name == "stats":
            self.obs.append(("stats", i, orc.format_stats_line(self.o.stats)))
        elif name == "dump":
            self.obs.append(("image", i, 1, 0, self.host[a["fb"]].copy()))
        else:
            raise AssertionError(name)
        if name in ("z_iter", "z_ref", "z_save", "z_load", "z_write", "z_copy", "init_zbuffer"):
            self.fetched = self.z.copy()


LAZY_RULES = ("late_state", "by_kind", "read_before", "read_dirty", "write_before", "save_before", "init_before", "upload_before", "late_plane",
              "indexed_first", "tail_first", "stats_before", "user_lost", "into_bound", "no_modified")


def run_model(program, lazy=None):
    """The observations of a program executed at once.  lazy = (rule, i): a deferred implementation that holds every run of triangles
    back until the next call into it, without one rule at operation i (None: everywhere):
      late_state     rasterize() does not cut its batch for other uniforms or another Viewport: the batch goes out under the last ones
      by_kind        one batch per kind, submitted in the order the kinds first came
      read_before    zbuffer[i] is read without completing the pending run
      read_dirty     zbuffer[i] marks the host copy modified without having fetched it: the copy fetched by the last whole access
                     (a range-for, a copy, an assignment) goes back to the device in front of the next run
      write_before   zbuffer[i] = v lands before the pending run is drawn
      save_before    saved = zbuffer / zbuffer = saved likewise
      init_before    init_zbuffer likewise: the pending run is tested against the fresh depths
      upload_before  gl_upload_texture likewise: the pending run samples the new texels
      late_plane     the pending run is cut by the plane set when it is submitted
      indexed_first  gl_draw_indexed draws in front of the pending run
      tail_first     a run longer than the batch bound: the triangles behind the last full batch come first
      stats_before   print_render_stats() does not count the pending run
      user_lost      a context for a framebuffer of another size has no user kinds: their triangles are not drawn
      into_bound     the triangles pending for a framebuffer of another size are drawn into the new one
      no_modified    gl_framebuffer_modified(other image) is not honoured: the draws land on the first image's pixels"""
    assert lazy is None or lazy[0] in LAZY_RULES, lazy
    m = _Model(program, lazy)
    for i, (name, a) in enumerate(program.ops):
        m.step(i, name, a)
    m.submit()
    m.obs.append(("error", len(program.ops), 0, ""))
    return m.obs


def differs(got, want):
    """Whether two lists of observations differ in any bit."""
    if len(got) != len(want):
        return True
    for g, w in zip(got, want):
        if g[:2] != w[:2] or len(g) != len(w):
            return True
        for x, y in zip(g[2:], w[2:]):
            if isinstance(y, np.ndarray):
                if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                    return True
            elif isinstance(y, float):
                if struct.pack("<d", x) != struct.pack("<d", y):
                    return True
            elif x != y:
                return True
    return False


def assert_same(program, got, want):
    """Every observation of the driver equals the model's, bit for bit; the message names the first that differs and the program up to it."""
    for k, (g, w) in enumerate(zip(got, want)):
        if differs([g], [w]):
            what = ""
            if g[:2] == w[:2] and isinstance(w[-1], np.ndarray) and g[-1].shape == w[-1].shape:
                bad = np.argwhere(g[-1].view(np.uint8 if w[-1].dtype == np.uint8 else np.uint64) != w[-1].view(np.uint8 if w[-1].dtype == np.uint8 else np.uint64))
                what = f"{len(bad)} elements differ, the first at {bad[0].tolist()}: got {g[-1][tuple(bad[0])]!r}, expected {w[-1][tuple(bad[0])]!r}; "
                g, w = g[:-1], w[:-1]
            raise AssertionError(f"program {program.family}: observation {k} ({w[0]} at operation {w[1]}) differs: {what}got {g}, expected {w}\n"
                                 f"{program.text(min(w[1], len(program.ops) - 1) + 1)}")
    assert len(got) == len(want), (len(got), len(want))


# ---- the driver's side -----------------------------------------------------------------------------------------------------------------
def _phong_fields(u, a):
    return (np.array(list(u.key_light_dir_eye) + list(u.fill_light_dir_eye) + list(u.rim_light_dir_eye) + [u.normal_map_strength], np.float64).tobytes() +
            struct.pack("<3i", *a["tex"]))


def encode(program):
    """The program as tests/host/shim_program.cpp reads it: 'SHIMPRG1', then per operation an int32 opcode, its fields and its arrays."""
    out, dims, user = [b"SHIMPRG1"], {}, []
    for name, a in program.ops:
        out.append(struct.pack("<i", OPCODES[name]))
        if name == "image":
            dims[a["fb"]] = (a["w"], a["h"], a["bpp"])
            out.append(struct.pack("<4i4B", a["fb"], a["w"], a["h"], a["bpp"], *a["fill"]))
        elif name == "register_shader":
            base, src, K, may_discard = cp.KINDS[a["src"]]
            user.append(a["src"])
            out.append(struct.pack("<3i", K, int(may_discard), len(src.encode())) + src.encode())
        elif name == "rasterize":
            clip, vary, col, u = run_arrays(dims[a["fb"]], a)
            code = KIND_CODES[a["kind"]] + (user.index(a["kind"]) if a["kind"] in user else 0)
            out.append(struct.pack("<4i", a["fb"], code, a["n"], a.get("cells", 0)))
            if a["kind"] == "PHONG":
                out.append(_phong_fields(u, a))
            out.append(np.ascontiguousarray(clip, np.float64).tobytes())
            out.append((np.zeros(a["n"], np.uint32) if col is None else np.ascontiguousarray(col, np.uint32)).tobytes())
            if vary is not None:
                out.append(np.ascontiguousarray(vary, np.float64).tobytes())
        elif name == "modelview":
            out.append(model_view(a["seed"]).tobytes())
        elif name == "init_viewport":
            out.append(struct.pack("<4i", *a["rect"]))
        elif name == "z_read":
            out.append(struct.pack("<i", a["i"]))
        elif name == "z_write":
            out.append(struct.pack("<id", a["i"], a["v"]))
        elif name == "z_copy":
            out.append(struct.pack("<2i", a["i"], a["j"]))
        elif name == "init_zbuffer":
            out.append(struct.pack("<2i", a["w"], a["h"]))
        elif name in ("flush", "fb_modified", "dump"):
            out.append(struct.pack("<i", a["fb"]))
        elif name == "fb_set":
            out.append(struct.pack("<3i4B", a["fb"], a["x"], a["y"], *a["c"]))
        elif name == "upload_texture":
            out.append(struct.pack("<5i", a["fb"], a["slot"], a["w"], a["h"], a["bpp"]) + np.ascontiguousarray(cp.texels(a)).tobytes())
        elif name == "clip_plane":
            plane = (0.0, 0.0, 0.0, 0.0) if a["plane"] == "off" else cp.PLANES[a["plane"]]
            out.append(struct.pack("<i4d", int(a["plane"] != "off"), *plane))
        elif name == "draw_indexed":
            verts, idx, u, proj = cp.mesh_arrays(_Dims(*dims[a["fb"]][:2]), a)
            out.append(struct.pack("<i", a["fb"]) + _phong_fields(u, a) + np.ascontiguousarray(proj, np.float64).tobytes())
            out.append(struct.pack("<3i", verts.shape[1], verts.shape[0], idx.shape[0]))
            out.append(np.ascontiguousarray(verts, np.float64).tobytes() + np.ascontiguousarray(idx, np.uint32).tobytes())
        else:
            assert name in ("z_save", "z_load", "z_iter", "z_size", "z_ref", "stats"), name
    out.append(struct.pack("<i", OPCODES["end"]))
    return b"".join(out)


def decode(program, out, err):
    """The observations of a driver run, in run_model's form: the records of its output file, and the lines print_render_stats() wrote to
    stderr, one per `stats` operation in their order."""
    dims = {a["fb"]: (a["w"], a["h"], a["bpp"]) for n, a in program.ops if n == "image"}
    obs, pos = [], 0
    while pos < len(out):
        tag, i, size = struct.unpack_from("<2iQ", out, pos)
        body = out[pos + 16: pos + 16 + size]
        pos += 16 + size
        tag = TAGS[tag]
        if tag == "image":
            ok, code = struct.unpack_from("<2i", body)
            d = dims[program.ops[i][1]["fb"]]
            obs.append((tag, i, ok, code, np.frombuffer(body, np.uint8, offset=8).reshape(d[1], d[0], d[2]).copy()))
        elif tag == "depths":
            obs.append((tag, i, np.frombuffer(body, np.float64).copy()))
        elif tag == "double":
            obs.append((tag, i, struct.unpack("<d", body)[0]))
        elif tag == "size":
            obs.append((tag, i, struct.unpack("<Q", body)[0]))
        elif tag == "kind":
            obs.append((tag, i, struct.unpack("<i", body)[0]))
        else:
            obs.append((tag, len(program.ops), struct.unpack_from("<i", body)[0], body[4:].decode()))
    lines = [ln for ln in err.splitlines() if ln.startswith("DEBUG: triangles=")]
    at = [i for i, (n, _) in enumerate(program.ops) if n == "stats"]
    assert len(lines) == len(at), (len(lines), len(at), err)
    obs += [("stats", i, ln) for i, ln in zip(at, lines)]
    return sorted(obs, key=lambda o: o[1])


PROGRAMS = _programs()
B64 = ("batch_bound", "z_reads", "kinds_small")         # the programs the driver with the small batch bound runs as well
