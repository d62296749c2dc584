"""Call sequences against an immediate-mode model of the reference.

The reference's rasterize() is immediate: it reads the Viewport, the textures, the z-buffer and the counters when it is called.  The
library queues draws and runs them at a flush, so whether a frame still equals the reference's depends on the host rules of
csrc/trgl_api.cpp (end_pending_raster, flush_queued, flush_sync, StageHold, the kind cut of trgl_draw).  A *program* is a list of API
calls made from a seed; run_model executes it at once on the CPU oracle, run_gpu on one Context, and both return the observations the
program asked for, which must be equal.

  generate(family, seed) -> Program         one line of text per operation: Program.text() / Program.parse()
  run_model(program)     -> [observation]   (+ the hazards it met, for tests/test_call_programs.py)
  run_gpu(program)       -> [observation]
  assert_same(program, got, want)

An operation is (name, args) with args a dict of ints, floats, names and tuples of ints; the arrays of a draw are made from the seed in
its args (draw_arrays, mesh_arrays, texels), so the text alone reproduces a program.  Families (FAMILIES): A flat kinds on bpp 1 / 3 / 4,
B shaded kinds with textures, E the same with EYE draws (compared with the harness's EYE rule), S strips over caller-written buffers,
D a discarding user kind between other kinds."""
import ctypes as C
import os
import re

import numpy as np

import cases
import discard_shader_sources as DS
import image_ops_model
import user_shader_sources as US
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, GOURAUD, PHONG, EYE, CHECKER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLUR_LDS_RADIUS = int(re.search(r"constexpr int BLUR_LDS_RADIUS = (\d+);",
                                open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()).group(1))
MAX_DRAWS = int(re.search(r"#define TRGL_MAX_DRAWS (\d+)",
                          open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "trgl_device.h")).read()).group(1))
E_INVALID, E_STATE = -1, -4

FAMILIES = "ABESD"
SEEDS = {f: tuple(range(8)) for f in FAMILIES}          # the committed seed list: tests/test_call_programs.py proves what it can notice

# kind name -> (the built-in kind the model renders it as, the source a context registers for it, K, may_discard)
KINDS = {"FLAT": (FLAT, None, 0, False), "GOURAUD": (GOURAUD, None, 3, False), "CHECKER": (CHECKER, None, 0, False),
         "PHONG": (PHONG, None, 24, False), "EYE": (EYE, None, 24, False),
         "UFLAT": (FLAT, US.FLAT, 0, False), "UGOURAUD": (GOURAUD, US.GOURAUD, 3, False), "UPHONG": (PHONG, US.PHONG, 24, False),
         "UCHECKER": (CHECKER, DS.CHECKER, 0, True)}
# sources that register_shader adds while draws are queued and that nothing draws
EXTRA_SOURCES = {"XGOURAUD_PADDED": (US.GOURAUD_PADDED, 5, False), "XEYE": (US.EYE, 24, False), "XCHECKER_B": (DS.CHECKER_B, 0, True),
                 "XDISCARD_ALL": (DS.DISCARD_ALL, 0, True)}
SHADED = (PHONG, EYE)                                   # kinds with uniforms, textures and 24 varyings
RADII = ((1, 8, 300), (4, 40, 120), (30, 160, 10))     # classes of a draw's triangles: rmin, rmax, most triangles
FRAMES = ((96, 64), (101, 67), (160, 128))
# operations that make a deferred implementation run what is queued (where a lazily applied state change would land)
FLUSH_POINTS = {"flush", "flush_begin", "flush_end", "read_fb", "read_z", "stats", "observe", "postprocess", "write_framebuffer",
                "write_zbuffer", "zbuffer_snapshot", "zbuffer_restore", "framebuffer_blur", "clear", "reset_stats", "upload_texture",
                "set_strip", "set_interleave", "set_stream", "set_viewport", "init_viewport"}
OBSERVATIONS = {"read_fb", "read_z", "stats", "observe", "postprocess"}
MID_OPS = ("draw", "set_viewport", "upload_texture", "clear", "zbuffer_snapshot", "framebuffer_blur", "set_stream", "register_shader",
           "mesh_bounds", "observe")


# ---- programs as text ---------------------------------------------------------------------------------------------------
def _fmt(v):
    if isinstance(v, tuple):
        return ",".join(str(int(x)) for x in v)
    return repr(v) if isinstance(v, float) else str(v)


def _parse(s):
    if "," in s:
        return tuple(int(x) for x in s.split(","))
    for conv in (int, float):
        try:
            return conv(s)
        except ValueError:
            pass
    return s


class Program:
    def __init__(self, family, seed, w, h, bpp, ops):
        self.family, self.seed, self.w, self.h, self.bpp, self.ops = family, seed, w, h, bpp, list(ops)

    def __eq__(self, other):
        return (self.family, self.seed, self.w, self.h, self.bpp, self.ops) == (other.family, other.seed, other.w, other.h, other.bpp, other.ops)

    def text(self, upto=None):
        """One line per operation (the first `upto` of them), behind a header line."""
        ops = self.ops if upto is None else self.ops[:upto]
        lines = [f"program family={self.family} seed={self.seed} w={self.w} h={self.h} bpp={self.bpp}"]
        lines += [" ".join([name] + [f"{k}={_fmt(v)}" for k, v in a.items()]) for name, a in ops]
        return "\n".join(lines)

    @staticmethod
    def parse(text):
        lines = [ln.split() for ln in text.strip().splitlines() if ln.strip()]
        assert lines[0][0] == "program", lines[0]
        head = {k: _parse(v) for k, v in (kv.split("=", 1) for kv in lines[0][1:])}
        ops = [(ln[0], {k: _parse(v) for k, v in (kv.split("=", 1) for kv in ln[1:])}) for ln in lines[1:]]
        return Program(str(head["family"]), head["seed"], head["w"], head["h"], head["bpp"], ops)

    def moved(self, i, j):
        """The program with operation i taken out and put in front of what is operation j now."""
        ops = list(self.ops)
        op = ops.pop(i)
        ops.insert(j - 1 if j > i else j, op)
        return Program(self.family, self.seed, self.w, self.h, self.bpp, ops)


# ---- the arrays an operation stands for -----------------------------------------------------------------------------------
def _shaded_uniforms(a):
    hd = scenes.head_standin(0, 16, 16, seed=a["seed"])
    return api.make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], a["s"] / 10.0, *a["tex"])


def draw_arrays(p, a):
    """(clip [n, 12], varyings or None, colors or None, uniforms or None) of a draw operation: fresh arrays on every call."""
    rmin, rmax, _ = RADII[a["r"]]
    n, base = a["n"], KINDS[a["kind"]][0]
    clip, _ = scenes.random_triangles(n, p.w, p.h, seed=a["seed"], rmin=rmin, rmax=rmax, perspective_w=True)
    col = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(a["seed"] * 97)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if base == GOURAUD:
        return clip, scenes.SplitMix64(a["seed"] + 1).uniform(n * 3, -0.2, 1.3).reshape(n, 3), col, None
    if base in SHADED:
        return clip, cases.phong_soup_varyings(n, a["seed"] + 2), None, _shaded_uniforms(a)
    return clip, None, col, api.make_uniforms(cells=a["cells"]) if base == CHECKER else None


def mesh_arrays(p, a):
    """(vertices [nv, 8], indices [nf, 3], uniforms, projection) of a draw_indexed operation: the head stand-in over icosphere(1)."""
    hd = scenes.head_standin(1, p.w, p.h, seed=a["seed"])
    verts = np.ascontiguousarray(np.concatenate([hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)], 1))
    idx = np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)
    u = api.make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], a["s"] / 10.0, *a["tex"])
    # (near and far planes close around the mesh: its depths spread over the range the triangle soups use, so neither hides the other)
    return verts, idx, u, np.ascontiguousarray(scenes.perspective(scenes.TAN_35DEG, p.w / p.h, 1.2, 4.5))


def _scribble_uniforms(u):
    """Other bytes in a Uniforms struct that are still a valid block (the model's lazy variant draws with them)."""
    v = api.make_uniforms(np.diag([1.0, -1.0, 1.0, 1.0]), key=(0, 1, 0), fill=(1, 0, 0), rim=(0, 0, -1), normal_map_strength=0.3,
                          cells=u.reserved + 1 if u.reserved > 0 else 0)
    C.memmove(C.addressof(u), C.addressof(v), C.sizeof(v))


def scribble_draw(p, a, clip, vary, col, u):
    """Overwrite the caller's arrays of a draw in place, as a caller may once trgl_draw has returned."""
    rmin, rmax, _ = RADII[a["r"]]
    clip[:] = scenes.random_triangles(clip.shape[0], p.w, p.h, seed=a["seed"] ^ 0x5C81B, rmin=rmin, rmax=rmax, perspective_w=True)[0]
    if vary is not None:
        vary[:] = vary[::-1].copy() * 0.5 + 0.25
    if col is not None:
        col[:] = ~col
    if u is not None:
        _scribble_uniforms(u)


def scribble_mesh(verts, idx, u, proj):
    verts[:] = verts[::-1].copy()
    idx[:] = idx[::-1].copy()
    proj[:] = np.diag([0.5, 0.5, 1.0, 1.0])
    _scribble_uniforms(u)


def texels(a):
    return cases._texels(scenes.SplitMix64(a["seed"]), a["w"], a["h"], a["bpp"])


def written_fb(p, a):
    fb, _ = cases.loaded_buffers(p.w, p.h, p.bpp)
    return ((fb.astype(np.int32) + 37 * a["v"]) & 0xFF).astype(np.uint8)


def written_z(p, a):
    _, z = cases.loaded_buffers(p.w, p.h, p.bpp)
    return np.ascontiguousarray(np.roll(z, 5 * a["v"], axis=0))


def bounds_mesh(a):
    return scenes.SplitMix64(a["seed"]).uniform(a["n"] * 5, -2.0, 2.0).reshape(a["n"], 5)


def burst_ops(a):
    """The draw operations a draw_burst stands for: `count` draws of one triangle each (more than a flush holds)."""
    return [dict(kind=a["kind"], n=1, seed=a["seed"] + 3 * k, r=a["r"], mem="host", scr=0, cells=a.get("cells", 3)) for k in range(a["count"])]


# ---- the generator --------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, family, seed):
        self.f = family
        self.r = scenes.SplitMix64(0xCA11 + 1000 * FAMILIES.index(family) + seed)
        self.w, self.h = FRAMES[1 + seed % 2] if family == "S" else FRAMES[seed % 3]
        self.bpp = (1, 3, 4)[(seed // 3 + seed) % 3] if family in "AS" else (3, 4)[seed % 2]
        self.ops, self.registered, self.extra = [], set(), list(EXTRA_SOURCES)
        self.rect = (0, 0, self.w, self.h)
        self.strip = (0, self.h)
        self.next_seed = 7000 + 500 * seed + 100000 * FAMILIES.index(family)
        self.snapped = set()
        self.torch_stream = False
        self.kinds = {"A": ("FLAT", "GOURAUD", "CHECKER", "UFLAT", "UGOURAUD"), "B": ("PHONG", "UPHONG", "FLAT", "GOURAUD"),
                      "E": ("PHONG", "UPHONG", "FLAT", "GOURAUD", "EYE"), "S": ("FLAT", "GOURAUD", "CHECKER", "PHONG"),
                      "D": ("FLAT", "GOURAUD", "CHECKER", "UCHECKER")}[family]
        self.tex_sets = ((0, 1, 2), (3, 4, 5), (0, 4, -1)) if family in "BE" else ((-1, -1, -1),)

    def below(self, k):
        return int(self.r.u64(1)[0] % np.uint64(k))

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def op(self, name, **a):
        self.ops.append((name, a))

    def seed(self):
        self.next_seed += 11
        return self.next_seed

    # -- single operations --
    def draw(self, kind=None, n=None, r=None, mem=None, seed=None, tex=None, scr=None):
        kind = kind or self.pick(self.kinds)
        if KINDS[kind][1] is not None and kind not in self.registered:
            self.registered.add(kind)
            self.op("register_shader", src=kind)
        r = self.below(3) if r is None else r
        n = 1 + self.below(RADII[r][2]) if n is None else n
        mem = mem or ("dev" if self.below(4) == 0 else "host")
        a = dict(kind=kind, n=n, seed=self.seed() if seed is None else seed, r=r, mem=mem,
                 scr=(self.below(2) if scr is None else scr) if mem == "host" else 0)
        base = KINDS[kind][0]
        if base in SHADED:
            a.update(tex=tex or self.pick(self.tex_sets), s=self.pick((0, 5, 10, 17)))
        if base == CHECKER:
            a.update(cells=2 + self.below(5))
        self.op("draw", **a)
        return a

    def draws(self, k=None):
        """One or two draws that a deferred implementation holds queued afterwards."""
        for _ in range(k or 1 + self.below(2)):
            self.draw()

    def indexed(self, mem=None, seed=None):
        kind = "PHONG" if self.f != "E" or self.below(2) else "EYE"
        mem = mem or ("dev" if self.below(3) == 0 else "host")
        self.op("draw_indexed", kind=kind, seed=self.seed() if seed is None else seed, mem=mem, scr=1 if mem == "host" else 0,
                tex=self.pick(self.tex_sets), s=self.pick((0, 5, 10)))

    def other_rect(self):
        w, h = self.w, self.h
        rects = [(8, 4, w - 16, h - 12), (0, 0, w // 2, h), (w // 4, h // 4, w // 2, h // 2), (-10, -6, w + 20, h + 12), (0, 0, w, h)]
        return self.pick([q for q in rects if q != self.rect])

    def set_viewport(self, same=False):
        if not same:
            self.rect = self.other_rect()
        self.op("set_viewport", rect=self.rect)

    def upload(self, slot, bpp=None):
        self.op("upload_texture", slot=slot, w=3 + 2 * self.below(20), h=3 + 2 * self.below(14), bpp=bpp or self.pick((1, 3, 4)), seed=self.seed())

    def clear(self):
        self.op("clear", bgra=tuple(self.below(256) for _ in range(4)), z=self.pick((0.25, 0.6, 0.9)))

    def observation(self):
        name = self.pick(("read_fb", "read_z", "stats", "observe"))
        self.op(name)

    def postprocess(self):
        self.op("postprocess", final=1 if self.bpp >= 3 and self.f != "E" else 0)

    def blur(self):
        self.op("framebuffer_blur", r=self.pick((1, 2, 3, 5, BLUR_LDS_RADIUS, BLUR_LDS_RADIUS + 1)))

    def snapshot(self):
        slot = self.below(2)
        self.snapped.add(slot)
        self.op("zbuffer_snapshot", slot=slot)

    def restore(self):
        if not self.snapped:
            self.snapshot()
        self.op("zbuffer_restore", slot=self.pick(sorted(self.snapped)))

    def set_stream(self):
        self.torch_stream = not self.torch_stream
        self.op("set_stream", to="torch" if self.torch_stream else "own")

    def register_extra(self):
        if self.extra:
            self.op("register_shader", src=self.extra.pop(0))
        else:
            self.op("mesh_bounds", n=40, seed=self.seed())

    def refused(self):
        what = ["unknown_kind", "bad_strip", "restore_empty"] + (["blur_in_strip"] if self.strip != (0, self.h) else [])
        self.op("refused", what=self.pick(what))

    def change_strip(self):
        if self.below(3) == 0:
            self.strip = (0, self.h)
            self.op("set_interleave", band=32, rank=0, world=1)
        else:
            y0 = self.below(self.h - 8)
            self.strip = (y0, y0 + 4 + self.below(self.h - y0 - 4))
            self.op("set_strip", y0=self.strip[0], y1=self.strip[1])

    # -- phrases: short sequences that put one rule of trgl_api.cpp to work --
    def p_vp_diff(self): self.draws(); self.set_viewport(); self.draws(1)
    def p_vp_same(self): self.draws(); self.set_viewport(same=True); self.draws(1)

    def p_init_vp(self):
        self.draws()
        self.rect = self.other_rect()
        self.op("init_viewport", rect=self.rect)
        self.draws(1)

    def p_write_queued(self):
        self.draws()
        self.op(self.pick(("write_framebuffer", "write_zbuffer")), v=1 + self.below(5))

    def p_reset_queued(self): self.draws(); self.op("reset_stats"); self.draws(1)
    def p_snapshot_restore(self): self.draws(); self.snapshot(); self.draws(); self.restore()
    def p_postprocess_queued(self): self.draws(); self.postprocess()
    def p_refused_queued(self): self.draws(); self.refused()
    def p_zero_draw(self): self.draws(1); self.draw(n=0, mem="host"); self.draw(n=0, mem="dev")
    def p_begin_twice(self): self.draws(); self.op("flush_begin"); self.op("flush_begin"); self.op("flush_end")
    def p_end_alone(self): self.draws(); self.op("flush_end"); self.op("stats")
    def p_stream(self): self.draws(); self.set_stream(); self.draws(); self.set_stream()
    def p_indexed(self): self.indexed(); self.observation()
    def p_dev_draw(self): self.draw(mem="dev"); self.draw(mem="host", scr=1); self.op("sync")
    def p_clear_queued(self): self.draws(); self.clear(); self.draws(1)
    def p_clear_only_flush(self): self.op("flush"); self.clear(); self.op(self.pick(("flush", "flush_begin"))); self.op("flush_end"); self.draws(1)
    def p_write_over_clear(self): self.clear(); self.op(self.pick(("write_framebuffer", "write_zbuffer")), v=1 + self.below(5)); self.draws(1)
    def p_blur_queued(self): self.draws(); self.blur()

    def p_tex_replace(self):
        tex = self.pick(self.tex_sets)
        kind = self.pick(("PHONG", "UPHONG"))
        self.draw(kind=kind, r=1, tex=tex)
        self.upload(self.pick([s for s in tex if s >= 0]))
        self.draw(kind=kind, r=1, tex=tex)

    def p_pfp(self):
        """A shaded flush, a flat flush and a shaded flush over the same pixels (the visibility buffer of the first is stale in the third)."""
        s = self.seed()
        flat = dict(kind="FLAT", n=40, r=1, seed=s, mem="host")
        if self.f in "BE":
            shaded = dict(kind=self.pick(("PHONG", "UPHONG")), n=40, r=1, seed=s, mem="host", tex=self.pick(self.tex_sets))
            self.draw(**shaded); self.op("flush"); self.draw(**flat); self.op("flush"); self.draw(**dict(shaded, seed=s + 1)); self.op("flush")
        else:
            self.indexed(seed=s); self.op("flush"); self.draw(**dict(flat, r=2, n=8)); self.op("flush"); self.indexed(seed=s + 1); self.op("flush")

    def p_mixed_flush(self):
        for kind in ("PHONG", "FLAT", "UPHONG", "GOURAUD"):
            self.draw(kind=kind, r=1)
        self.op("flush")

    def p_single_kind_flush(self):
        kind = self.pick(self.kinds)
        self.draw(kind=kind); self.draw(kind=kind); self.op("flush")

    def p_eye(self): self.draw(kind="EYE", r=1, n=60); self.draws(1)
    def p_strip_change(self): self.draws(); self.change_strip(); self.draws()
    def p_blur_refused(self): self.draws(); self.op("refused", what="blur_in_strip" if self.strip != (0, self.h) else "bad_strip")

    def p_kind_cut(self):
        self.draw(kind=self.pick(("FLAT", "GOURAUD", "CHECKER")), r=1)
        self.draw(kind="UCHECKER", r=1)
        self.draw(kind=self.pick(("FLAT", "GOURAUD", "CHECKER")), r=1)

    def p_burst(self):
        self.op("draw_burst", kind=self.pick(("FLAT", "CHECKER")), count=MAX_DRAWS + 6, seed=self.seed(), r=1, cells=3)
        self.draw(kind="UCHECKER", r=1)

    def mid(self, k):
        """draws, flush_begin, one call, then flush_end, nothing, or a second flush_begin: every entry point completes a begun flush"""
        allowed = [m for m in MID_OPS if not (m == "upload_texture" and self.f not in "BE") and not (m == "clear" and self.f == "S")
                   and not (m == "framebuffer_blur" and self.f in "SE")]
        m = allowed[k % len(allowed)]
        if m == "upload_texture":
            tex = self.tex_sets[0]
            self.draw(kind="PHONG", r=1, tex=tex)
        else:
            self.draws()
        self.op("flush_begin")
        {"draw": lambda: self.draws(1), "set_viewport": self.set_viewport, "upload_texture": lambda: self.upload(0), "clear": self.clear,
         "zbuffer_snapshot": self.snapshot, "framebuffer_blur": self.blur, "set_stream": self.set_stream, "register_shader": self.register_extra,
         "mesh_bounds": lambda: self.op("mesh_bounds", n=30 + self.below(60), seed=self.seed()), "observe": self.observation}[m]()
        tail = self.below(3)
        if tail == 0:
            self.op("flush_end")
        elif tail == 1:
            self.op("flush_begin"); self.op("flush_end")
        if m == "upload_texture":
            self.draw(kind="PHONG", r=1, tex=tex)

    def phrases(self):
        """(the phrases every family may hold, the family's own: its first one goes into every program)"""
        common = [self.p_vp_diff, self.p_vp_same, self.p_init_vp, self.p_write_queued, self.p_reset_queued, self.p_snapshot_restore,
                  self.p_postprocess_queued, self.p_refused_queued, self.p_zero_draw, self.p_begin_twice, self.p_end_alone, self.p_stream,
                  self.p_dev_draw]
        if self.f != "S":
            common += [self.p_clear_queued, self.p_clear_only_flush, self.p_write_over_clear]
        return common, {"A": [self.p_pfp, self.p_single_kind_flush, self.p_indexed, self.p_blur_queued],
                        "B": [self.p_tex_replace, self.p_pfp, self.p_mixed_flush, self.p_single_kind_flush, self.p_indexed, self.p_blur_queued],
                        "E": [self.p_tex_replace, self.p_pfp, self.p_mixed_flush, self.p_indexed],
                        "S": [self.p_strip_change, self.p_blur_refused, self.p_indexed],
                        "D": [self.p_kind_cut, self.p_burst, self.p_indexed, self.p_blur_queued]}[self.f]


def generate(family, seed):
    """The program of (family, seed)."""
    g = _Gen(family, seed)
    if family == "S":                       # no clear in this family: trgl.h leaves the rows outside a strip unspecified after one
        g.op("write_framebuffer", v=0); g.op("write_zbuffer", v=0)
        g.change_strip()
    if family in "BE":
        for slot, bpp in enumerate((3, 3, 1, 1, 4, 4)):
            g.upload(slot, bpp)
    if family == "E":
        g.p_eye()
    common, specific = g.phrases()
    # the family's first phrase always, one more of its own in turn, and three of the common ones in turn
    chosen = [specific[0], specific[1 + seed % (len(specific) - 1)]] + [common[(seed * 3 + k) % len(common)] for k in range(3)]
    take = len(chosen)
    order = np.argsort(g.r.u64(take), kind="stable")
    mids = [3 * (seed + 8 * FAMILIES.index(family)) + k for k in range(3)]
    for k, i in enumerate(order):
        chosen[i]()
        if g.below(3) == 0:
            g.observation()                 # (between phrases: nothing is queued on purpose here, it only narrows down a failure)
        if k < 3:
            g.mid(mids[k])
    if g.torch_stream:
        g.set_stream()
    if g.below(2):
        g.postprocess()
    g.op("observe")
    return Program(family, seed, g.w, g.h, g.bpp, g.ops)


# ---- what a deferred implementation holds at each point of a program: the hazards a program contains ----------------------------
class _Shadow:
    """Follows the queue of draws, a begun flush and a pending clear through a program by the rules of trgl_api.cpp, and notes each
    hazard (name, operation index) at which a rule of that file is what keeps the frame right.  `live`: a queued draw put fragments
    into the model's frame, so running it late or under another state shows."""

    def __init__(self):
        self.queued, self.begun, self.clear_pending = [], False, False
        self.events, self.flushes, self.stale = [], "", set()

    def hit(self, name, i):
        self.events.append((name, i))

    def live(self):
        return any(d["frags"] for d in self.queued)

    def raster(self, i):
        drawn = [d for d in self.queued if d["frags"]]
        if drawn:
            self.flushes += "P" if any(d["idbuf"] for d in drawn) else "F"
            if self.flushes.endswith("PFP"):
                self.hit("phong_flat_phong", i)
        self.queued, self.begun, self.clear_pending = [], False, False

    def end_begun(self, i):
        if self.begun:
            self.raster(i)

    def flush_queued(self, i):
        if self.queued:
            self.raster(i)

    def before(self, i, name, a, different_viewport=False):
        """The bookkeeping of operation i, ahead of the model's own execution of it."""
        q = bool(self.queued) and self.live() and not self.begun
        if self.begun and self.live():
            m = "observe" if name in OBSERVATIONS else "draw" if name in ("draw_indexed", "draw_burst") else name
            if m in MID_OPS:
                self.hit("mid_" + m, i)
        if name in ("draw", "draw_indexed", "draw_burst"):
            self.end_begun(i)
        elif name == "set_viewport":
            if q:
                self.hit("vp_diff_queued" if different_viewport else "vp_same_queued", i)
            self.end_begun(i)
            if different_viewport:
                self.flush_queued(i)
        elif name == "init_viewport":
            if q:
                self.hit("init_vp_queued", i)
            if self.queued:
                self.end_begun(i)
                if different_viewport:
                    self.flush_queued(i)
        elif name == "upload_texture":
            if q and any(d["frags"] and a["slot"] in d["tex"] for d in self.queued):
                self.hit("tex_replace_queued", i)
                self.stale.add(a["slot"])
            self.end_begun(i)
            self.flush_queued(i)
        elif name == "clear":
            if q:
                self.hit("clear_queued", i)
            self.end_begun(i)
            self.flush_queued(i)
            self.clear_pending = True
        elif name in ("flush", "flush_end"):
            if name == "flush" or self.begun:
                if self.clear_pending and not self.queued:
                    self.hit("clear_only_flush", i)
                self.raster(i)
        elif name == "flush_begin":
            self.begun = self.begun or bool(self.queued) or self.clear_pending
        elif name == "sync":
            self.end_begun(i)
        elif name in ("write_framebuffer", "write_zbuffer"):
            if self.clear_pending:
                self.hit("write_over_clear", i)
            if q:
                self.hit("write_queued", i)
            self.raster(i)
        elif name in ("reset_stats", "postprocess", "zbuffer_snapshot", "zbuffer_restore", "framebuffer_blur"):
            if q:
                self.hit(name.replace("zbuffer_", "").replace("framebuffer_", "") + "_queued", i)
            self.raster(i)
        elif name in OBSERVATIONS:
            self.raster(i)
        elif name == "set_stream":
            self.end_begun(i)
            self.flush_queued(i)
        elif name == "refused":
            if q:
                self.hit("refused_queued", i)
            if a["what"] in ("unknown_kind", "bad_strip"):
                self.end_begun(i)
        elif name in ("set_strip", "set_interleave"):
            if q:
                self.hit("strip_queued", i)
            self.end_begun(i)
            self.flush_queued(i)

    def queue(self, i, kind, frags, tex, scribbled, indexed):
        """A draw of `frags` fragments (in the model) joins the queue."""
        base, source, _, may_discard = KINDS[kind]
        if self.queued and self.queued[-1]["kind"] != kind and (may_discard or self.queued[-1]["discards"]):
            if self.live() or frags:
                self.hit("kind_cut", i)
            self.raster(i)
        if len(self.queued) >= MAX_DRAWS:
            if self.live():
                self.hit("max_draws", i)
            self.raster(i)
        self.queued.append(dict(kind=kind, frags=frags, tex=tuple(tex), discards=may_discard,
                                idbuf=base in SHADED or (source is not None and not may_discard)))
        if frags and scribbled:
            self.hit("scribble_indexed" if indexed else "scribble_draw", i)
        if frags and self.stale & set(tex):
            self.hit("tex_replace_sampled", i)
            self.stale -= set(tex)


# ---- the immediate interpreter ---------------------------------------------------------------------------------------------
def _orc_uniforms(u):
    from oracle import orc
    return None if u is None else orc.Uniforms.from_buffer_copy(bytes(u))


def run_model(program, lazy_scribble=None, shadow=None):
    """Execute the program at once, as the reference would: every call takes effect where it stands.  Returns the observations:
    (tag, operation index, eye, payload...) with tags 'fb', 'z', 'stats', 'frame', 'post' and 'bounds'.  lazy_scribble = i: the
    scribble of operation i happens BEFORE its draw (what an implementation that reads the caller's arrays late would render).
    shadow: a _Shadow that collects the hazards of the program."""
    from oracle import orc
    p = program
    o = orc.Oracle(p.w, p.h, p.bpp)
    sh = shadow or _Shadow()
    obs, snaps, eye = [], {}, False
    rect = (0, 0, p.w, p.h)

    def frags():
        return o.stats[1]

    def draw(i, a, indexed=False):
        nonlocal eye
        base = KINDS[a["kind"]][0]
        before = frags()
        if indexed:
            verts, idx, u, proj = mesh_arrays(p, a)
            if lazy_scribble == i:
                scribble_mesh(verts, idx, u, proj)
            clip, vary = orc.vertex_stage(np.array(u.model_view).reshape(4, 4), proj, verts, idx)
            col = None
        else:
            clip, vary, col, u = draw_arrays(p, a)
            if lazy_scribble == i:
                scribble_draw(p, a, clip, vary, col, u)
        if clip.shape[0]:
            o.draw(base, clip, vary, col, _orc_uniforms(u))
            eye = eye or base == EYE
        sh.queue(i, a["kind"], frags() - before, a.get("tex", ()), bool(a.get("scr")), indexed)

    for i, (name, a) in enumerate(p.ops):
        if name in ("set_viewport", "init_viewport"):
            sh.before(i, name, a, different_viewport=tuple(a["rect"]) != rect)
            rect = tuple(a["rect"])
            o.set_viewport(scenes.init_viewport(*rect))
            continue
        sh.before(i, name, a)
        if name == "draw":
            if a["n"] == 0:
                sh.hit("zero_draw", i)
            else:
                draw(i, a)
        elif name == "draw_indexed":
            draw(i, a, indexed=True)
        elif name == "draw_burst":
            for b in burst_ops(a):
                draw(i, b)
        elif name == "upload_texture":
            o.upload_texture(a["slot"], texels(a))
        elif name == "clear":
            o.clear(a["bgra"], a["z"])
        elif name == "write_framebuffer":
            o.fb[:] = written_fb(p, a)
        elif name == "write_zbuffer":
            o.z[:] = written_z(p, a)
        elif name == "reset_stats":
            o.reset_stats()
        elif name == "zbuffer_snapshot":
            snaps[a["slot"]] = o.z.copy()
        elif name == "zbuffer_restore":
            o.z[:] = snaps[a["slot"]]
        elif name == "framebuffer_blur":
            o.fb[:] = image_ops_model.gaussian_blur(o.fb, api.gaussian_kernel(a["r"]))
        elif name == "set_strip":
            o.set_strip(a["y0"], a["y1"])
        elif name == "set_interleave":
            assert a["world"] == 1
            o.set_strip(0, p.h)
        elif name == "read_fb":
            obs.append(("fb", i, eye, o.fb.copy()))
        elif name == "read_z":
            obs.append(("z", i, eye, o.z.copy()))
        elif name == "stats":
            obs.append(("stats", i, eye, o.stats, orc.format_stats_line(o.stats)))
        elif name == "observe":
            obs.append(("frame", i, eye, o.fb.copy(), o.z.copy(), o.stats, orc.format_stats_line(o.stats)))
        elif name == "postprocess":
            ao = orc.ssao(o.z)
            fin = orc.composite(np.ascontiguousarray(o.fb[:, :, :3]), ao) if a["final"] else None
            obs.append(("post", i, eye, orc.zbuffer_image(o.z), ao, fin))
        elif name == "mesh_bounds":
            v = bounds_mesh(a)[:, :3]
            lo, hi = v.min(0), v.max(0)
            margin = (hi - lo) * 0.01                           # model.cpp:35-36
            obs.append(("bounds", i, eye, lo - margin, hi + margin))
        else:
            assert name in ("flush", "flush_begin", "flush_end", "sync", "set_stream", "register_shader", "refused"), name
    return obs


def hazards(program):
    """[(hazard name, operation index)] of a program, from a run of the model."""
    sh = _Shadow()
    run_model(program, shadow=sh)
    return sh.events


# ---- the interpreter over the C ABI ----------------------------------------------------------------------------------------
def run_gpu(program):
    """Execute the program on one Context; the observations in run_model's form (eye left False).  Device arrays stay alive until
    the context is closed and are never scribbled; host arrays are scribbled right after the draw that took them returns."""
    import torch
    p = program
    obs, keep, kinds = [], [], {}
    streams = []
    ctx = api.Context(p.w, p.h, p.bpp)
    try:
        def draw(a):
            clip, vary, col, u = draw_arrays(p, a)
            kind = kinds[a["kind"]] if KINDS[a["kind"]][1] is not None else KINDS[a["kind"]][0]
            if a["mem"] == "dev":
                dev = tuple(None if x is None else cases.device_array(x) for x in (clip, vary, col))
                torch.cuda.synchronize()                        # the uploads ran on torch's stream, which the context's does not follow
                keep.append(dev)
                ctx.draw(kind, dev[0], dev[1], dev[2], u, device=True)
            else:
                ctx.draw(kind, clip, vary, col, u)
                if a["scr"]:
                    scribble_draw(p, a, clip, vary, col, u)

        for i, (name, a) in enumerate(p.ops):
            if name == "draw":
                draw(a)
            elif name == "draw_burst":
                for b in burst_ops(a):
                    draw(b)
            elif name == "draw_indexed":
                verts, idx, u, proj = mesh_arrays(p, a)
                if a["mem"] == "dev":
                    dev = (cases.device_array(verts), cases.device_array(idx))
                    torch.cuda.synchronize()
                    keep.append(dev)
                    ctx.draw_indexed(KINDS[a["kind"]][0], u, proj, dev[0], dev[1], device=True)
                else:
                    ctx.draw_indexed(KINDS[a["kind"]][0], u, proj, verts, idx)
                    if a["scr"]:
                        scribble_mesh(verts, idx, u, proj)
            elif name == "register_shader":
                source, K, may_discard = (KINDS[a["src"]][1:] if a["src"] in KINDS else EXTRA_SOURCES[a["src"]])
                kinds[a["src"]] = ctx.register_shader(source, K, may_discard)
            elif name == "set_viewport":
                ctx.set_viewport(scenes.init_viewport(*a["rect"]))
            elif name == "init_viewport":
                ctx.init_viewport(*a["rect"])
            elif name == "upload_texture":
                ctx.upload_texture(a["slot"], texels(a))
            elif name == "clear":
                ctx.clear(a["bgra"], a["z"])
            elif name == "write_framebuffer":
                ctx.write_framebuffer(written_fb(p, a))
            elif name == "write_zbuffer":
                ctx.write_zbuffer(written_z(p, a))
            elif name in ("reset_stats", "flush", "flush_begin", "flush_end", "sync"):
                getattr(ctx, name)()
            elif name in ("zbuffer_snapshot", "zbuffer_restore"):
                getattr(ctx, name)(a["slot"])
            elif name == "framebuffer_blur":
                ctx.framebuffer_blur(a["r"])
            elif name == "set_strip":
                ctx.set_strip(a["y0"], a["y1"])
            elif name == "set_interleave":
                ctx.set_interleave(a["band"], a["rank"], a["world"])
            elif name == "set_stream":
                if a["to"] == "torch":
                    streams.append(torch.cuda.Stream())
                    ctx.set_stream(streams[-1].cuda_stream)
                else:
                    ctx.set_stream(0, use_own=True)
            elif name == "refused":
                if a["what"] == "unknown_kind":
                    clip = draw_arrays(p, dict(kind="FLAT", n=5, seed=1, r=1))[0]
                    rc, want = ctx.L.trgl_draw(ctx.h, api.SHADER_USER_FIRST + api.MAX_USER_SHADERS - 1, None, clip.ctypes.data, None, None, 5, api.MEM_HOST), E_INVALID
                elif a["what"] == "bad_strip":
                    rc, want = ctx.L.trgl_set_strip(ctx.h, 5, 3), E_INVALID
                elif a["what"] == "blur_in_strip":
                    rc, want = ctx.L.trgl_framebuffer_blur(ctx.h, 2), E_STATE
                else:
                    rc, want = ctx.L.trgl_zbuffer_restore(ctx.h, api.MAX_Z_SNAPSHOTS - 1), E_STATE
                assert rc == want, f"operation {i} ({a['what']}): return code {rc}, expected {want}\n{p.text(i + 1)}"
            elif name == "read_fb":
                obs.append(("fb", i, False, ctx.read_framebuffer()))
            elif name == "read_z":
                obs.append(("z", i, False, ctx.read_zbuffer()))
            elif name == "stats":
                obs.append(("stats", i, False, ctx.stats(), ctx.stats_line()))
            elif name == "observe":
                obs.append(("frame", i, False, ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()))
            elif name == "postprocess":
                out = ctx.postprocess(final=bool(a["final"]))
                obs.append(("post", i, False, out["zbuffer_image"], out["ao"], out["final"]))
            elif name == "mesh_bounds":
                obs.append(("bounds", i, False) + tuple(ctx.mesh_bounds(bounds_mesh(a))))
            else:
                raise AssertionError(f"unknown operation {name}")
    finally:
        ctx.close()             # waits for the stream in use; only then may the device arrays and the torch streams go
        del keep, streams
    return obs


# ---- comparison --------------------------------------------------------------------------------------------------------------
def _same(got, want, eye):
    tag = want[0]
    assert got[0] == tag and got[1] == want[1], (got[:2], want[:2])
    if tag == "fb":
        zero = np.zeros(want[3].shape[:2])
        cases.assert_same_frame((got[3], zero, None), (want[3], zero, None), eye=eye, stats=False, what="read_framebuffer")
    elif tag == "z":
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)), "read_zbuffer: z bits differ"
    elif tag == "stats":
        assert got[3:] == want[3:], f"stats {got[3:]} != {want[3:]}"
    elif tag == "frame":
        cases.assert_same_frame(got[3:], want[3:], eye=eye)
    elif tag == "post":
        for what, g, w in zip(("zbuffer_image", "ao", "final"), got[3:], want[3:]):
            assert (g is None) == (w is None) and (w is None or np.array_equal(g, w)), f"postprocess: {what} differs"
    else:
        assert all(np.array_equal(g.view(np.uint64), w.view(np.uint64)) for g, w in zip(got[3:], want[3:])), f"{tag}: {got[3:]} != {want[3:]}"


def differs(got, want):
    """Whether two observations of the model differ at all (bit for bit)."""
    try:
        _same(got, want, False)
    except AssertionError:
        return True
    return False


def assert_same(program, got, want):
    """Every observation of `got` (run_gpu) equals that of `want` (run_model); in family E, after the first EYE draw, framebuffer
    bytes by the EYE rule of cases.assert_same_frame.  The message names the seed, the first differing observation and the program
    up to it."""
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        try:
            _same(g, w, eye=w[2] and program.family == "E")
        except AssertionError as e:
            raise AssertionError(f"family {program.family} seed {program.seed}: observation {k} ({w[0]} at operation {w[1]}) differs: {e}\n"
                                 f"{program.text(w[1] + 1)}") from None


def simple_case(program):
    """The cases.make_case dict of a program that is only state (set_viewport, upload_texture, clear), then draws, then one observe."""
    p = program
    vp, tex, clear, zclear, draws = scenes.init_viewport(0, 0, p.w, p.h), {}, cases.DEFAULT_CLEAR, np.inf, []
    for name, a in p.ops:
        if name == "set_viewport":
            vp = scenes.init_viewport(*a["rect"])
        elif name == "upload_texture":
            tex[a["slot"]] = texels(a)
        elif name == "clear":
            clear, zclear = a["bgra"], a["z"]
        elif name == "draw":
            clip, vary, col, u = draw_arrays(p, a)
            draws.append((KINDS[a["kind"]][0], u, clip, vary, col))
        else:
            assert name == "observe", name
    return cases.make_case(p.w, p.h, draws, bpp=p.bpp, viewport=vp, textures=tex, clear=clear, zclear=zclear)
