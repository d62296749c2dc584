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
D a discarding user kind between other kinds, T translucent kinds (in.dst, the depth-write mask) over every way a frame comes to be
resident, P the passes over the resident frame and its depth snapshots (occlusion codes, shadow masks, modulate), I instanced draws,
their culling and ordering chain in device memory, and clipped draws.

Families P and I keep arrays in named *registers* (`array reg=...`, or `instances` for the arrays of one instanced call): a register is a host array or a device tensor, the passes read
and write registers, and `read_reg` observes one.  A register in device memory is read by the library when the stream gets there, so
the program alone decides what a queued call sees."""
import collections
import ctypes as C
import os
import re

import numpy as np

import blend_model as B
import cases
import clip_model
import discard_shader_sources as DS
import image_ops_model
import instance_cull_cases as CC
import instance_model as IM
import instanced_cases as IC
import occlusion_model
import order_cases as OC
import order_model
import scene_model
import shadow_model
import user_shader_sources as US
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, GOURAUD, PHONG, EYE, CHECKER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLUR_LDS_RADIUS = int(re.search(r"constexpr int BLUR_LDS_RADIUS = (\d+);",
                                open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()).group(1))
MAX_DRAWS = int(re.search(r"#define TRGL_MAX_DRAWS (\d+)",
                          open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "trgl_device.h")).read()).group(1))
E_INVALID, E_STATE = -1, -4

FAMILIES = "ABESDTPI"
SEEDS = {f: tuple(range(8)) for f in FAMILIES}          # the committed seed list: tests/test_call_programs.py proves what it can notice

# kind name -> (the built-in kind the model renders it as, the source a context registers for it, K, may_discard)
KINDS = {"FLAT": (FLAT, None, 0, False), "GOURAUD": (GOURAUD, None, 3, False), "CHECKER": (CHECKER, None, 0, False),
         "PHONG": (PHONG, None, 24, False), "EYE": (EYE, None, 24, False),
         "UFLAT": (FLAT, US.FLAT, 0, False), "UGOURAUD": (GOURAUD, US.GOURAUD, 3, False), "UPHONG": (PHONG, US.PHONG, 24, False),
         "UCHECKER": (CHECKER, DS.CHECKER, 0, True),
         # translucent kinds (MAY_DISCARD | READS_DEST): the model renders them by blend_model's per-triangle scheme, BLEND
         "TOVER": (FLAT, B.OVER_SRC, 0, True), "TOVER_ND": (FLAT, B.OVER_SRC, 0, True), "TADD": (FLAT, B.ADD_SRC, 0, True)}
# translucent kind -> (blend_model's restatement of its shader, whether a drawn fragment writes the depth)
BLEND = {"TOVER": (B.f_over, True), "TOVER_ND": (B.f_over, False), "TADD": (B.f_add, True)}
# vertex stages of the instanced calls: None is the built-in one (K = 24); "k0" adds the record's first three doubles to the position,
# "quad" the translation of the record's row-major matrix (the records trgl_instance_depths and trgl_instance_boxes read)
VERTEX_STAGES = {"builtin": None, "k0": IC.STAGES["k0"], "quad": (OC.QUAD_VS, 0)}
PLANES = {"near": clip_model.NEAR, "slant": (1.0, 0.0, 0.0, 0.2), "dropall": (0.0, 0.0, 0.0, -1.0)}      # dropall: d = -w < 0 everywhere
INST_BLOCK = int(re.search(r"constexpr int INST_BLOCK = (\d+);", open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()).group(1))
FRUSTUM_TOP = 3                                         # Frustum::PlaneIndex (our_gl.h:71-78): LEFT, RIGHT, BOTTOM, TOP, NEAR, FAR
# (mesh memory, instance memory, visibility bytes or not - they are where the instances are -, order memory or None): what the header
# allows an instanced call.  The phrases that leave them open take them in turn (a stride of 7 spreads neighbours over the seeds)
MEMORY_COMBOS = [(m, i, v, o) for m in ("host", "dev") for i in ("host", "dev") for v in (False, True) for o in (None, "host", "dev")]
FREE_COMBOS = [MEMORY_COMBOS[7 * k % 24] for k in range(24)]
# where each committed seed of family I enters FREE_COMBOS: found by search so that the eight programs together hold all 24
# (tests/test_call_programs.py asserts it; a change to the phrases of family I needs a new search)
COMBO_START = (9, 2, 8, 3, 16, 22, 20, 21)
LOCAL_BOX = {"cube": (-0.5, -0.5, -0.5, 0.5, 0.5, 0.5), "quad": (-0.3, -0.3, 0.0, 0.3, 0.3, 0.0)}
SHADOW_BIAS, SHADOW_DARKNESS = 1e-3, 0.5
# sources that register_shader adds while draws are queued and that nothing draws
EXTRA_SOURCES = {"XGOURAUD_PADDED": (US.GOURAUD_PADDED, 5, False), "XEYE": (US.EYE, 24, False), "XCHECKER_B": (DS.CHECKER_B, 0, True),
                 "XDISCARD_ALL": (DS.DISCARD_ALL, 0, True)}
SHADED = (PHONG, EYE)                                   # kinds with uniforms, textures and 24 varyings
RADII = ((1, 8, 300), (4, 40, 120), (30, 160, 10))     # classes of a draw's triangles: rmin, rmax, most triangles
FRAMES = ((96, 64), (101, 67), (160, 128))
# operations that make a deferred implementation run what is queued (where a lazily applied state change would land)
FLUSH_POINTS = {"flush", "flush_begin", "flush_end", "read_fb", "read_z", "stats", "observe", "postprocess", "write_framebuffer",
                "write_zbuffer", "zbuffer_snapshot", "zbuffer_restore", "framebuffer_blur", "clear", "reset_stats", "upload_texture",
                "set_strip", "set_interleave", "set_stream", "set_viewport", "init_viewport", "occlusion_boxes", "shadow_mask",
                "framebuffer_modulate"}
OBSERVATIONS = {"read_fb", "read_z", "stats", "observe", "postprocess"}
# device calls that are queued on the stream and touch nothing else: no flush, not even the second half of a begun one
QUIET_OPS = ("instance_boxes", "frustum_boxes", "instance_depths", "depth_order")
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
    clip = shifted(clip, a)
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


def shifted(clip, a):
    """The clip rows of a draw with `zoff` tenths added to every vertex's z / w: the same triangles, further from the eye."""
    if a.get("zoff"):
        clip = clip.copy()
        clip[:, 2::4] += (a["zoff"] / 10.0) * clip[:, 3::4]
    return clip


Camera = collections.namedtuple("Camera", "model_view projection view_proj planes key fill rim")
_cameras = {}


def camera(p):
    """The camera of the instanced calls of a program (shared, do not write to it): matrices, view_proj [16], frustum planes [6, 4] and
    the light directions of its uniform block."""
    if (p.w, p.h) not in _cameras:
        hd = scenes.head_standin(1, p.w, p.h)
        # (near and far planes close around the instances: their depths spread over the range the triangle soups and the clears use)
        mv, proj = np.ascontiguousarray(hd["model_view"], np.float64), np.ascontiguousarray(scenes.perspective(scenes.TAN_35DEG, p.w / p.h, 1.2, 4.5))
        view_proj = IM.mat_product(proj, mv).reshape(16)
        # Frustum::createFromMatrix wants the transpose of a matrix that multiplies column vectors (instance_cull_cases.cull_scene)
        _cameras[p.w, p.h] = Camera(mv, proj, view_proj, scene_model.frustum_from_matrix(view_proj.reshape(4, 4).T), hd["key"], hd["fill"], hd["rim"])
    return _cameras[p.w, p.h]


def mesh_of(name):
    """(vertices [nv, 8], indices [nf, 3], one colour per face) of 'cube' (12 faces) or 'quad' (2 faces): fresh arrays."""
    verts, idx = IC.cube(8, 0.5) if name == "cube" else OC.quad(0.3)
    return verts, idx, IC.colors(idx.shape[0], 7, alpha=True)


def reject_planes():
    """Six planes of which one rejects every box: a zero normal with d = -1."""
    planes = np.tile(np.array(CC.ACCEPT, np.float64), (6, 1))
    planes[FRUSTUM_TOP] = 0.0, 0.0, 0.0, -1.0
    return planes


def array_of(p, a):
    """The numpy array an `array` (or `dev_copy`) operation stands for, by its `what`."""
    what, n, seed = a["what"], a["n"], a["seed"]
    if what == "inst":                                  # row-major matrices, then extras
        return IC.instances(n, a["stride"], seed=seed, spread=0.9, scale=(0.15, 0.4))
    if what == "icol":
        return IC.colors(n, seed, alpha=True)
    if what == "vis":
        return IC.visible(a["pattern"], n, seed)
    if what == "order":                                 # a shuffle of 0..n-1 with its first entries once more at the end
        o = np.argsort(scenes.SplitMix64(seed).u64(n), kind="stable").astype(np.uint32)
        o = np.concatenate([o, o[:min(3, n)]])
        if a.get("bad"):
            o[len(o) // 2] = n                          # not an instance: a host list with it is refused
        return o
    if what == "boxes":                                 # boxes in NDC (the occlusion query runs under the identity) around the frame
        r = scenes.SplitMix64(seed)
        c = np.stack([r.uniform(n, -1.1, 1.1), r.uniform(n, -1.1, 1.1), r.uniform(n, -1.6, 1.6)], 1)
        half = np.stack([r.uniform(n, 0.01, 0.1), r.uniform(n, 0.01, 0.1), r.uniform(n, 0.01, 0.3)], 1)
        b = np.concatenate([c - half, c + half], 1)
        b[0, [2, 5]] = 2.5, 3.0                         # behind the far plane: OUTSIDE whatever the depths are
        return np.ascontiguousarray(b)
    assert what == "mask", what
    return (scenes.SplitMix64(seed).u64(p.w * p.h) >> np.uint64(23)).astype(np.uint8).reshape(p.h, p.w)


def arrays_of(name, a):
    """The `array` operations an operation stands for: itself, or for `instances` the arrays of one instanced call - the records, and
    where it names them colours, visibility bytes (where the records are) and an order list (in memory of its own)."""
    if name == "array":
        return [a]
    if name != "instances":
        return []
    out = [dict(reg=a["reg"], what="inst", mem=a["mem"], n=a["n"], seed=a["seed"], stride=a["stride"])]
    if a["col"] != "none":
        out.append(dict(reg=a["col"], what="icol", mem=a["mem"], n=a["n"], seed=a["seed"] + 1))
    if a["vis"] != "none":
        out.append(dict(reg=a["vis"], what="vis", mem=a["mem"], n=a["n"], seed=a["seed"] + 2, pattern=a["pattern"]))
    if a["ord"] != "none":
        out.append(dict(reg=a["ord"], what="order", mem=a["omem"], n=a["n"], seed=a["seed"] + 3))
    return out


def scribble_reg(x, what):
    """Other valid contents of the same kind, in place: what a caller may put into a host array once the call that took it has returned."""
    if what == "mask":
        x[:] = ~x
    elif what in ("vis", "codes"):
        x[:] = x ^ 1
    elif what == "icol":
        x[:] = ~x
    else:                                               # instances, or an order list: the same entries, backwards
        assert what in ("inst", "order"), what
        x[:] = x[::-1].copy()


def shadow_params_of(a):
    """(screen_to_light [4, 4], pcf radius): the light's map is the frame, moved by a few pixels."""
    m = np.eye(4)
    m[0, 3], m[1, 3] = a["dx"], a["dy"]
    return m, a["r"]


def instanced_rows(p, a, verts, idx, fcol, inst, icol, vis, order, order_device):
    """(clip, varyings or None, colours or None, number of drawn instances) of an instanced call, as include/trgl.h defines the loop."""
    cam = camera(p)
    mv, proj, key = cam.model_view, cam.projection, cam.key
    n = a["n"]
    if order is None:
        drawn = IM.compact(vis, n)
    else:
        drawn = order_model.visit(order, n, vis, skip_out_of_range=order_device)
    nf = idx.shape[0]
    if a["vs"] == "builtin":
        clip, vary, _ = IM.builtin_rows(mv, proj, verts, idx, inst[drawn], None)
    else:
        rec = inst if a["vs"] == "k0" else inst[:, [3, 7, 11]]
        clip, vary = IC.expect_user("k0", mv, proj, key, verts, idx, rec, np.asarray(drawn, np.int64))
    return clip, vary, IM.colors(np.asarray(drawn, np.int64), nf, fcol, icol), len(drawn)


def blend_draw(o, clip, colors, fn, depth_write):
    """blend_model.Model's per-triangle scheme on the oracle `o`: the triangle FLAT, the pixels whose depth bits changed are its
    z-passes; dst is the frame before it masked to bpp bytes, the frame gets bpp bytes of fn(src, dst), and with depth writes off
    the depths go back.  (The kinds of BLEND never discard, so the oracle's own counters are the frame's.)  Returns the mask of
    pixels the draw wrote and whether a triangle of it wrote over an earlier one of the same draw."""
    touched, self_overlap = np.zeros((o.h, o.w), bool), False
    keep = np.uint32(0xffffffff >> (8 * (4 - o.bpp)))
    for i in range(clip.shape[0]):
        z0, fb0 = o.z.copy(), o.fb.copy()
        o.draw(FLAT, clip[i:i + 1], None, colors[i:i + 1])
        ys, xs = np.nonzero(o.z.view(np.uint64) != z0.view(np.uint64))
        if ys.size:
            dst = np.zeros(ys.shape, np.uint32)
            for b in range(o.bpp):
                dst |= fb0[ys, xs, b].astype(np.uint32) << np.uint32(8 * b)
            discard, out = fn(np.full(ys.shape, colors[i], np.uint32), dst & keep)
            assert not discard.any()
            for b in range(o.bpp):
                o.fb[ys, xs, b] = (out.astype(np.uint32) >> np.uint32(8 * b)).astype(np.uint8)
            self_overlap = self_overlap or bool(touched[ys, xs].any())
            touched[ys, xs] = True
        if not depth_write:
            o.z[:] = z0
    return touched, self_overlap


# ---- the generator --------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, family, seed):
        self.f, self.s = family, seed
        self.r = scenes.SplitMix64(0xCA11 + 1000 * FAMILIES.index(family) + seed)
        self.w, self.h = FRAMES[1 + seed % 2] if family == "S" else FRAMES[seed % 3]
        self.bpp = (1, 3, 4)[(seed // 3 + seed) % 3] if family in "AST" else (3, 4)[seed % 2]
        self.ops, self.registered, self.extra = [], set(), list(EXTRA_SOURCES)
        self.rect = (0, 0, self.w, self.h)
        self.strip = (0, self.h)
        self.next_seed = 7000 + 500 * seed + 100000 * FAMILIES.index(family)
        self.snapped = set()
        self.torch_stream = False
        self.kinds = {"A": ("FLAT", "GOURAUD", "CHECKER", "UFLAT", "UGOURAUD"), "B": ("PHONG", "UPHONG", "FLAT", "GOURAUD"),
                      "E": ("PHONG", "UPHONG", "FLAT", "GOURAUD", "EYE"), "S": ("FLAT", "GOURAUD", "CHECKER", "PHONG"),
                      "D": ("FLAT", "GOURAUD", "CHECKER", "UCHECKER"), "T": ("TOVER", "TOVER_ND", "TADD", "FLAT", "GOURAUD"),
                      "P": ("FLAT", "GOURAUD", "CHECKER"), "I": ("FLAT", "GOURAUD", "CHECKER")}[family]
        self.regs, self.vertex_registered, self.combo = {}, set(), seed
        if family == "I":                   # (its three user sources are taken: the blending kind and two vertex stages)
            self.extra = []
            self.combo = COMBO_START[seed % len(COMBO_START)]
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
    def need_kind(self, kind):
        if KINDS[kind][1] is not None and kind not in self.registered:
            self.registered.add(kind)
            self.op("register_shader", src=kind)

    def draw(self, kind=None, n=None, r=None, mem=None, seed=None, tex=None, scr=None, zoff=None, plane=None):
        kind = kind or self.pick(self.kinds)
        self.need_kind(kind)
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
        if zoff:
            a.update(zoff=zoff)
        if plane:
            a.update(plane=plane)
        self.op("draw", **a)
        return a

    def draws(self, k=None):
        """One or two draws that a deferred implementation holds queued afterwards."""
        for _ in range(k or 1 + self.below(2)):
            self.draw()

    def indexed(self, mem=None, seed=None, plane=None):
        kind = "PHONG" if self.f != "E" or self.below(2) else "EYE"
        mem = mem or ("dev" if self.below(3) == 0 else "host")
        extra = dict(plane=plane) if plane else {}
        self.op("draw_indexed", kind=kind, seed=self.seed() if seed is None else seed, mem=mem, scr=1 if mem == "host" else 0,
                tex=self.pick(self.tex_sets), s=self.pick((0, 5, 10)), **extra)

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
        self.last_snapshot = slot
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
        what += {"P": ["occl_empty_slot", "shadow_empty_slot"], "I": ["inst_bad_order", "inst_k_differs"]}.get(self.f, [])
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

    # -- family T: translucent kinds --
    def tdraw(self, kind=None, **kw):
        return self.draw(kind=kind or self.pick(tuple(BLEND)), **kw)

    def modulate_host(self):
        self.op("framebuffer_modulate", mask="none", seed=self.seed(), scr=1)

    def p_blend_kind_cut(self):
        self.draw(kind=self.pick(("FLAT", "GOURAUD")), r=2, n=8)
        self.tdraw(r=2, n=6)
        self.draw(kind=self.pick(("FLAT", "GOURAUD")), r=1)

    def p_blend_twice(self):
        kind = self.pick(tuple(BLEND))
        self.draw(kind=kind, r=2, n=8); self.draw(kind=kind, r=1, n=90); self.op("flush")

    def p_blend_over_clear(self): self.op("flush"); self.clear(); self.tdraw(r=2, n=6)
    def p_blend_over_written(self): self.op("write_framebuffer", v=1 + self.below(5)); self.tdraw(r=2, n=6); self.op("read_fb")

    def p_blend_over_pass(self):
        self.draws(); self.blur(); self.tdraw(r=2, n=6)
        self.modulate_host(); self.tdraw(r=2, n=6); self.op("read_fb")

    def p_nodepth_then_opaque(self):
        s = self.seed()
        self.draw(kind="TOVER_ND", r=2, n=6, seed=s, mem="host"); self.draw(kind="FLAT", r=2, n=6, seed=s, mem="host", zoff=2)

    def p_blend_begun(self): self.draws(); self.op("flush_begin"); self.tdraw(r=2, n=6); self.op("flush_end")

    def p_blend_restore(self):
        self.draws(1); self.snapshot(); self.tdraw(kind=self.pick(("TOVER", "TADD")), r=2, n=6); self.tdraw(r=1)      # (one layer that writes depths)
        self.op("zbuffer_restore", slot=self.last_snapshot)
        self.draw(kind="FLAT", r=2, n=6); self.op("read_fb")

    # -- registers (families P and I) --
    def reg(self, prefix, **meta):
        name = f"{prefix}{len(self.regs)}"
        self.regs[name] = meta
        return name

    def array(self, what, mem, n=0, **kw):
        name = self.reg(what[0], what=what, mem=mem, n=n)
        self.op("array", reg=name, what=what, mem=mem, n=n, seed=self.seed(), **kw)
        return name

    def mem(self):
        return self.pick(("host", "dev"))

    def read(self, *names):
        self.op("read_reg", regs="+".join(names))

    # -- family P: passes over the resident frame and the snapshots --
    def occl(self, boxes, slot=-1, cmem=None, vp="ndc"):
        out = self.reg("c", what="codes", mem=cmem or self.mem(), n=self.regs[boxes]["n"])
        self.op("occlusion_boxes", slot=slot, boxes=boxes, out=out, cmem=self.regs[out]["mem"], vp=vp)
        return out

    def shadow(self, slot, mem=None):
        out = self.reg("m", what="mask", mem=mem or self.mem(), n=0)
        self.op("shadow_mask", slot=slot, out=out, mem=self.regs[out]["mem"], dx=self.below(7) - 3, dy=self.below(5) - 2, r=self.below(3))
        return out

    def modulate(self, mask):
        self.op("framebuffer_modulate", mask=mask, seed=0, scr=1 if self.regs[mask]["mem"] == "host" else 0)

    def finite_clear(self, z=None):
        self.op("clear", bgra=tuple(self.below(256) for _ in range(4)), z=z or self.pick((0.25, 0.6, 0.9)))

    def cover(self, k=2, zoff=None):
        for _ in range(k):
            self.draw(kind=self.pick(("FLAT", "GOURAUD")), r=2, n=10, zoff=zoff)

    def p_occl_queued(self):
        b = self.array("boxes", self.mem(), 12 + self.below(20))
        self.finite_clear(); self.cover()
        if self.below(2):
            self.op("flush_begin")
        self.read(self.occl(b))

    def p_occl_clear_pending(self):
        b = self.array("boxes", self.mem(), 12 + self.below(20))
        self.cover(1); self.op("flush"); self.finite_clear()
        self.read(self.occl(b))

    def p_occl_snapshot_stale(self):
        b = self.array("boxes", self.mem(), 24 + self.below(16))
        self.finite_clear(); self.cover(1); self.snapshot(); self.cover(3, zoff=-8)       # (nearer than what the snapshot holds)
        self.read(self.occl(b, slot=self.last_snapshot), self.occl(b))

    def p_shadow_queued(self):
        self.finite_clear(); self.cover(); self.snapshot(); self.finite_clear(); self.cover()
        if self.below(2):
            self.op("flush_begin")
        self.read(self.shadow(self.last_snapshot))

    def p_shadow_chain(self):
        self.finite_clear(); self.cover(); self.snapshot(); self.finite_clear(); self.cover()
        m = self.shadow(self.last_snapshot, mem="dev")
        self.op("image_blur", reg=m, r=self.pick((1, 2, 3)))
        self.modulate(m); self.draws(1)

    def p_modulate_queued(self):
        m = self.array("mask", self.mem())
        self.finite_clear(0.9); self.cover()
        if self.below(2):
            self.op("flush_begin")
        self.modulate(m); self.draws(1)

    def p_pass_then_stream(self):
        b = self.array("boxes", "dev", 12 + self.below(20))
        self.finite_clear(); self.cover(); self.snapshot(); self.cover(1)
        c, m = self.occl(b, cmem="dev"), self.shadow(self.last_snapshot, mem="dev")
        self.set_stream()
        self.modulate(m); self.read(c)
        self.set_stream()

    def p_pass_refused(self):
        """Passes refused for an empty slot, then on a strip context (the strip is given up again behind them): the queued draws land."""
        self.cover(1); self.op("refused", what="occl_empty_slot"); self.op("refused", what="shadow_empty_slot")
        self.op("set_strip", y0=8, y1=self.h - 8); self.cover(1)
        self.op("refused", what=self.pick(("occl_in_strip", "shadow_in_strip")))
        self.op("set_interleave", band=32, rank=0, world=1)

    def p_snapshot_free_queued(self):
        b = self.array("boxes", "dev", 12 + self.below(20))
        self.finite_clear(); self.cover(1); self.snapshot(); self.cover(2, zoff=-8)      # (nearer than what the snapshot holds)
        slot = self.last_snapshot
        c = self.occl(b, slot=slot, cmem="dev")
        self.op("zbuffer_snapshot_free", slot=slot)
        self.snapped.discard(slot)
        self.read(c)

    # -- family I: instances and clipping --
    def need_stage(self, vs):
        if vs != "builtin" and vs not in self.vertex_registered:
            self.vertex_registered.add(vs)
            self.op("register_vertex_shader", src=vs)

    def mems(self, ok=lambda t: True):
        """(mesh memory, instance memory, whether the call has visibility bytes, order memory or None) of an instanced call whose
        phrase leaves them open: the next of MEMORY_COMBOS, in turn, that the phrase can take (`ok`)."""
        while True:
            self.combo += 1
            t = FREE_COMBOS[self.combo % len(FREE_COMBOS)]
            if ok(t):
                return t

    def inst_arrays(self, n, mem, colors=True, vis=None, order=None):
        """Registers of an instanced call, made by one `instances` operation: (instances, colours or 'none', visible or 'none', order or
        'none'); vis: a pattern of instanced_cases.visible, order: the memory of the list."""
        i = self.reg("i", what="inst", mem=mem, n=n)
        c = self.reg("i", what="icol", mem=mem, n=n) if colors else "none"
        v = self.reg("v", what="vis", mem=mem, n=n) if vis else "none"
        o = self.reg("o", what="order", mem=order, n=n) if order else "none"
        self.op("instances", reg=i, mem=mem, n=n, stride=self.pick((16, 19)), seed=self.seed(), col=c, vis=v, pattern=vis or "none", ord=o,
                omem=order or "none")
        return i, c, v, o

    def instanced(self, call, regs, n, mmem, vs=None, kind=None, mesh=None, scr=None):
        """A draw_instanced or instance_stage over the registers `regs`; the kind follows the stage (K = 24: PHONG, K = 0: a colour kind)."""
        i, c, v, o = regs
        vs = vs or self.pick(("builtin", "k0", "quad"))
        self.need_stage(vs)
        # (at most 300 triangles per draw: the cube's 12 faces only under few instances, an order list names three of them twice)
        a = dict(vs=vs, mesh=mesh or (self.pick(("cube", "quad")) if n <= 22 else "quad"), mmem=mmem, n=n, inst=i, icol="none" if vs == "builtin" else c,
                 fcol=1 if vs != "builtin" and c == "none" else 0, vis=v, ord=o)
        host = self.regs[i]["mem"] == "host"
        a["scr"] = (self.below(2) if scr is None else scr) if host or mmem == "host" else 0
        if call == "draw_instanced":
            kind = "PHONG" if vs == "builtin" else kind or self.pick(("FLAT", "TOVER_ND", "CHECKER"))
            self.need_kind(kind)
            a = dict(kind=kind, **a)
            if KINDS[kind][0] == CHECKER:
                a.update(cells=2 + self.below(5))
        self.op(call, **a)

    def p_chain_device(self):
        n = 24 + self.below(17)
        i, c, _, _ = self.inst_arrays(n, "dev")
        self.need_kind("TOVER_ND"); self.need_stage("quad")
        self.finite_clear(0.9); self.draw(kind="FLAT", r=1, n=30, mem="host")       # (small triangles: most of the instances stay in sight)
        b = self.reg("b", what="boxes", mem="dev", n=n)
        self.op("instance_boxes", inst=i, mesh="quad", out=b)
        if self.below(2):
            v = self.reg("c", what="codes", mem="dev", n=n)
            self.op("frustum_boxes", boxes=b, codes=v, merge=0, planes="cam")
        else:
            v = self.occl(b, cmem="dev", vp="cam")
            self.draw(kind=self.pick(("FLAT", "GOURAUD")), r=2, n=10, mem="host")     # (host arrays: the interpreter waits for no upload inside the chain)
            self.op("frustum_boxes", boxes=b, codes=v, merge=1, planes="cam")
        d = self.reg("d", what="depths", mem="dev", n=n)
        self.op("instance_depths", inst=i, out=d)
        o = self.reg("o", what="order", mem="dev", n=n)
        self.op("depth_order", depths=d, out=o, dir=0)
        self.instanced("draw_instanced", (i, c, v, o), n, ("host", "dev")[self.s % 2], vs="quad", kind="TOVER_ND", mesh="quad", scr=0)
        self.read(b, v, d, o); self.op("read_fb")

    def p_inst_host_scribbled(self):
        n = 8 + self.below(30)
        mmem, _, vis, omem = self.mems(lambda t: t[1] == "host")
        regs = self.inst_arrays(n, "host", vis=self.pick(("random", "alternating")) if vis else None, order=omem)
        self.finite_clear(0.9); self.draws(1); self.instanced("draw_instanced", regs, n, mmem, scr=1); self.draws(1)

    def p_inst_dev_overwritten(self):
        """A device-memory instanced call, then - before any flush - two of its arrays rewritten in stream order: visible (frustum codes
        SET with rejecting planes) or the order (sorted the other way), and the instances or the colours (a torch copy on the stream the
        context was given)."""
        n = 12 + self.below(28)
        self.combo += 1
        if not self.torch_stream:
            self.set_stream()
        i, c, _, _ = self.inst_arrays(n, "dev")
        self.need_kind("TOVER_ND"); self.need_stage("quad")
        self.finite_clear(0.9); self.draw(kind="FLAT", r=1, n=30, mem="host")       # (small triangles: most of the instances stay in sight)
        if self.combo % 2 == 0:
            b = self.reg("b", what="boxes", mem="dev", n=n)
            self.op("instance_boxes", inst=i, mesh="quad", out=b)
            v = self.reg("c", what="codes", mem="dev", n=n)
            self.op("frustum_boxes", boxes=b, codes=v, merge=0, planes="cam")
            self.instanced("draw_instanced", (i, c, v, "none"), n, "dev", vs="quad", kind="TOVER_ND", mesh="quad")
            self.op("frustum_boxes", boxes=b, codes=v, merge=0, planes="reject")
        else:
            d = self.reg("d", what="depths", mem="dev", n=n)
            self.op("instance_depths", inst=i, out=d)
            o = self.reg("o", what="order", mem="dev", n=n)
            self.op("depth_order", depths=d, out=o, dir=0)
            self.instanced("draw_instanced", (i, c, "none", o), n, "host", vs="quad", kind="TOVER_ND", mesh="quad", scr=0)
            self.op("depth_order", depths=d, out=o, dir=1)
        target = i if self.combo % 4 < 2 else c
        spec = [b for nm, a in self.ops for b in arrays_of(nm, a) if b["reg"] == target][0]
        self.op("dev_copy", **dict(spec, seed=self.seed()))
        self.op("flush")

    def p_inst_two_calls(self):
        n1, n2 = 20 + self.below(20), INST_BLOCK + 1 + self.below(40)
        mmem, _, _, omem = self.mems(lambda t: t[1] == "dev" and t[2])      # (a host list among them: device bytes behind a host list)
        a = self.inst_arrays(n1, "dev", vis="random", colors=False, order=omem)
        b = self.inst_arrays(n2, "dev", vis="alternating", colors=False)
        vs = self.pick(("k0", "quad", "builtin"))
        self.finite_clear(0.9)
        self.instanced("draw_instanced", a, n1, mmem, vs=vs, kind="FLAT", mesh="quad", scr=0)
        self.instanced("draw_instanced", b, n2, "host", vs=vs, kind="FLAT", mesh="quad", scr=0)
        self.op("flush")

    def p_inst_begun(self):
        n = 8 + self.below(30)
        mmem, imem, vis, omem = self.mems()
        regs = self.inst_arrays(n, imem, vis="random" if vis else None, order=omem, colors=self.below(2))
        self.draws(1); self.op("flush_begin")
        self.instanced("draw_instanced", regs, n, mmem)
        self.op("flush_end")

    def p_inst_zero_refused(self):
        """An instanced call whose device bytes draw nothing, then two refused instanced calls, all between queued draws."""
        n = 8 + self.below(30)
        mmem, _, _, omem = self.mems(lambda t: t[1] == "dev" and t[2])
        regs = self.inst_arrays(n, "dev", vis="all0", order=omem, colors=False)
        self.draws(1); self.instanced("draw_instanced", regs, n, mmem); self.draws(1)
        self.op("refused", what="inst_bad_order"); self.op("refused", what="inst_k_differs")

    def p_clip_drops_all_queued(self):
        self.draw(kind="FLAT", r=1, mem="host", scr=1); self.draw(kind="FLAT", r=1, mem="dev", plane="dropall")
        self.draw(kind="FLAT", r=1, mem="host", scr=0); self.op("flush")

    def p_clip_idle_wait(self):
        """Nothing queued: a clipped device draw that drops everything, then a staged draw; then a clipped device draw that waits for
        its count between queued draws of another kind; the clip stage alone."""
        self.op("flush"); self.draw(kind="FLAT", r=1, mem="dev", plane="dropall"); self.draw(kind="FLAT", r=1, mem="host", scr=1)
        self.draw(kind="GOURAUD", r=1)
        self.draw(kind=self.pick(("FLAT", "TOVER", "CHECKER")), r=2, n=10, mem="dev", plane=self.pick(("near", "slant")))
        self.draw(kind="GOURAUD", r=1)
        self.op("clip_stage", kind=self.pick(("FLAT", "GOURAUD")), n=20 + self.below(60), seed=self.seed(), r=2, mem=("host", "dev")[self.s % 2],
                plane=self.pick(("near", "slant")))

    def p_quiet_begun(self):
        n = 8 + self.below(30)
        i, _, _, _ = self.inst_arrays(n, "dev", colors=False)
        self.draws(1); self.op("flush_begin")
        b, v, d, o = (self.reg(x, what=w, mem="dev", n=n) for x, w in (("b", "boxes"), ("c", "codes"), ("d", "depths"), ("o", "order")))
        self.op("instance_boxes", inst=i, mesh="cube", out=b); self.op("frustum_boxes", boxes=b, codes=v, merge=0, planes="cam")
        self.op("instance_depths", inst=i, out=d); self.op("depth_order", depths=d, out=o, dir=self.below(2))
        self.op("flush_end")
        self.read(b, v, d, o)

    def p_stage_rows(self):
        """instance_stage four times, with the next four memory combinations."""
        n = 4 + self.below(20)
        for _ in range(4):
            mmem, imem, vis, omem = self.mems()
            regs = self.inst_arrays(n, imem, vis=self.pick(("random", "first")) if vis else None, order=omem, colors=False)
            self.instanced("instance_stage", regs, n, mmem)

    def p_host_quiet(self):
        """The four quiet calls over host memory (no GPU work), and a clipped indexed draw."""
        n = 8 + self.below(30)
        i, _, _, _ = self.inst_arrays(n, "host", colors=False)
        b, v, d, o = (self.reg(x, what=w, mem="host", n=n) for x, w in (("b", "boxes"), ("c", "codes"), ("d", "depths"), ("o", "order")))
        self.draws(1)
        self.op("instance_boxes", inst=i, mesh="cube", out=b); self.op("frustum_boxes", boxes=b, codes=v, merge=0, planes="cam")
        self.op("instance_depths", inst=i, out=d); self.op("depth_order", depths=d, out=o, dir=self.below(2))
        self.read(b, v, d, o)
        self.indexed(plane=self.pick(("near", "slant")))
        mmem, imem, vis, omem = self.mems()
        self.instanced("draw_instanced", self.inst_arrays(n, imem, vis="random" if vis else None, order=omem, colors=self.below(2)), n, mmem)

    def mid(self, k):
        """draws, flush_begin, one call, then flush_end, nothing, or a second flush_begin: every entry point completes a begun flush"""
        allowed = [m for m in MID_OPS if not (m == "upload_texture" and self.f not in "BET") and not (m == "clear" and self.f == "S")
                   and not (m == "framebuffer_blur" and self.f in "SE")]
        m = allowed[k % len(allowed)]
        if m == "upload_texture" and self.f != "T":
            tex = self.tex_sets[0]
            self.draw(kind="PHONG", r=1, tex=tex)
        elif self.f == "T":                 # (family T: the call stands between two translucent draws - an upload_texture too: none samples it)
            self.tdraw(r=2, n=6)
        else:
            self.draws()
        self.op("flush_begin")
        {"draw": (lambda: self.tdraw(r=1)) if self.f == "T" else (lambda: self.draws(1)), "set_viewport": self.set_viewport, "upload_texture": lambda: self.upload(0), "clear": self.clear,
         "zbuffer_snapshot": self.snapshot, "framebuffer_blur": self.blur, "set_stream": self.set_stream, "register_shader": self.register_extra,
         "mesh_bounds": lambda: self.op("mesh_bounds", n=30 + self.below(60), seed=self.seed()), "observe": self.observation}[m]()
        tail = self.below(3)
        if tail == 0:
            self.op("flush_end")
        elif tail == 1:
            self.op("flush_begin"); self.op("flush_end")
        if m == "upload_texture" and self.f != "T":
            self.draw(kind="PHONG", r=1, tex=tex)
        elif self.f == "T":
            self.tdraw(r=2, n=6)

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
                        "D": [self.p_kind_cut, self.p_burst, self.p_indexed, self.p_blur_queued],
                        "T": [self.p_blend_kind_cut, self.p_blend_twice, self.p_blend_over_clear, self.p_blend_over_written, self.p_blend_over_pass,
                              self.p_nodepth_then_opaque, self.p_blend_begun, self.p_blend_restore],
                        "P": [self.p_shadow_chain, self.p_occl_queued, self.p_occl_clear_pending, self.p_occl_snapshot_stale, self.p_shadow_queued,
                              self.p_modulate_queued, self.p_pass_then_stream, self.p_pass_refused, self.p_snapshot_free_queued],
                        "I": [self.p_chain_device, self.p_inst_host_scribbled, self.p_inst_dev_overwritten, self.p_inst_two_calls, self.p_inst_begun,
                              self.p_inst_zero_refused, self.p_clip_drops_all_queued, self.p_clip_idle_wait, self.p_quiet_begun,
                              self.p_stage_rows, self.p_host_quiet]}[self.f]


# families T, P and I: (phrases of the family's own besides its first, common phrases, calls inside a begun flush) of one program
NEW_FAMILY_SHAPE = {"T": (3, 2, 5), "P": (3, 1, 2), "I": (4, 0, 1)}


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
    mids = [3 * (seed + 8 * FAMILIES.index(family)) + k for k in range(3)]
    if family in NEW_FAMILY_SHAPE:          # more of the family's own, so that each of its phrases comes three times over eight seeds
        own, shared, n_mid = NEW_FAMILY_SHAPE[family]
        chosen = [specific[0]] + [specific[1 + (seed * own + k) % (len(specific) - 1)] for k in range(own)] + \
                 [common[(seed * 3 + k) % len(common)] for k in range(shared)]
        mids = [n_mid * seed + k for k in range(n_mid)]
    take = len(chosen)
    order = np.argsort(g.r.u64(take), kind="stable")
    for k, i in enumerate(order):
        chosen[i]()
        if g.below(3) == 0:
            g.observation()                 # (between phrases: nothing is queued on purpose here, it only narrows down a failure)
        if k < len(mids):
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
        # the last call that wrote the frame directly (no draw since); whether the call at hand found a begun flush with fragments in it
        self.prev, self.was_begun = None, False
        # registers: memory kind, the call that wrote each, device registers written since the stream was last waited for, those among
        # them that a set_stream passed, device masks that were blurred, and per snapshot slot whether a translucent draw came since
        self.reg_mem, self.reg_by, self.unsynced, self.crossed, self.blurred, self.blend_since = {}, {}, set(), set(), set(), {}
        self.last_query = None              # (operation index, slot, out) of a device query against a snapshot that ran waiting draws
        self.fed = set()                    # registers written by a pass that ran queued or begun draws with fragments

    def wait(self):
        """The host waited for the stream: every register in device memory is complete."""
        self.unsynced.clear()
        self.crossed.clear()

    def wrote(self, reg, mem, by, fed=False):
        """fed: the call that wrote the register ran draws that were queued or begun and put fragments into the frame."""
        self.reg_mem[reg], self.reg_by[reg] = mem, by
        self.fed.discard(reg)
        if fed:
            self.fed.add(reg)
        self.blurred.discard(reg)
        if mem == "dev":
            self.unsynced.add(reg)

    def consumed(self, i, reg):
        """A call reads register `reg` on the stream in use."""
        if reg in self.crossed:
            if reg in self.fed:
                self.hit("pass_then_stream", i)
            self.crossed.discard(reg)

    def overwritten(self, i, reg):
        """A call rewrites device register `reg`: legal while a queued draw names it, since that draw's stages ran when it was queued."""
        if any(d["frags"] and reg in d["regs"] for d in self.queued):
            self.hit("inst_dev_overwritten", i)

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
        self.was_begun = live_begun = self.begun and self.live()
        if live_begun:
            m = "observe" if name in OBSERVATIONS else "draw" if name in ("draw_indexed", "draw_burst") else name
            if m in MID_OPS:
                self.hit("mid_" + m, i)
                if any(d["frags"] and d["kind"] in BLEND for d in self.queued):
                    self.hit("blend_mid_" + m, i)
        if name in ("write_framebuffer", "framebuffer_blur", "framebuffer_modulate", "zbuffer_restore"):
            self.prev = name
        if name == "read_reg":              # (it reads on the stream in use, then waits for it)
            for reg in a["regs"].split("+"):
                self.consumed(i, reg)
        if name in OBSERVATIONS or name in ("write_framebuffer", "write_zbuffer", "sync", "read_reg"):
            self.wait()
        # the interpreter uploads the arrays of a device-memory draw when it meets it, and waits for that; it waits for the rows of an
        # instance_stage in device memory, and a clip_stage over device arrays waits for its count
        if name in ("draw", "draw_indexed", "clip_stage") and a.get("mem") == "dev" or \
                name == "instance_stage" and self.reg_mem[a["inst"]] == "dev":
            self.wait()
        if name in ("clear", "write_zbuffer"):                          # (the frame a pass or a write left is gone, or no longer what a draw lands on)
            self.prev = None
        if name == "set_stream":            # (the library waits for the stream it leaves)
            passed = set(self.unsynced)
            self.wait()
            self.crossed = passed
        if name == "zbuffer_snapshot":
            self.blend_since[a["slot"]] = False
        if name == "zbuffer_restore" and self.blend_since.get(a["slot"]):
            self.hit("blend_restore", i)
        query, self.last_query = self.last_query, None
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
            if (q or live_begun) and a["what"] in ("occl_empty_slot", "shadow_empty_slot", "occl_in_strip", "shadow_in_strip"):
                self.hit("pass_refused_queued", i)
            if q and a["what"].startswith("inst_"):
                self.hit("inst_refused_queued", i)
            if a["what"] in ("unknown_kind", "bad_strip", "inst_bad_order", "inst_k_differs"):
                self.end_begun(i)
        elif name in ("occlusion_boxes", "shadow_mask", "framebuffer_modulate"):
            short = {"occlusion_boxes": "occl", "shadow_mask": "shadow", "framebuffer_modulate": "modulate"}[name]
            resident = name != "occlusion_boxes" or a["slot"] < 0
            if (q or live_begun) and resident:
                self.hit(short + "_queued", i)
            if name == "occlusion_boxes" and resident and self.clear_pending and not self.queued:
                self.hit("occl_clear_pending", i)
            fed = q or live_begun
            self.raster(i)
            if name == "framebuffer_modulate":
                mask = a["mask"]
                if mask == "none" or self.reg_mem[mask] == "host":
                    if a["scr"] and fed:
                        self.hit("modulate_scribbled", i)
                else:
                    self.consumed(i, mask)
                    if mask in self.blurred and mask in self.unsynced and self.reg_by[mask] == "shadow_chain":
                        self.hit("shadow_chain", i)
            else:
                if name == "occlusion_boxes" and self.reg_mem[a["boxes"]] == "dev":
                    self.consumed(i, a["boxes"])
                mem = a["cmem"] if name == "occlusion_boxes" else a["mem"]
                if mem == "host":
                    self.wait()
                # (a mask made while draws were waiting is the first link of a shadow chain)
                self.wrote(a["out"], mem, "shadow_chain" if name == "shadow_mask" and fed else name, fed=fed)
                if mem == "dev" and a["slot"] >= 0 and fed:
                    self.last_query = (i, a["slot"], a["out"])
        elif name == "image_blur":
            self.end_begun(i)
            self.consumed(i, a["reg"])
            self.blurred.add(a["reg"])
        elif name == "zbuffer_snapshot_free":
            if query and query[0] == i - 1 and query[1] == a["slot"] and query[2] in self.unsynced:
                self.hit("snapshot_free_queued", i)
            self.end_begun(i)
        elif name in ("array", "instances"):
            for b in arrays_of(name, a):
                self.reg_mem[b["reg"]], self.reg_by[b["reg"]] = b["mem"], "array"       # (uploaded before the program's first call: no wait here)
        elif name == "read_reg":
            self.end_begun(i)
        elif name in QUIET_OPS:
            src = a["inst"] if "inst" in a else a["boxes"] if "boxes" in a else a["depths"]
            out = a["codes"] if name == "frustum_boxes" else a["out"]
            if self.reg_mem[src] == "dev":
                if live_begun:
                    self.hit("quiet_begun", i)
                self.consumed(i, src)
                if out in self.reg_mem:
                    self.overwritten(i, out)
            self.wrote(out, self.reg_mem[src], name)
        elif name == "dev_copy":
            self.overwritten(i, a["reg"])
            self.wrote(a["reg"], "dev", name)
        elif name in ("draw_instanced", "instance_stage", "clip_stage"):
            if live_begun and name != "clip_stage":
                self.hit("inst_begun", i)
            if name != "clip_stage" or a["mem"] == "dev":
                self.end_begun(i)
        elif name in ("set_strip", "set_interleave"):
            if q:
                self.hit("strip_queued", i)
            self.end_begun(i)
            self.flush_queued(i)

    def queue(self, i, kind, frags, tex, scribbled, indexed, regs=(), touched=None, self_overlap=False, a=None, device_visible=0):
        """A draw of `frags` fragments (in the model) joins the queue.  regs: the device registers its call read; touched: the pixels
        a translucent draw wrote; device_visible: the instances of a call whose visibility bytes are in device memory."""
        base, source, _, may_discard = KINDS[kind]
        last = self.queued[-1] if self.queued else None
        if kind in BLEND and frags:
            if last and last["kind"] != kind and last["frags"]:
                self.hit("blend_kind_cut", i)
            if last and last["kind"] == kind and last["frags"] and last["touched"] is not None and (last["touched"] & touched).any() and self_overlap:
                self.hit("blend_same_kind_twice", i)
            if self.clear_pending and not self.queued:
                self.hit("blend_over_clear", i)
            if self.prev == "write_framebuffer":
                self.hit("blend_over_written", i)
            if self.prev in ("framebuffer_blur", "framebuffer_modulate"):
                self.hit("blend_over_pass", i)
            if self.was_begun:
                self.hit("blend_begun", i)
            self.blend_since = {slot: True for slot in self.blend_since}
        elif frags and last and last["kind"] == "TOVER_ND" and last["frags"] and a is not None and a.get("zoff", 0) > 0 and last["seed"] == a.get("seed"):
            self.hit("nodepth_then_opaque", i)      # the same triangles, further away: they pass only because the depths were left alone
        if device_visible and any(d["frags"] and 0 < d["device_visible"] < device_visible for d in self.queued) and device_visible > INST_BLOCK:
            self.hit("inst_two_calls", i)
        self.prev, self.was_begun = None, False
        if self.queued and self.queued[-1]["kind"] != kind and (may_discard or self.queued[-1]["discards"]):
            if self.live() or frags:
                self.hit("kind_cut", i)
            self.raster(i)
        if len(self.queued) >= MAX_DRAWS:
            if self.live():
                self.hit("max_draws", i)
            self.raster(i)
        self.queued.append(dict(kind=kind, frags=frags, tex=tuple(tex), discards=may_discard, regs=set(regs), touched=touched,
                                seed=None if a is None else a.get("seed"), device_visible=device_visible, staged=bool(a and a.get("mem") == "host"),
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


def call_uniforms(p, a):
    """The uniform block of an instanced call: the camera's, with the cells of a CHECKER kind."""
    cam = camera(p)
    return api.make_uniforms(cam.model_view, cam.key, cam.fill, cam.rim, cells=a.get("cells", 0))


def run_model(program, lazy_scribble=None, shadow=None, reverse_order=None, swap_arrays=None, alter=None):
    """Execute the program at once, as the reference would: every call takes effect where it stands.  Returns the observations:
    (tag, operation index, eye, payload...) with tags 'fb', 'z', 'stats', 'frame', 'post', 'bounds', 'rows' (clip, varyings, colours
    and their count) and, for a register, what it holds: 'codes', 'mask', 'boxes', 'depths', 'order'.  lazy_scribble = i: the
    scribble of operation i happens BEFORE its call (what an implementation that reads the caller's arrays late would render).
    reverse_order = i: the instanced call i visits its order list backwards.  swap_arrays = {k: j}: the draw k renders the arrays of
    the draw j (what it reads when the staging arena was reset under it and the draw j's arrays took their place).
    alter = {i: how}: operation i without one rule - 'stale': it reads its device registers as they were before anything wrote them
    (zeros: the pass that fills them has not run on the stream it reads them on); 'all_visible': an instanced call ignores its
    visibility bytes; 'no_plane': a clipped draw ignores its plane; 'resident': a query against a snapshot reads the resident depths
    (the slot's memory is gone).
    shadow: a _Shadow that collects the hazards of the program."""
    from oracle import orc
    p = program
    o = orc.Oracle(p.w, p.h, p.bpp)
    sh = shadow or _Shadow()
    obs, snaps, eye = [], {}, False
    rect = (0, 0, p.w, p.h)
    regs, what_of = {}, {}                              # registers: every one a numpy array here
    swap_arrays, alter = swap_arrays or {}, alter or {}

    def reg(i, r):
        return np.zeros_like(regs[r]) if alter.get(i) == "stale" and sh.reg_mem[r] == "dev" else regs[r]

    def put(i, reg, what, value, observe=False):
        regs[reg], what_of[reg] = value, what
        if observe:
            obs.append((what, i, eye, value.copy()))

    def instanced(i, name, a):
        verts, idx, fc = mesh_of(a["mesh"])
        names = [a[k] for k in ("inst", "icol", "vis", "ord") if a[k] != "none"]
        host = [r for r in names if sh.reg_mem[r] == "host"]
        dev = [r for r in names if sh.reg_mem[r] == "dev"]
        if a["scr"] and lazy_scribble == i:
            for r in host:
                scribble_reg(regs[r], what_of[r])
            if a["mmem"] == "host":
                verts[:], idx[:], fc[:] = verts[::-1].copy(), idx[::-1].copy(), ~fc
        inst, icol, vis, order = (None if a[k] == "none" else regs[a[k]] for k in ("inst", "icol", "vis", "ord"))
        if alter.get(i) == "all_visible":
            vis = None
        if order is not None and reverse_order == i:
            order = order[::-1]
        device_order = a["ord"] != "none" and sh.reg_mem[a["ord"]] == "dev"
        device_visible = a["vis"] != "none" and sh.reg_mem[a["vis"]] == "dev"
        clip, vary, col, n_drawn = instanced_rows(p, a, verts, idx, fc if a["fcol"] else None, inst, icol, vis, order, device_order)
        live = bool(sh.queued) and sh.live()
        if name == "instance_stage":
            obs.append(("rows", i, eye, clip, vary, col, clip.shape[0]))
        else:
            if n_drawn == 0 and device_visible and live:
                sh.hit("inst_zero", i)
            before, touched, overlap = frags(), None, False
            if n_drawn:
                if a["kind"] in BLEND:
                    touched, overlap = blend_draw(o, clip, col, *BLEND[a["kind"]])
                else:
                    o.draw(KINDS[a["kind"]][0], clip, vary, col, _orc_uniforms(call_uniforms(p, a)))
                drawn = frags() - before
                if drawn and a["kind"] in BLEND and device_order and device_visible and {a["vis"], a["ord"]} <= sh.unsynced and \
                        sh.reg_by[a["ord"]] == "depth_order" and sh.reg_by[a["vis"]] == "frustum_boxes":
                    sh.hit("chain_device", i)
                sh.queue(i, a["kind"], drawn, (), False, False, regs=dev, touched=touched, self_overlap=overlap,
                         device_visible=a["n"] if device_visible else 0)
                if drawn and a["scr"] and host:
                    sh.hit("inst_host_scribbled", i)
        if device_visible or device_order:
            sh.wait()                                   # the one wait of such a call, for the count
        if a["scr"] and lazy_scribble != i:
            for r in host:
                scribble_reg(regs[r], what_of[r])

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
            clip, vary, col, u = draw_arrays(p, dict(p.ops[swap_arrays[i]][1], kind=a["kind"]) if i in swap_arrays else a)
            if lazy_scribble == i:
                scribble_draw(p, a, clip, vary, col, u)
        if a.get("plane") and alter.get(i) != "no_plane":       # the clip stage in front of the draw
            clip, vary, col = clip_model.clip_model(PLANES[a["plane"]], clip, vary, col, attrs=clip_model.LAYOUTS[base])
            if a["mem"] == "dev":
                live = bool(sh.queued) and sh.live()
                if clip.shape[0] == 0 and live and any(d["staged"] and d["frags"] for d in sh.queued):
                    sh.hit("clip_drops_all_queued", i)
                elif clip.shape[0] == 0 and not sh.queued and not sh.clear_pending:
                    sh.hit("clip_drops_all_idle", i)
                elif clip.shape[0] and live and sh.queued[-1]["kind"] != a["kind"]:
                    sh.hit("clip_wait_queued", i)
                sh.wait()                               # the one wait of a clipped draw of device arrays
            if clip.shape[0] == 0:
                return
        touched, overlap = None, False
        if a["kind"] in BLEND:
            touched, overlap = blend_draw(o, clip, col, *BLEND[a["kind"]])
        elif clip.shape[0]:
            o.draw(base, clip, vary, col, _orc_uniforms(u))
            eye = eye or base == EYE
        sh.queue(i, a["kind"], frags() - before, a.get("tex", ()), bool(a.get("scr")), indexed, touched=touched, self_overlap=overlap, a=a)

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
        elif name in ("array", "instances"):
            for b in arrays_of(name, a):
                put(i, b["reg"], b["what"], array_of(p, b))
        elif name == "dev_copy":
            regs[a["reg"]][...] = array_of(p, a)
        elif name == "read_reg":
            for r in a["regs"].split("+"):
                obs.append((what_of[r], i, eye, reg(i, r).copy()))
        elif name == "occlusion_boxes":
            depth = o.z if a["slot"] < 0 or alter.get(i) == "resident" else snaps[a["slot"]]
            view_proj = np.eye(4) if a["vp"] == "ndc" else camera(p).view_proj
            codes = occlusion_model.codes(depth, np.array(o.t.viewport).reshape(4, 4), view_proj, regs[a["boxes"]])
            prev = p.ops[i - 1] if i else None
            if a["slot"] < 0 and prev and prev[0] == name and prev[1]["slot"] >= 0 and prev[1]["boxes"] == a["boxes"] and \
                    not np.array_equal(codes, regs[prev[1]["out"]]):
                sh.hit("occl_snapshot_stale", i)
            put(i, a["out"], "codes", codes, observe=a["cmem"] == "host")
        elif name == "shadow_mask":
            m, r = shadow_params_of(a)
            put(i, a["out"], "mask", shadow_model.shadow_mask(o.z, m, snaps[a["slot"]], SHADOW_BIAS, SHADOW_DARKNESS, r), observe=a["mem"] == "host")
        elif name == "framebuffer_modulate":
            host = a["mask"] == "none" or sh.reg_mem[a["mask"]] == "host"
            mask = array_of(p, dict(what="mask", n=0, seed=a["seed"])) if a["mask"] == "none" else reg(i, a["mask"])
            if host and a["scr"] and lazy_scribble == i:
                scribble_reg(mask, "mask")
            o.fb[:] = shadow_model.modulate(o.fb, mask)
            if host and a["scr"] and lazy_scribble != i:
                scribble_reg(mask, "mask")
        elif name == "image_blur":
            regs[a["reg"]] = image_ops_model.gaussian_blur(regs[a["reg"]][..., None], api.gaussian_kernel(a["r"]))[..., 0]
        elif name == "zbuffer_snapshot_free":
            snaps.pop(a["slot"], None)
        elif name == "instance_boxes":
            put(i, a["out"], "boxes", CC.model_boxes(np.array(LOCAL_BOX[a["mesh"]]), regs[a["inst"]]))
        elif name == "frustum_boxes":
            planes = camera(p).planes if a["planes"] == "cam" else reject_planes()
            put(i, a["codes"], "codes", CC.model_codes(planes, regs[a["boxes"]], regs[a["codes"]] if a["merge"] else None))
        elif name == "instance_depths":
            put(i, a["out"], "depths", order_model.depths(camera(p).model_view, np.zeros(3), regs[a["inst"]]))
        elif name == "depth_order":
            put(i, a["out"], "order", order_model.order(regs[a["depths"]], a["dir"]))
        elif name in ("draw_instanced", "instance_stage"):
            instanced(i, name, a)
        elif name == "clip_stage":
            clip, vary, col, _ = draw_arrays(p, a)
            out = clip_model.clip_model(PLANES[a["plane"]], clip, vary, col, attrs=clip_model.LAYOUTS[KINDS[a["kind"]][0]])
            obs.append(("rows", i, eye) + tuple(out) + (out[0].shape[0],))
        else:
            assert name in ("flush", "flush_begin", "flush_end", "sync", "set_stream", "register_shader", "register_vertex_shader", "refused"), name
    return obs


def hazards(program):
    """[(hazard name, operation index)] of a program, from a run of the model."""
    sh = _Shadow()
    run_model(program, shadow=sh)
    return sh.events


# ---- the interpreter over the C ABI ----------------------------------------------------------------------------------------
def run_gpu(program):
    """Execute the program on one Context; the observations in run_model's form (eye left False).  Device arrays stay alive until
    the context is closed and are never scribbled; host arrays are scribbled right after the draw that took them returns.
    Registers in device memory are written only by the program's own operations (a pass, a quiet call, a dev_copy on the stream the
    context was given), so a queued call reads what stream order gives it; read_reg waits for the stream and copies them back."""
    import torch
    p = program
    obs, keep, kinds = [], [], {}
    streams = []
    regs, reg_mem, what_of, stages = {}, {}, {}, {}     # registers: numpy arrays (host) or torch tensors (dev); vertex stages by name
    ctx = api.Context(p.w, p.h, p.bpp)
    try:
        def to_dev(x):
            t = torch.from_numpy(np.ascontiguousarray(x)).cuda() if x.dtype == np.uint8 else cases.device_array(x)
            torch.cuda.synchronize()                            # the upload ran on torch's stream, which the context's does not follow
            return t

        def put(reg, what, mem, value):
            regs[reg], what_of[reg], reg_mem[reg] = value, what, mem

        # Everything the program keeps in device memory is uploaded before its first call, and outputs are allocated uninitialised: the
        # interpreter itself never waits for the device between the calls of a program (a wait there would complete what a queued
        # call is meant to find in stream order).  An `array` in device memory only names its tensor; its contents were there.
        uploads = {(i, b["reg"]): to_dev(array_of(p, b)) for i, (name, a) in enumerate(p.ops)
                   for b in ([a] if name == "dev_copy" else arrays_of(name, a)) if b["mem"] == "dev"}
        meshes = {m: tuple(cases.device_array(x) for x in mesh_of(m))
                  for m in sorted({a["mesh"] for name, a in p.ops if name in ("draw_instanced", "instance_stage") and a["mmem"] == "dev"})}
        torch.cuda.synchronize()

        def kind_of(name):
            return kinds[name] if KINDS[name][1] is not None else KINDS[name][0]

        def host_value(r):
            v = regs[r] if reg_mem[r] == "host" else regs[r].cpu().numpy()
            return np.array(v.view(np.uint32) if v.dtype == np.int32 else v)

        def draw(a):
            clip, vary, col, u = draw_arrays(p, a)
            kind = kind_of(a["kind"])
            plane = dict(clip_plane=PLANES[a["plane"]]) if a.get("plane") else {}
            if a["mem"] == "dev":
                dev = tuple(None if x is None else cases.device_array(x) for x in (clip, vary, col))
                torch.cuda.synchronize()                        # the uploads ran on torch's stream, which the context's does not follow
                keep.append(dev)
                ctx.draw(kind, dev[0], dev[1], dev[2], u, device=True, **plane)
            else:
                ctx.draw(kind, clip, vary, col, u, **plane)
                if a["scr"]:
                    scribble_draw(p, a, clip, vary, col, u)

        def instanced(i, name, a):
            verts, idx, fc = mesh_of(a["mesh"])
            names = [a[k] for k in ("inst", "icol", "vis", "ord") if a[k] != "none"]
            inst, icol, vis, order = (None if a[k] == "none" else regs[a[k]] for k in ("inst", "icol", "vis", "ord"))
            mesh_dev, inst_dev = a["mmem"] == "dev", reg_mem[a["inst"]] == "dev"
            order_dev = order is not None and reg_mem[a["ord"]] == "dev"
            fcol = fc if a["fcol"] else None
            mesh = (verts, idx, fcol)
            if mesh_dev:
                mesh = meshes[a["mesh"]][:2] + (meshes[a["mesh"]][2] if a["fcol"] else None,)
            vs = None if a["vs"] == "builtin" else stages[a["vs"]]
            u, proj = call_uniforms(p, a), camera(p).projection
            common = dict(instances=inst, face_colors=mesh[2], instance_colors=icol, visible=vis, device=mesh_dev, instances_device=inst_dev,
                          order=order, order_device=order_dev)
            if name == "draw_instanced":
                ctx.draw_instanced(kind_of(a["kind"]), u, proj, mesh[0], mesh[1], vertex_shader=vs, **common)
            else:
                nf, K = idx.shape[0], 24 if vs is None else 0
                out = None
                if inst_dev:
                    cap = max((a["n"] if order is None else int(order.shape[0])) * nf, 1)
                    out = (torch.empty((cap, 12), dtype=torch.float64, device="cuda"), torch.empty((cap, K), dtype=torch.float64, device="cuda") if K else None,
                           torch.empty(cap, dtype=torch.int32, device="cuda") if icol is not None or fcol is not None else None)
                clip, vary, col, n = ctx.instance_stage(-1 if vs is None else vs, u, proj, mesh[0], mesh[1], out=out, **common)
                if inst_dev:
                    ctx.sync()
                    clip, vary, col = (None if x is None else x.cpu().numpy()[:n] for x in (clip, vary, col))
                    col = None if col is None else col.view(np.uint32)
                obs.append(("rows", i, False, np.array(clip), np.array(vary) if K else None, None if col is None else np.array(col), n))
            if a["scr"]:
                for r in names:
                    if reg_mem[r] == "host":
                        scribble_reg(regs[r], what_of[r])
                if not mesh_dev:
                    verts[:], idx[:], fc[:] = verts[::-1].copy(), idx[::-1].copy(), ~fc

        for i, (name, a) in enumerate(p.ops):
            if name == "draw":
                draw(a)
            elif name == "draw_burst":
                for b in burst_ops(a):
                    draw(b)
            elif name == "draw_indexed":
                verts, idx, u, proj = mesh_arrays(p, a)
                plane = dict(clip_plane=PLANES[a["plane"]]) if a.get("plane") else {}
                if a["mem"] == "dev":
                    dev = (cases.device_array(verts), cases.device_array(idx))
                    torch.cuda.synchronize()
                    keep.append(dev)
                    ctx.draw_indexed(KINDS[a["kind"]][0], u, proj, dev[0], dev[1], device=True, **plane)
                else:
                    ctx.draw_indexed(KINDS[a["kind"]][0], u, proj, verts, idx, **plane)
                    if a["scr"]:
                        scribble_mesh(verts, idx, u, proj)
            elif name == "register_shader":
                source, K, may_discard = (KINDS[a["src"]][1:] if a["src"] in KINDS else EXTRA_SOURCES[a["src"]])
                blend = dict(reads_dest=True, depth_write=BLEND[a["src"]][1]) if a["src"] in BLEND else {}
                kinds[a["src"]] = ctx.register_shader(source, K, may_discard, **blend)
            elif name == "register_vertex_shader":
                stages[a["src"]] = ctx.register_vertex_shader(*VERTEX_STAGES[a["src"]])
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
                elif a["what"] == "occl_empty_slot":
                    boxes, out = array_of(p, dict(what="boxes", n=4, seed=1)), np.zeros(4, np.uint8)
                    rc, want = ctx.L.trgl_occlusion_boxes(ctx.h, api._dp(np.eye(4).reshape(16)), boxes.ctypes.data, 4, api.MEM_HOST, api.MAX_Z_SNAPSHOTS - 1,
                                                          out.ctypes.data, api.MEM_HOST), E_STATE
                elif a["what"] == "occl_in_strip":              # (the resident depths: no slot to be empty)
                    boxes, out = array_of(p, dict(what="boxes", n=4, seed=1)), np.zeros(4, np.uint8)
                    rc, want = ctx.L.trgl_occlusion_boxes(ctx.h, api._dp(np.eye(4).reshape(16)), boxes.ctypes.data, 4, api.MEM_HOST, -1,
                                                          out.ctypes.data, api.MEM_HOST), E_STATE
                elif a["what"] in ("shadow_empty_slot", "shadow_in_strip"):
                    out, params = np.zeros((p.h, p.w), np.uint8), api.make_shadow_params(np.eye(4), SHADOW_BIAS, SHADOW_DARKNESS, 0)
                    slot = api.MAX_Z_SNAPSHOTS - 1 if a["what"] == "shadow_empty_slot" else 0        # (the strip is looked at before the slot's contents)
                    rc, want = ctx.L.trgl_shadow_mask(ctx.h, C.byref(params), slot, out.ctypes.data, api.MEM_HOST), E_STATE
                elif a["what"] in ("inst_bad_order", "inst_k_differs"):
                    verts, idx, _ = mesh_of("cube")
                    inst, u, proj = array_of(p, dict(what="inst", n=3, stride=16, seed=2)), call_uniforms(p, a), camera(p).projection.reshape(16)
                    order = np.array([2, 3, 0], np.uint32)      # 3 is not an instance
                    mesh = (verts.ctypes.data, 8, 8, idx.ctypes.data, 12, None, api.MEM_HOST, inst.ctypes.data, 16, 3, None, None, api.MEM_HOST)
                    if a["what"] == "inst_bad_order":
                        rc = ctx.L.trgl_draw_instanced_ordered(ctx.h, -1, PHONG, C.byref(u), api._dp(proj), *mesh, order.ctypes.data, 3, api.MEM_HOST)
                    else:                                       # the built-in stage has 24 varyings, FLAT none
                        rc = ctx.L.trgl_draw_instanced(ctx.h, -1, FLAT, C.byref(u), api._dp(proj), *mesh)
                    want = E_INVALID
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
            elif name in ("array", "instances"):
                for b in arrays_of(name, a):
                    put(b["reg"], b["what"], b["mem"], uploads[i, b["reg"]] if b["mem"] == "dev" else array_of(p, b))
            elif name == "dev_copy":                            # in stream order behind what the context has queued: it is on this torch stream
                src = uploads[i, a["reg"]]
                assert streams and ctx.stream == streams[-1].cuda_stream, "dev_copy: the context is not on a torch stream"
                with torch.cuda.stream(streams[-1]):
                    regs[a["reg"]].copy_(src)
            elif name == "read_reg":
                ctx.sync()
                for r in a["regs"].split("+"):
                    obs.append((what_of[r], i, False, host_value(r)))
            elif name == "occlusion_boxes":
                boxes, dev = regs[a["boxes"]], reg_mem[a["boxes"]] == "dev"
                n = int(boxes.shape[0])
                view_proj = np.ascontiguousarray(np.eye(4).reshape(16) if a["vp"] == "ndc" else camera(p).view_proj, np.float64)
                out = torch.empty(n, dtype=torch.uint8, device="cuda") if a["cmem"] == "dev" else np.zeros(n, np.uint8)     # (every code is written)
                ctx._chk(ctx.L.trgl_occlusion_boxes(ctx.h, api._dp(view_proj), boxes.data_ptr() if dev else boxes.ctypes.data, n,
                                                    api.MEM_DEVICE if dev else api.MEM_HOST, a["slot"], out.data_ptr() if a["cmem"] == "dev" else out.ctypes.data,
                                                    api.MEM_DEVICE if a["cmem"] == "dev" else api.MEM_HOST))
                put(a["out"], "codes", a["cmem"], out)
                if a["cmem"] == "host":
                    obs.append(("codes", i, False, out.copy()))
            elif name == "shadow_mask":
                m, r = shadow_params_of(a)
                out = ctx.shadow_mask(api.make_shadow_params(m, SHADOW_BIAS, SHADOW_DARKNESS, r), a["slot"], device=a["mem"] == "dev")
                put(a["out"], "mask", a["mem"], out)
                if a["mem"] == "host":
                    obs.append(("mask", i, False, out.copy()))
            elif name == "framebuffer_modulate":
                mask = array_of(p, dict(what="mask", n=0, seed=a["seed"])) if a["mask"] == "none" else regs[a["mask"]]
                host = a["mask"] == "none" or reg_mem[a["mask"]] == "host"
                ctx.framebuffer_modulate(mask, device=not host)
                if host and a["scr"]:
                    scribble_reg(mask, "mask")
            elif name == "image_blur":
                ctx.image_blur(regs[a["reg"]].view(p.h, p.w, 1), a["r"], device=True)
            elif name == "zbuffer_snapshot_free":
                ctx.zbuffer_snapshot_free(a["slot"])
            elif name == "instance_boxes":
                put(a["out"], "boxes", reg_mem[a["inst"]], ctx.instance_boxes(np.array(LOCAL_BOX[a["mesh"]]), regs[a["inst"]]))
            elif name == "frustum_boxes":
                planes = camera(p).planes if a["planes"] == "cam" else reject_planes()
                put(a["codes"], "codes", reg_mem[a["boxes"]], ctx.frustum_boxes(planes, regs[a["boxes"]], codes=regs.get(a["codes"]), merge=bool(a["merge"])))
            elif name == "instance_depths":
                dev = reg_mem[a["inst"]] == "dev"
                put(a["out"], "depths", reg_mem[a["inst"]], ctx.instance_depths(camera(p).model_view, np.zeros(3), regs[a["inst"]], device=dev))
            elif name == "depth_order":
                d = regs[a["depths"]]
                if reg_mem[a["depths"]] == "dev":               # through the C ABI: the order goes into the register it already has, when it has one
                    if a["out"] not in regs:
                        put(a["out"], "order", "dev", torch.empty(int(d.shape[0]), dtype=torch.int32, device="cuda"))
                    ctx._chk(ctx.L.trgl_depth_order(ctx.h, d.data_ptr(), int(d.shape[0]), a["dir"], api.MEM_DEVICE, regs[a["out"]].data_ptr()))
                else:
                    put(a["out"], "order", "host", ctx.depth_order(d, front_to_back=bool(a["dir"])))
            elif name in ("draw_instanced", "instance_stage"):
                instanced(i, name, a)
            elif name == "clip_stage":
                clip, vary, col, _ = draw_arrays(p, a)
                attrs = clip_model.LAYOUTS[KINDS[a["kind"]][0]]
                if a["mem"] == "dev":
                    dev = tuple(None if x is None else to_dev(x) for x in (clip, vary, col))
                    oc, ov, ocol, n = ctx.clip_stage(PLANES[a["plane"]], *dev, attrs=attrs, device=True)
                    out = tuple(None if x is None else x.cpu().numpy()[:n] for x in (oc, ov, ocol))      # (the call has waited for the stream)
                    out = (out[0], out[1], None if out[2] is None else out[2].view(np.uint32))
                else:
                    out = ctx.clip_stage(PLANES[a["plane"]], clip, vary, col, attrs=attrs)
                obs.append(("rows", i, False) + tuple(None if x is None else np.array(x) for x in out) + (out[0].shape[0],))
            else:
                raise AssertionError(f"unknown operation {name}")
    finally:
        ctx.close()             # waits for the stream in use; only then may the device arrays and the torch streams go
        del keep, streams, regs, uploads, meshes
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
    elif tag == "rows":
        assert got[6] == want[6], f"rows: {got[6]} rows, expected {want[6]}"
        for what, g, w in zip(("clip", "varyings", "colours"), got[3:6], want[3:6]):
            assert clip_model.same_bits(g, w), f"rows: {what} differ"
    elif tag in ("codes", "mask", "boxes", "depths", "order"):
        assert clip_model.same_bits(got[3], want[3]), f"{tag}: {got[3]} != {want[3]}"
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
