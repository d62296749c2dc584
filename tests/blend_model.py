"""The yardstick of the blending tests (include/trgl.h, "User shaders that blend"): an immediate-mode renderer whose fragment() sees the
pixel it is drawn over and may leave the depth alone, built on the CPU oracle and on nothing of the library under test.

One triangle at a time on an orc.Oracle: save z and the frame, draw the triangle FLAT, and the pixels whose depth bits changed are
exactly this triangle's z-passes (the test is strict <, our_gl.cpp:165).  For those pixels dst is the saved frame masked to bpp bytes
(TGAImage::get), a numpy restatement of the test shader maps (src colour, dst) to (discard, colour), the frame gets bpp bytes of it
(TGAImage::set), and the saved depth goes back where the fragment was discarded - or everywhere when depth writes are off.
The triangle count and the bbox are the oracle's; fragments_drawn and the z range are folded here in the reference's order
(triangle, then x, then y) with std::min / std::max's keep-the-first rule, so the sign of a zero end comes out right.

The test shaders depend on in.color and in.dst only: each is a HIP source and the numpy function that restates it."""
import math

import numpy as np

from oracle import orc
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import FLAT

# ---- the test shaders: (HIP source, restatement) ----------------------------------------------------------------------
OVER_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
"""
# alpha test: fragments below half coverage are discarded, the others blended
ALPHA_TEST_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    return trgl_frag_out{ (in.color >> 24) < 128u, trgl_blend_over(in.color, in.dst) };
}
"""
# additive, saturating per byte: a second blending kind
ADD_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    uint32_t out = 0;
    for (int i = 0; i < 32; i += 8) {
        const uint32_t s = ((in.color >> i) & 255u) + ((in.dst >> i) & 255u);
        out |= (s > 255u ? 255u : s) << i;
    }
    return trgl_frag_out{ false, out };
}
"""
# a plain discarding kind: odd colours are discarded.  Registered without TRGL_SHADER_READS_DEST, so in.dst is 0
ODD_DISCARD_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ (in.color & 1u) != 0, in.color ^ in.dst }; }
"""
# returns 0xAA in the three upper bytes and puts what dst holds above the frame's bytes into the blue byte: dst >> 24 for a
# 3-byte frame, bytes 1 to 3 for a 1-byte frame.  Blue stays 0 exactly when dst is masked to the frame's bytes.
PROBE_BPP3_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    return trgl_frag_out{ false, 0xAA000000u | (in.color & 0x00ffff00u) | (in.dst >> 24) };
}
"""
PROBE_BPP1_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    return trgl_frag_out{ false, 0xAAAAAA00u | (((in.dst >> 8) | (in.dst >> 16) | (in.dst >> 24)) & 255u) };
}
"""
# the same source under every contract: the plain one returns the colour
PORTABLE_SRC = r"""
#if TRGL_USER_MAY_DISCARD
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, in.color ^ in.dst }; }
#else
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color ^ in.dst; }
#endif
"""


def blend_over(src, dst):
    """trgl_blend_over, in integers."""
    src, dst = src.astype(np.uint32), dst.astype(np.uint32)
    a = src >> 24
    na = 255 - a
    out = np.zeros_like(src)
    for i in (0, 8, 16):
        out |= ((((src >> i) & 255) * a + ((dst >> i) & 255) * na + 127) // 255) << i
    return out | (((255 * a + (dst >> 24) * na + 127) // 255) << 24)


def f_source(src, dst):
    """return src, never discard: the FLAT kind."""
    return np.zeros(src.shape, bool), src


def f_over(src, dst):
    return np.zeros(src.shape, bool), blend_over(src, dst)


def f_alpha_test(src, dst):
    return (src >> 24) < 128, blend_over(src, dst)


def f_add(src, dst):
    out = np.zeros_like(src)
    for i in (0, 8, 16, 24):
        out |= np.minimum(((src >> i) & 255) + ((dst >> i) & 255), 255).astype(np.uint32) << i
    return np.zeros(src.shape, bool), out


def f_odd_discard(src, dst):
    return (src & 1) != 0, src


def f_probe_bpp3(src, dst):
    return np.zeros(src.shape, bool), np.uint32(0xAA000000) | (src & np.uint32(0x00ffff00)) | (dst >> 24)


def f_probe_bpp1(src, dst):
    return np.zeros(src.shape, bool), np.uint32(0xAAAAAA00) | (((dst >> 8) | (dst >> 16) | (dst >> 24)) & 255)


# ---- the model --------------------------------------------------------------------------------------------------------
class Model:
    """fb, z and stats of an immediate-mode renderer.  start = (fb, z): the frame starts from these buffers; stats0: the counters
    so far (a stats tuple), for a frame that earlier draws of another renderer began.  mask_dst=False forms dst from four bytes of
    the last colour written, as a renderer that kept the pixel in a 32-bit register and forgot the frame's width would."""

    def __init__(self, w, h, bpp, viewport=None, clear=(0, 0, 0, 255), zclear=np.inf, start=None, stats0=None, mask_dst=True):
        self.o = orc.Oracle(w, h, bpp, viewport=viewport, clear_bgra=clear, z_clear=zclear)
        self.bpp, self.mask_dst = bpp, mask_dst
        if start is not None:
            self.o.fb[:] = start[0]
            self.o.z[:] = start[1]
        self.frags, self.min_z, self.max_z = 0, math.inf, -math.inf
        if stats0 is not None:
            s = self.o.t.stats
            s.triangles_rasterized, self.frags, s.min_x, s.min_y, s.max_x, s.max_y = stats0[:6]
            self.min_z, self.max_z = math.copysign(stats0[6], stats0[8]), math.copysign(stats0[7], stats0[9])
        # the pixel as a 32-bit word: the frame's bytes, and above them what the last writer's colour had there
        self.word = np.zeros((h, w), np.uint32)
        for i in range(bpp):
            self.word |= self.o.fb[..., i].astype(np.uint32) << (8 * i)
        if start is None and not mask_dst:
            for i in range(bpp, 4):
                self.word |= np.uint32(clear[i]) << np.uint32(8 * i)

    def draw(self, clip, colors, fn, depth_write=True):
        o = self.o
        clip = np.ascontiguousarray(clip, np.float64)
        colors = np.ascontiguousarray(colors, np.uint32)
        keep = np.uint32(0xffffffff >> (8 * (4 - self.bpp)))
        for i in range(clip.shape[0]):
            z0 = o.z.copy()
            o.draw(FLAT, clip[i:i + 1], None, colors[i:i + 1])
            ys, xs = np.nonzero(o.z.view(np.uint64) != z0.view(np.uint64))          # this triangle's z-passes
            if ys.size == 0:
                continue
            order = np.lexsort((ys, xs))                                            # our_gl.cpp:147-148: x outside, y inside
            ys, xs = ys[order], xs[order]
            zn = o.z[ys, xs]
            dst = self.word[ys, xs] & keep if self.mask_dst else self.word[ys, xs]
            discard, out = fn(np.full(ys.shape, colors[i], np.uint32), dst)
            out = out.astype(np.uint32)
            drawn = ~discard
            self.word[ys[drawn], xs[drawn]] = out[drawn]
            if depth_write:
                o.z[ys[discard], xs[discard]] = z0[ys[discard], xs[discard]]         # our_gl.cpp:188
            else:
                o.z[:] = z0
            zd = zn[drawn]
            self.frags += int(drawn.sum())
            if zd.size:
                lo, hi = zd.min(), zd.max()
                lo, hi = float(zd[np.flatnonzero(zd == lo)[0]]), float(zd[np.flatnonzero(zd == hi)[0]])   # the first of equals
                if lo < self.min_z:                                                 # std::min(min_z, z): z only when smaller
                    self.min_z = lo
                if self.max_z < hi:
                    self.max_z = hi
        for b in range(self.bpp):                                                   # TGAImage::set: bpp bytes
            o.fb[..., b] = (self.word >> np.uint32(8 * b)).astype(np.uint8)

    @property
    def fb(self):
        return self.o.fb

    @property
    def z(self):
        return self.o.z

    @property
    def stats(self):
        t = self.o.stats
        return (t[0], self.frags) + t[2:6] + (self.min_z, self.max_z, math.copysign(1.0, self.min_z), math.copysign(1.0, self.max_z))

    def result(self):
        """(fb, z, stats tuple, stats line), as the GPU harnesses return them (copies)."""
        return self.fb.copy(), self.z.copy(), self.stats, orc.format_stats_line(self.stats)


# ---- seeded scenes ----------------------------------------------------------------------------------------------------
def scene(w, h, n, seed, rmin=3.0, rmax=40.0, vw=None, vh=None):
    """n overlapping triangles for a w x h frame (or a vw x vh viewport in it) with random 32-bit colours: random alphas."""
    clip, _ = scenes.random_triangles(n, vw or w, vh or h, seed=seed, rmin=rmin, rmax=rmax, perspective_w=True)
    col = (scenes.SplitMix64(seed + 1000).u64(n) >> np.uint64(32)).astype(np.uint32)
    return clip, col


# the frames of the GPU tests: small, and each where the kernel can still go wrong
FRAMES = {
    # (blue 0 in these two clears: the probe shaders of the 3-byte alpha case leave blue 0 on every pixel)
    "96x64_bpp1": dict(w=96, h=64, bpp=1, n=260, seed=7101, clear=(0, 30, 40, 255)),
    "96x64_bpp3": dict(w=96, h=64, bpp=3, n=260, seed=7102, clear=(0, 30, 40, 255)),
    "96x64_bpp4": dict(w=96, h=64, bpp=4, n=260, seed=7103),
    "37x29_partial_blocks": dict(w=37, h=29, bpp=3, n=150, seed=7104, rmax=20.0),              # below one tile
    "32x32_long_list": dict(w=32, h=32, bpp=4, n=300, seed=7105, rmin=6.0, rmax=30.0),         # a tile list past one 64-entry step
    "101x67_viewport_zclear": dict(w=101, h=67, bpp=3, n=260, seed=7106, vx=9, vy=5, vw=80, vh=56, clear=(7, 8, 9, 10), zclear=0.25),
}


def frame(name):
    """The make_case-style description of FRAMES[name] and its one draw: (dict for Model / a context, clip, colours)."""
    f = FRAMES[name]
    clip, col = scene(f["w"], f["h"], f["n"], f["seed"], f.get("rmin", 3.0), f.get("rmax", 40.0), f.get("vw"), f.get("vh"))
    vp = scenes.init_viewport(f.get("vx", 0), f.get("vy", 0), f.get("vw", f["w"]), f.get("vh", f["h"]))
    return dict(w=f["w"], h=f["h"], bpp=f["bpp"], viewport=vp, clear=f.get("clear", (20, 30, 40, 255)), zclear=f.get("zclear", np.inf)), clip, col


_cache = {}


def model_frame(name, fn, depth_write=True, reverse=False, mask_dst=True):
    """The model's result() for FRAMES[name] drawn with one shader; computed once per argument set and shared (do not write to it)."""
    key = (name, fn, depth_write, reverse, mask_dst)
    if key not in _cache:
        cfg, clip, col = frame(name)
        m = Model(**cfg, mask_dst=mask_dst)
        m.draw(clip[::-1] if reverse else clip, col[::-1] if reverse else col, fn, depth_write)
        _cache[key] = m.result()
    return _cache[key]
