"""ctypes binding of the CPU oracle (oracle/libtrgl_oracle.so) — TEST INFRASTRUCTURE, NOT PRODUCT.

Importable only from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
Also holds the writers/runners for oracle/_ref/ref_harness (the reference's own rasterize() compiled in place from the
reference tree) and oracle/_ref/ref_shaders (the same plus the reference's own main.cpp shaders, vertex stage, z-buffer
image and SSAO, and model.cpp samplers); both exist only where the reference tree does.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtrgl_oracle.so")
REF_HARNESS = os.path.join(HERE, "_ref", "ref_harness")
REF_HARNESS_FAST = os.path.join(HERE, "_ref", "ref_harness_fast")   # -O3 -DNDEBUG build, for cpu_baseline timing
REF_SHADERS = os.path.join(HERE, "_ref", "ref_shaders")             # the reference's own PhongShader / EyeShader

MAX_TEXTURES = 16
FLAT, GOURAUD, PHONG, EYE, CHECKER = 0, 1, 2, 3, 4
VARY = {FLAT: 0, GOURAUD: 3, PHONG: 24, EYE: 24, CHECKER: 0}


class Uniforms(C.Structure):
    _fields_ = [("model_view", C.c_double * 16), ("key_light_dir_eye", C.c_double * 3),
                ("fill_light_dir_eye", C.c_double * 3), ("rim_light_dir_eye", C.c_double * 3),
                ("normal_map_strength", C.c_double), ("tex_diffuse", C.c_int32), ("tex_normal", C.c_int32),
                ("tex_specular", C.c_int32), ("reserved", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("triangles_rasterized", C.c_uint64), ("fragments_drawn", C.c_uint64),
                ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32),
                ("min_z", C.c_double), ("max_z", C.c_double)]

    def astuple(self):
        # z range as (value, sign bit) so that -0.0 and +0.0 compare unequal, as their printed forms do
        import math
        return (self.triangles_rasterized, self.fragments_drawn, self.min_x, self.min_y, self.max_x, self.max_y,
                self.min_z, self.max_z, math.copysign(1.0, self.min_z), math.copysign(1.0, self.max_z))


class Texture(C.Structure):
    _fields_ = [("data", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("bpp", C.c_int)]


class Target(C.Structure):
    _fields_ = [("fb", C.c_void_p), ("zbuf", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("bpp", C.c_int),
                ("clip_y0", C.c_int), ("clip_y1", C.c_int), ("viewport", C.c_double * 16), ("stats", Stats)]


def make_uniforms(model_view=None, key=(0, 0, 1), fill=(0, 0, 1), rim=(0, 0, 1), normal_map_strength=1.0,
                  tex_diffuse=-1, tex_normal=-1, tex_specular=-1, cells=0) -> Uniforms:
    u = Uniforms()
    mv = np.eye(4) if model_view is None else np.asarray(model_view, np.float64)
    u.model_view[:] = mv.reshape(16).tolist()
    u.key_light_dir_eye[:] = list(map(float, key))
    u.fill_light_dir_eye[:] = list(map(float, fill))
    u.rim_light_dir_eye[:] = list(map(float, rim))
    u.normal_map_strength = float(normal_map_strength)
    u.tex_diffuse, u.tex_normal, u.tex_specular, u.reserved = tex_diffuse, tex_normal, tex_specular, int(cells)      # cells: CHECKER only
    return u


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C oracle` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.orc_init_viewport.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int]
        L.orc_stats_init.argtypes = [C.POINTER(Stats)]
        L.orc_clear.argtypes = [C.POINTER(Target), C.c_void_p, C.c_double]
        L.orc_rasterize.argtypes = [C.POINTER(Target), C.c_int, C.POINTER(Uniforms), C.POINTER(Texture),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.orc_fragment.argtypes = [C.c_int, C.POINTER(Uniforms), C.POINTER(Texture), C.c_void_p, C.c_uint32,
                                   C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        L.orc_fragment.restype = C.c_int
        L.orc_tex_fetch.argtypes = [C.POINTER(Texture), C.c_void_p, C.c_void_p]
        L.orc_tex_fetch.restype = C.c_int
        L.orc_normalized3.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_mat4_mul_dir.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_interp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.orc_tga_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.orc_tga_encode.restype = C.c_uint64
        L.orc_tga_decode.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_uint64]
        L.orc_tga_decode.restype = C.c_int
        L.orc_vertex_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.orc_zbuffer_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.orc_ssao.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.orc_composite.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


class Oracle:
    """A framebuffer + z-buffer + stats driven through the CPU restatement."""

    def __init__(self, width, height, bpp=3, viewport=None, clear_bgra=None, z_clear=np.inf, strip=None):
        self.L = lib()
        self.w, self.h, self.bpp = width, height, bpp
        self.fb = np.zeros((height, width, bpp), np.uint8)
        self.z = np.empty((height, width), np.float64)
        self.t = Target()
        self.t.fb, self.t.zbuf = self.fb.ctypes.data, self.z.ctypes.data
        self.t.w, self.t.h, self.t.bpp = width, height, bpp
        self.t.clip_y0, self.t.clip_y1 = (0, height) if strip is None else strip
        vp = np.asarray(viewport, np.float64).reshape(16) if viewport is not None else None
        if vp is None:
            self.L.orc_init_viewport(self.t.viewport, 0, 0, width, height)
        else:
            self.t.viewport[:] = vp.tolist()
        self.L.orc_stats_init(C.byref(self.t.stats))
        self.textures = (Texture * MAX_TEXTURES)()
        self._tex_keep = {}
        cb = None if clear_bgra is None else np.asarray(clear_bgra, np.uint8)
        self.L.orc_clear(C.byref(self.t), None if cb is None else cb.ctypes.data, float(z_clear))

    # ---- the reference's globals, changed between rasterize() calls (each takes effect at once: the reference is immediate) ----
    def set_viewport(self, m):
        """The global Viewport (our_gl.cpp:14) as a row-major 4x4."""
        self.t.viewport[:] = np.asarray(m, np.float64).reshape(16).tolist()

    def clear(self, clear_bgra=None, z_clear=np.inf):
        """A fresh TGAImage(w, h, bpp, clear) and init_zbuffer (tgaimage.cpp:8-17, our_gl.cpp:72-74): every row, whatever the strip."""
        cb = None if clear_bgra is None else np.asarray(clear_bgra, np.uint8)
        self.L.orc_clear(C.byref(self.t), None if cb is None else cb.ctypes.data, float(z_clear))

    def reset_stats(self):
        """The counters back to their initial values (our_gl.cpp:18-22)."""
        self.L.orc_stats_init(C.byref(self.t.stats))

    def set_strip(self, y0, y1):
        """Later draws write rows [y0, y1) only (they still count and bound every triangle)."""
        self.t.clip_y0, self.t.clip_y1 = int(y0), int(y1)

    def upload_texture(self, slot, texels):
        t = np.ascontiguousarray(texels, np.uint8)
        if t.ndim == 2:
            t = t[..., None]
        self._tex_keep[slot] = t
        self.textures[slot] = Texture(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])

    def draw(self, kind, clip, varyings=None, colors=None, uniforms=None):
        clip = np.ascontiguousarray(clip, np.float64)
        n = clip.shape[0]
        K = VARY[kind]
        v = None if K == 0 else np.ascontiguousarray(varyings, np.float64)
        if v is not None:
            assert v.shape == (n, K), v.shape
        c = None if colors is None else np.ascontiguousarray(colors, np.uint32)
        u = uniforms if uniforms is not None else make_uniforms()
        self.L.orc_rasterize(C.byref(self.t), kind, C.byref(u), self.textures, clip.ctypes.data,
                             None if v is None else v.ctypes.data, None if c is None else c.ctypes.data, n)

    @property
    def stats(self):
        return self.t.stats.astuple()


# ---------------------------------------------------------------------------------------------
# reference harness (build container only)
# ---------------------------------------------------------------------------------------------
def ref_available() -> bool:
    return os.path.exists(REF_HARNESS) and os.path.exists(REF_SHADERS)


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * ((8 - len(b) % 8) % 8)


def write_scene(path, width, height, bpp, viewport, draws, textures=None, clear_bgra=(0, 0, 0, 255), z_clear=np.inf):
    """draws: list of (kind, Uniforms|None, clip, varyings|None, colors|None); textures: {slot: array}."""
    textures = textures or {}
    with open(path, "wb") as f:
        f.write(b"TRGSCN01")
        f.write(struct.pack("<6i", width, height, bpp, len(draws), len(textures), 0))
        f.write(np.asarray(viewport, np.float64).reshape(16).tobytes())
        f.write(bytes(bytearray(clear_bgra)) + b"\0\0\0\0")
        f.write(struct.pack("<d", float(z_clear)))
        for slot, t in textures.items():
            t = np.ascontiguousarray(t, np.uint8)
            if t.ndim == 2:
                t = t[..., None]
            f.write(struct.pack("<4i", slot, t.shape[1], t.shape[0], t.shape[2]))
            f.write(_pad8(t.tobytes()))
        for kind, u, clip, vary, colors in draws:
            clip = np.ascontiguousarray(clip, np.float64)
            n = clip.shape[0]
            f.write(struct.pack("<iiQ", kind, 0, n))
            f.write(bytes(u if u is not None else make_uniforms()))
            f.write(clip.tobytes())
            if VARY[kind]:
                f.write(np.ascontiguousarray(vary, np.float64).tobytes())
            cols = np.ascontiguousarray(colors, np.uint32) if colors is not None else np.full(n, 0xFFFFFFFF, np.uint32)
            f.write(_pad8(cols.tobytes()))


def parse_stats_line(line: str):
    """'DEBUG: triangles=N fragments_drawn=M bbox=[a,b] - [c,d] z-range=[lo,hi]' (our_gl.cpp:205-209)."""
    import re
    m = re.search(r"triangles=(\d+) fragments_drawn=(\d+) bbox=\[(-?\d+),(-?\d+)\] - \[(-?\d+),(-?\d+)\] z-range=\[([^,]+),([^\]]+)\]", line)
    tri, frag, x0, y0, x1, y1 = (int(m.group(i)) for i in range(1, 7))
    return tri, frag, x0, y0, x1, y1, m.group(7), m.group(8)


def run_reference(width, height, bpp, viewport, draws, textures=None, clear_bgra=(0, 0, 0, 255), z_clear=np.inf,
                  harness=None, with_time=False):
    """Render with the reference's own rasterize(); returns (fb[h,w,bpp] u8, z[h,w] f64, stats line)
    [+ seconds spent in the rasterize() loops when with_time].  A scene with a PHONG or EYE draw goes to ref_shaders (the
    reference's own PhongShader / EyeShader), any other to ref_harness, unless `harness` names one."""
    if harness is None:
        harness = REF_SHADERS if any(d[0] in (PHONG, EYE) for d in draws) else REF_HARNESS
    with tempfile.TemporaryDirectory() as d:
        sp, op = os.path.join(d, "scene.bin"), os.path.join(d, "out.bin")
        write_scene(sp, width, height, bpp, viewport, draws, textures, clear_bgra, z_clear)
        subprocess.run([harness, "scene", sp, op], check=True)
        raw = open(op, "rb").read()
    return _parse_frame(raw, 0, width, height, bpp, with_time)


def _parse_frame(raw, off, width, height, bpp, with_time=False):
    nfb = width * height * bpp
    fb = np.frombuffer(raw, np.uint8, nfb, off).reshape(height, width, bpp).copy()
    off += (nfb + 7) & ~7
    z = np.frombuffer(raw, np.float64, width * height, off).reshape(height, width).copy()
    off += width * height * 8
    (ln,) = struct.unpack_from("<i", raw, off)
    line = raw[off + 4: off + 4 + ln].decode()
    if with_time:
        toff = off + ((4 + ln + 7) & ~7)
        (secs,) = struct.unpack_from("<d", raw, toff)
        return fb, z, line.strip(), secs
    return fb, z, line.strip()


def format_stats_line(stats_tuple) -> str:
    """The print_render_stats() line (our_gl.cpp:205-209) for an oracle/GPU stats tuple."""
    tri, frag, x0, y0, x1, y1, zlo, zhi = stats_tuple[:8]
    lo = f"{zlo:.6f}" if np.isfinite(zlo) else "inf"
    hi = f"{zhi:.6f}" if np.isfinite(zhi) else "-inf"
    return f"DEBUG: triangles={tri} fragments_drawn={frag} bbox=[{x0},{y0}] - [{x1},{y1}] z-range=[{lo},{hi}]"


def tga_encode(img: np.ndarray, vflip=True, rle=True) -> bytes:
    """TGAImage::write_tga_file bytes for an [h,w,bpp] uint8 image, via the C restatement."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = img.shape
    out = np.empty(18 + img.size + w * h + 16, np.uint8)
    n = lib().orc_tga_encode(img.ctypes.data, w, h, bpp, int(vflip), int(rle), out.ctypes.data)
    return out[:n].tobytes()


def run_reference_tga(img: np.ndarray, vflip=True, rle=True) -> bytes:
    """The file the reference's own TGAImage::write_tga_file writes (build container only)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = img.shape
    with tempfile.TemporaryDirectory() as d:
        ip, op = os.path.join(d, "in.bin"), os.path.join(d, "out.tga")
        with open(ip, "wb") as f:
            f.write(struct.pack("<6i", w, h, bpp, int(vflip), int(rle), 0))
            f.write(img.tobytes())
        subprocess.run([REF_HARNESS, "tga", ip, op], check=True)
        return open(op, "rb").read()


def tga_decode(file_bytes: bytes):
    """TGAImage::read_tga_file on a file image, via the C restatement: [h,w,bpp] uint8, or None where it returns false."""
    buf = np.frombuffer(file_bytes, np.uint8)
    w, h, bpp = C.c_int(), C.c_int(), C.c_int()
    cap = 16 if len(buf) < 18 else (int(buf[12]) | (int(buf[13]) << 8)) * (int(buf[14]) | (int(buf[15]) << 8)) * 4 + 16
    out = np.empty(cap, np.uint8)
    ok = lib().orc_tga_decode(buf.ctypes.data if len(buf) else None, len(buf), C.byref(w), C.byref(h), C.byref(bpp), out.ctypes.data, out.size)
    if not ok:
        return None
    return out[:w.value * h.value * bpp.value].reshape(h.value, w.value, bpp.value).copy()


def run_reference_tga_read(file_bytes: bytes):
    """What the reference's own TGAImage::read_tga_file makes of the file (build container only): array or None."""
    with tempfile.TemporaryDirectory() as d:
        ip, op = os.path.join(d, "in.tga"), os.path.join(d, "out.bin")
        open(ip, "wb").write(file_bytes)
        subprocess.run([REF_HARNESS, "tgaread", ip, op], check=True, stderr=subprocess.DEVNULL)
        raw = open(op, "rb").read()
    ok, w, h, bpp = struct.unpack("<4i", raw[:16])
    if not ok:
        return None
    return np.frombuffer(raw[16:], np.uint8).reshape(h, w, bpp).copy()


def vertex_stage(model_view, projection, vertices, indices):
    """main.cpp:71-90 for an indexed mesh; vertices [nv, stride>=8] (pos3, nrm3, uv2, ...), indices [nf,3] uint32."""
    mv = np.ascontiguousarray(model_view, np.float64).reshape(16)
    pj = np.ascontiguousarray(projection, np.float64).reshape(16)
    v = np.ascontiguousarray(vertices, np.float64)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    nf = idx.shape[0]
    clip, vary = np.empty((nf, 12)), np.empty((nf, 24))
    lib().orc_vertex_stage(mv.ctypes.data, pj.ctypes.data, v.ctypes.data, v.shape[1], idx.ctypes.data, nf, clip.ctypes.data, vary.ctypes.data)
    return clip, vary


def zbuffer_image(z):
    z = np.ascontiguousarray(z, np.float64); h, w = z.shape
    out = np.empty((h, w, 3), np.uint8); lib().orc_zbuffer_image(z.ctypes.data, w, h, out.ctypes.data); return out


def ssao(z):
    z = np.ascontiguousarray(z, np.float64); h, w = z.shape
    out = np.empty((h, w, 3), np.uint8); lib().orc_ssao(z.ctypes.data, w, h, out.ctypes.data); return out


def composite(fb, ao):
    fb = np.ascontiguousarray(fb, np.uint8); ao = np.ascontiguousarray(ao, np.uint8); h, w, _ = fb.shape
    out = np.empty((h, w, 3), np.uint8); lib().orc_composite(fb.ctypes.data, ao.ctypes.data, w, h, out.ctypes.data); return out


def tex_fetch(texels, uv):
    """The samplers' nearest-texel fetch (model.cpp:415-425) through the C restatement: [n, 5] uint8 = bgra[4], bytespp."""
    t = np.ascontiguousarray(texels, np.uint8)
    if t.ndim == 2:
        t = t[..., None]
    tex = Texture(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    out = np.zeros((uv.shape[0], 5), np.uint8)
    px = np.zeros(4, np.uint8)
    for i in range(uv.shape[0]):
        out[i, 4] = lib().orc_tex_fetch(C.byref(tex), uv[i].ctypes.data, px.ctypes.data)
        out[i, :4] = px
    return out


def run_reference_sample2d(texels, uv):
    """IShader::sample2D (our_gl.h:38-44) of the compiled reference on a texture and uv list (build container only): [n, 5] uint8."""
    t = np.ascontiguousarray(texels, np.uint8)
    if t.ndim == 2:
        t = t[..., None]
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    with tempfile.TemporaryDirectory() as d:
        ip, op = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(ip, "wb") as f:
            f.write(struct.pack("<4i", t.shape[1], t.shape[0], t.shape[2], uv.shape[0]))
            f.write(_pad8(t.tobytes()))
            f.write(uv.tobytes())
        subprocess.run([REF_HARNESS, "sample2d", ip, op], check=True)
        raw = np.frombuffer(open(op, "rb").read(), np.uint8).reshape(-1, 8)
    return raw[:, :5].copy()


# ---- oracle/_ref/ref_shaders: the reference's own main.cpp / model.cpp code (build container only) ----------------------------
def _write_textures(f, textures):
    for slot, t in textures.items():
        t = np.ascontiguousarray(t, np.uint8)
        if t.ndim == 2:
            t = t[..., None]
        f.write(struct.pack("<4i", slot, t.shape[1], t.shape[0], t.shape[2]))
        f.write(_pad8(t.tobytes()))


def _run_ref_shaders(mode, payload: bytes) -> bytes:
    with tempfile.TemporaryDirectory() as d:
        ip, op = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        open(ip, "wb").write(payload)
        subprocess.run([REF_SHADERS, mode, ip, op], check=True, stderr=subprocess.DEVNULL)
        return open(op, "rb").read()


def run_reference_fragments(textures, kinds, uniforms, varyings, bary):
    """PhongShader / EyeShader ::fragment (main.cpp:92-170, 220-261) of the compiled reference, one call per row: kinds [n],
    uniforms [n] (Uniforms), varyings [n, 24], bary [n, 3].  Returns [n, 5] uint8: bgra[4], bytespp."""
    import io
    varyings = np.ascontiguousarray(varyings, np.float64)
    bary = np.ascontiguousarray(bary, np.float64)
    f = io.BytesIO()
    f.write(b"TRGFRG01" + struct.pack("<2i", len(textures), len(kinds)))
    _write_textures(f, textures)
    for i, k in enumerate(kinds):
        f.write(struct.pack("<2i", int(k), 0) + bytes(uniforms[i]) + varyings[i].tobytes() + bary[i].tobytes())
    raw = np.frombuffer(_run_ref_shaders("frag", f.getvalue()), np.uint8).reshape(-1, 8)
    assert not raw[:, 5].any(), "a PHONG / EYE fragment discarded"
    return raw[:, :5].copy()


def fragments(textures, kinds, uniforms, varyings, bary):
    """orc_fragment (the restatement) over the same rows as run_reference_fragments: [n, 5] uint8."""
    tex = (Texture * MAX_TEXTURES)()
    keep = []
    for slot, t in textures.items():
        t = np.ascontiguousarray(t, np.uint8)
        t = t[..., None] if t.ndim == 2 else t
        keep.append(t)
        tex[slot] = Texture(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])
    varyings = np.ascontiguousarray(varyings, np.float64)
    bary = np.ascontiguousarray(bary, np.float64)
    out = np.zeros((len(kinds), 5), np.uint8)
    px = (C.c_uint8 * 4)()
    L = lib()
    for i, k in enumerate(kinds):
        b = (C.c_double * 3)(*bary[i])
        u = Uniforms.from_buffer_copy(bytes(uniforms[i]))
        out[i, 4] = L.orc_fragment(int(k), C.byref(u), tex, varyings[i].ctypes.data, 0, b, px)
        out[i, :4] = np.frombuffer(bytes(px), np.uint8)
    return out


def run_reference_lights(model_views, key, fill, rim):
    """PhongShader::initLightDirections(key, fill, rim) and EyeShader::initLightDirections(key, rim) (main.cpp:55-69, 187-197)
    of the compiled reference: model_views [n, 16], world directions [n, 3] each.  Returns [n, 15] f64: Phong key, fill, rim,
    Eye key, rim (eye space)."""
    mv = np.ascontiguousarray(model_views, np.float64).reshape(-1, 16)
    rows = np.concatenate([mv, np.asarray(key, np.float64), np.asarray(fill, np.float64), np.asarray(rim, np.float64)], 1)
    raw = _run_ref_shaders("lights", struct.pack("<2i", rows.shape[0], 0) + np.ascontiguousarray(rows).tobytes())
    return np.frombuffer(raw, np.float64).reshape(-1, 15).copy()


def run_reference_mesh(width, height, bpp, kind, viewport, projection, uniforms, vertices, indices, textures=None):
    """A mesh through the reference's Model::load (via the Assimp stand-ins) and shader.vertex(f, v) for every face
    (main.cpp:71-90 / 199-218), then rasterize() of each face as main.cpp:692-698.  vertices [nv, 8] float32 (position,
    normal, uv), indices [nf, 3].  Returns (clip [nf, 12], varyings [nf, 24], fb, z, stats line)."""
    import io
    textures = textures or {}
    v = np.ascontiguousarray(vertices, np.float32)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    f = io.BytesIO()
    f.write(b"TRGMSH01" + struct.pack("<8i", width, height, bpp, kind, len(textures), v.shape[0], idx.shape[0], 0))
    f.write(np.asarray(viewport, np.float64).reshape(16).tobytes() + np.asarray(projection, np.float64).reshape(16).tobytes())
    f.write(bytes(uniforms))
    _write_textures(f, textures)
    f.write(v.tobytes() + idx.tobytes())
    raw = _run_ref_shaders("mesh", f.getvalue())
    nf = idx.shape[0]
    clip = np.frombuffer(raw, np.float64, nf * 12).reshape(nf, 12).copy()
    vary = np.frombuffer(raw, np.float64, nf * 24, nf * 96).reshape(nf, 24).copy()
    fb, z, line = _parse_frame(raw, nf * 288, width, height, bpp)
    return clip, vary, fb, z, line


def run_reference_zbuffer_image(z):
    """save_zbuffer_image (main.cpp:269-314) of the compiled reference, read back with TGAImage::read_tga_file: [h, w, 3] uint8."""
    z = np.ascontiguousarray(z, np.float64); h, w = z.shape
    raw = _run_ref_shaders("zimage", struct.pack("<2i", w, h) + z.tobytes())
    return np.frombuffer(raw, np.uint8).reshape(h, w, 3).copy()


def run_reference_ssao(z):
    """compute_ssao_at (main.cpp:324-362) in the loop of main.cpp:756-763, compiled reference: [h, w, 3] uint8."""
    z = np.ascontiguousarray(z, np.float64); h, w = z.shape
    raw = _run_ref_shaders("ssao", struct.pack("<2i", w, h) + z.tobytes())
    return np.frombuffer(raw, np.uint8).reshape(h, w, 3).copy()
