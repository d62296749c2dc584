"""Context: one rasterizer context on one GPU - lifetime, state, draw() and draw_indexed(), the flush, read-back, stats and the debug
hooks of a flush.  The methods of each family come from the family's module."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .clip import _ClipCalls, _clip_attrs
from .edges import _EdgeCalls
from .images import _ImageCalls
from .instances import _InstanceCalls
from .loader import (DBG_BMASK, DBG_CNT, DBG_INFO, DBG_INFO_FIELDS, DBG_RECS, DBG_TILE_END, DBG_TILE_START, DBG_TILEBOX, DBG_VALS, MEM_DEVICE,
                     MEM_HOST, NUM_PHASES, SAMPLE_TRILINEAR, SHADER_USER_FIRST, TRI_REC, VARY, Stats, load_library)
from .marshal import _check, _device_ptr, _dp, _f64, _failure, _mem, _ptr, _ref
from .mesh import _MeshCalls
from .order import _OrderCalls
from .quads import _QuadCalls
from .rccl import _RcclCalls
from .shaders import _ShaderCalls
from .shadow import _ShadowCalls
from .skin import _SkinCalls
from .subdiv import _SubdivCalls
from .weld import _WeldCalls


class Context(_ImageCalls, _ShadowCalls, _ClipCalls, _InstanceCalls, _OrderCalls, _QuadCalls, _EdgeCalls, _SubdivCalls, _WeldCalls, _SkinCalls,
              _MeshCalls, _RcclCalls, _ShaderCalls):
    """One rasterizer context on one GPU — the reference's globals (Viewport, zbuffer, counters,
    our_gl.cpp:12-22) plus the framebuffer TGAImage, as an object."""

    def __init__(self, width: int, height: int, bpp: int = 3, device: int = 0):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L, None, "trgl_create", self.L.trgl_create(device, width, height, bpp, C.byref(self.h)))
        self.width, self.height, self.bpp, self.device = width, height, bpp, device
        self._keep = []
        self._user_vary = {}        # kind -> K of the user shaders registered here
        self._vertex_vary = {}      # vertex shader -> K of the user vertex shaders registered here

    def _chk(self, rc):
        if rc != 0:
            raise _failure("trgl call", rc, self.L.trgl_last_error(self.h).decode())

    def _hold(self, device, arrays):
        """Keep the arrays of a device=True call alive until the next sync or read-back: the stream reads them after the call returns."""
        if device:
            self._keep.append(arrays)

    def close(self):
        if self.h:
            self.L.trgl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state ----
    def set_viewport(self, m):
        m = np.ascontiguousarray(m, np.float64).reshape(16)
        self._chk(self.L.trgl_set_viewport(self.h, _dp(m)))

    def init_viewport(self, x, y, w, h):
        self._chk(self.L.trgl_init_viewport(self.h, x, y, w, h))

    def clear(self, bgra=None, z=np.inf):
        b = None if bgra is None else np.asarray(bgra, np.uint8)
        self._chk(self.L.trgl_clear(self.h, None if b is None else b.ctypes.data, float(z)))

    def upload_texture(self, slot, texels):
        t = np.ascontiguousarray(texels, np.uint8)
        if t.ndim == 2:
            t = t[..., None]
        self._chk(self.L.trgl_upload_texture(self.h, slot, t.ctypes.data, t.shape[1], t.shape[0], t.shape[2]))

    def set_strip(self, y0, y1):
        self._chk(self.L.trgl_set_strip(self.h, y0, y1))

    def set_interleave(self, band_rows, rank, world):
        """Own the bands of `band_rows` rows whose number is `rank` modulo `world` (instead of one strip)."""
        self._chk(self.L.trgl_set_interleave(self.h, band_rows, rank, world))

    # ---- submission ----
    def draw(self, kind, clip, varyings=None, colors=None, uniforms=None, n=None, device=False, clip_plane=None, clip_attrs=None,
             order=None, order_device=False, group=1):
        """order: a list of groups of `group` consecutive triangles - the groups it names are drawn, in its order (trgl_draw_ordered; no
        wait).  A numpy array, or with order_device=True a 32-bit integer device tensor such as Context.depth_order(device=True) returns;
        device arrays of such a draw are read when the call's gather runs on the stream, not at the flush.  Not with clip_plane.
        clip_plane: four doubles - the list is cut against that plane first (trgl_draw_clipped; the call waits for the stream once, for
        the count of output triangles), with clip_attrs a list of (offset, components) or None for the kind's built-in layout.
        Host arrays (numpy) are copied before return; with device=True pass torch CUDA tensors (or raw
        pointers with n) that stay alive until the flush has completed: every array of such a draw, a host array
        among them is a TypeError (_device_ptr).  include/trgl.h, TRGL_MEM_DEVICE: alignment and stream ordering."""
        # (a kind in the user range that was not registered here goes to the library, which refuses it)
        K = self._user_vary.get(kind, 0) if kind >= SHADER_USER_FIRST else VARY[kind]
        if not device:
            clip = np.ascontiguousarray(clip, np.float64)
            n = clip.shape[0] if n is None else n
            if K:
                varyings = np.ascontiguousarray(varyings, np.float64)
                assert varyings.shape == (n, K), varyings.shape
            if colors is not None:
                colors = np.ascontiguousarray(colors, np.uint32)
                assert colors.shape == (n,)
            ptrs = (_ptr(clip), _ptr(varyings) if K else None, _ptr(colors))
        else:
            ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings"), _device_ptr(colors, "colors"))
            if not K:
                ptrs = (ptrs[0], None, ptrs[2])
            assert n is not None or hasattr(clip, "shape")
            n = clip.shape[0] if n is None else n
            self._hold(True, (clip, varyings, colors))
        if order is not None:
            assert clip_plane is None and clip_attrs is None, "order=: not with clip_plane="
            oargs, _, keep = self._order_args(order, order_device)
            self._hold(order_device, keep)
            self._chk(self.L.trgl_draw_ordered(self.h, kind, _ref(uniforms), ptrs[0], ptrs[1], ptrs[2], int(n), _mem(device), oargs[0], oargs[1], int(group),
                                               oargs[2]))
            return
        if clip_plane is not None:
            arr, na = _clip_attrs(clip_attrs)
            self._chk(self.L.trgl_draw_clipped(self.h, kind, _ref(uniforms), _dp(_f64(clip_plane, 4, "clip_plane")), arr, na, ptrs[0], ptrs[1], ptrs[2],
                                               int(n), _mem(device)))
            return
        assert clip_attrs is None, "clip_attrs: only with clip_plane="
        self._chk(self.L.trgl_draw(self.h, kind, _ref(uniforms), ptrs[0], ptrs[1], ptrs[2], int(n), _mem(device)))

    def _mesh_ptrs(self, vertices, indices, colors, device):
        """The arrays of an indexed mesh as (vertices, indices, colors, their three addresses): host arrays made contiguous, device
        arrays checked by _device_ptr before anything reaches the library."""
        if not device:
            vertices = np.ascontiguousarray(vertices, np.float64)
            indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
            if colors is not None:
                colors = np.ascontiguousarray(colors, np.uint32)
                assert colors.shape == (indices.shape[0],), colors.shape
            return vertices, indices, colors, (_ptr(vertices), _ptr(indices), _ptr(colors))
        return vertices, indices, colors, (_device_ptr(vertices, "vertices"), _device_ptr(indices, "indices"), _device_ptr(colors, "colors"))

    def _order_args(self, order, order_device):
        """The three order arguments of the ordered calls as (ctypes arguments, n_order, what to keep alive)."""
        if order_device:
            if str(getattr(order, "dtype", "")) not in ("torch.int32", "torch.uint32") or not order.is_contiguous() or order.dim() != 1:
                raise ValueError("order_device=True: order must be a contiguous 32-bit integer device tensor [n_order]")
            n = int(order.shape[0])
            return [_device_ptr(order, "order") if n else None, n, MEM_DEVICE], n, order
        order = np.ascontiguousarray(order, np.uint32).reshape(-1)
        return [order.ctypes.data if order.size else None, int(order.size), MEM_HOST], int(order.size), order

    def draw_indexed(self, kind, uniforms, projection, vertices, indices, device=False, vertex_shader=None, colors=None,
                     clip_plane=None, clip_attrs=None):
        """clip_plane / clip_attrs: as for draw() - the faces are cut between the vertex stage and the draw (trgl_draw_indexed_vs_clipped).
        Vertex stage on the device (main.cpp:71-90) + draw.  vertices [nv, stride>=8] f64, indices [nf,3] u32.
        vertex_shader: a number from register_vertex_shader - its trgl_vertex runs in place of the built-in stage
        (trgl_draw_indexed_vs): any `kind` with the vertex shader's K, vertices [nv, stride>=1] in the layout the shader reads,
        uniforms None where draw() allows it, colors [nf] u32 per face or None."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        if clip_plane is not None:
            assert vertex_shader is not None or colors is None, "colors: only with vertex_shader="
            vertices, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
            self._hold(device, (vertices, indices, colors))
            arr, na = _clip_attrs(clip_attrs)
            self._chk(self.L.trgl_draw_indexed_vs_clipped(self.h, -1 if vertex_shader is None else int(vertex_shader), kind, _ref(uniforms), _dp(pj),
                                                          _dp(_f64(clip_plane, 4, "clip_plane")), arr, na, ptrs[0], vertices.shape[1], vertices.shape[0],
                                                          ptrs[1], indices.shape[0], ptrs[2], _mem(device)))
            return
        assert clip_attrs is None, "clip_attrs: only with clip_plane="
        if vertex_shader is not None:
            vertices, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
            self._hold(device, (vertices, indices, colors))
            nv, stride = vertices.shape
            nf = indices.shape[0]
            self._chk(self.L.trgl_draw_indexed_vs(self.h, int(vertex_shader), kind, _ref(uniforms), _dp(pj), ptrs[0], stride, nv, ptrs[1], nf, ptrs[2],
                                                  _mem(device)))
            return
        assert colors is None, "colors: only with vertex_shader="
        vertices, indices, _, ptrs = self._mesh_ptrs(vertices, indices, None, device)
        self._hold(device, (vertices, indices))
        nv, stride = vertices.shape
        nf = indices.shape[0]
        self._chk(self.L.trgl_draw_indexed(self.h, kind, C.byref(uniforms), _dp(pj), ptrs[0], stride, nv, ptrs[1], nf, _mem(device)))

    def postprocess(self, zbuffer_image=True, ao=True, final=True, params=None):
        """main.cpp:269-311,317-362,757-783 on the device; returns dict of [h,w,3] uint8 images."""
        out = {}
        shape = (self.height, self.width, 3)
        zi = np.empty(shape, np.uint8) if zbuffer_image else None
        a = np.empty(shape, np.uint8) if ao else None
        f = np.empty(shape, np.uint8) if final else None
        self._chk(self.L.trgl_postprocess(self.h, _ref(params), None if zi is None else zi.ctypes.data, None if a is None else a.ctypes.data,
                                          None if f is None else f.ctypes.data))
        return dict(zbuffer_image=zi, ao=a, final=f)

    def flush(self):
        self._chk(self.L.trgl_flush(self.h))

    def flush_begin(self):
        """Setup + binning of what was submitted (does not touch the framebuffer / z-buffer); flush_end() runs the raster."""
        self._chk(self.L.trgl_flush_begin(self.h))

    def flush_end(self):
        self._chk(self.L.trgl_flush_end(self.h))

    def sync(self):
        self._chk(self.L.trgl_sync(self.h))
        self._keep.clear()

    # ---- results ----
    def read_framebuffer(self) -> np.ndarray:
        out = np.empty((self.height, self.width, self.bpp), np.uint8)
        self._chk(self.L.trgl_read_framebuffer(self.h, out.ctypes.data))
        self._keep.clear()
        return out

    def read_zbuffer(self) -> np.ndarray:
        out = np.empty((self.height, self.width), np.float64)
        self._chk(self.L.trgl_read_zbuffer(self.h, out.ctypes.data))
        self._keep.clear()
        return out

    def write_framebuffer(self, fb):
        fb = np.ascontiguousarray(fb, np.uint8)
        assert fb.size == self.width * self.height * self.bpp
        self._chk(self.L.trgl_write_framebuffer(self.h, fb.ctypes.data))

    def write_zbuffer(self, z):
        z = np.ascontiguousarray(z, np.float64)
        assert z.size == self.width * self.height
        self._chk(self.L.trgl_write_zbuffer(self.h, z.ctypes.data))

    def stats(self):
        s = Stats()
        self._chk(self.L.trgl_get_stats(self.h, C.byref(s)))
        return s.astuple()

    def stats_line(self) -> str:
        s = Stats()
        self._chk(self.L.trgl_get_stats(self.h, C.byref(s)))
        buf = C.create_string_buffer(1024)
        self._chk(self.L.trgl_format_stats(C.byref(s), buf, 1024))
        return buf.value.decode().strip()

    def reset_stats(self):
        self._chk(self.L.trgl_reset_stats(self.h))

    @property
    def framebuffer_ptr(self) -> int:
        return self.L.trgl_framebuffer_device_ptr(self.h)

    @property
    def zbuffer_ptr(self) -> int:
        return self.L.trgl_zbuffer_device_ptr(self.h)

    @property
    def stream(self) -> int:
        return self.L.trgl_stream(self.h)

    def set_stream(self, hip_stream, use_own: bool = False):
        """Enqueue on the caller's hipStream_t (int handle, e.g. torch.cuda.current_stream().cuda_stream; 0 is the
        legacy default stream).  use_own=True returns to the context's own stream."""
        self._chk(self.L.trgl_set_stream(self.h, hip_stream or None, 1 if use_own else 0))

    # ---- measurement ----
    def set_profiling(self, on: bool):
        self._chk(self.L.trgl_set_profiling(self.h, 1 if on else 0))

    def phase_ms(self):
        ms = (C.c_double * NUM_PHASES)()
        n = C.c_uint64()
        self._chk(self.L.trgl_get_phase_ms(self.h, ms, C.byref(n)))
        return list(ms), n.value

    def reset_phase_ms(self):
        self._chk(self.L.trgl_reset_phase_ms(self.h))

    def selftest_division(self, samples: int, seed: int = 1) -> int:
        bad = C.c_uint64()
        self._chk(self.L.trgl_selftest_division(self.h, samples, seed, C.byref(bad)))
        return bad.value

    def selftest_sampler(self, slot: int, uv) -> np.ndarray:
        """The device samplers' texel fetch of texture `slot` at uv [n,2]: [n,5] uint8 = bgra[4], bytespp."""
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        out = np.zeros((uv.shape[0], 5), np.uint8)
        self._chk(self.L.trgl_selftest_sampler(self.h, slot, uv.ctypes.data, uv.shape[0], out.ctypes.data))
        return out

    def selftest_sampler_lod(self, slot: int, uv, lod, mode=SAMPLE_TRILINEAR) -> np.ndarray:
        """The filtered device samplers of the user shaders on texture `slot` at uv [n,2] and lod [n] (mode SAMPLE_LEVEL, SAMPLE_LINEAR:
        lod converted to int; SAMPLE_TRILINEAR): [n,5] uint8 = bgra[4], bytespp."""
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        lod = np.ascontiguousarray(np.broadcast_to(np.asarray(lod, np.float64), (uv.shape[0],)))
        out = np.zeros((uv.shape[0], 5), np.uint8)
        self._chk(self.L.trgl_selftest_sampler_lod(self.h, int(slot), uv.ctypes.data, lod.ctypes.data, int(mode), uv.shape[0], out.ctypes.data))
        return out

    def last_flush_info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.trgl_get_last_flush_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(triangles=a.value, pairs=b.value, tiles=c.value)

    def debug_binning(self, mode=None, S=0, G=0):
        """Test hook (trgl_debug_binning).  mode BIN_AUTO / BIN_EXPAND / BIN_DIRECT (with segments of S pair slots and groups of G
        setup blocks) sets how the next flushes bin; None changes nothing.  Returns what the last complete flush did:
        dict(direct=..., fell_back=...)."""
        d, f = C.c_int(), C.c_int()
        self._chk(self.L.trgl_debug_binning(self.h, -1 if mode is None else mode, S, G, C.byref(d), C.byref(f)))
        return dict(direct=bool(d.value), fell_back=bool(f.value))

    def debug_radix_blocks(self, n=None):
        """Test hook (trgl_debug_radix_blocks).  n caps the grids of the radix scatters of the next flushes (0: automatic, as many
        blocks as the device holds at once; every block walks its chunks with a stride of the grid); None changes nothing.  Returns
        the grids of the last binning queued: dict(first=..., last=...)."""
        if n is not None:
            self._radix_blocks = int(n)
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.trgl_debug_radix_blocks(self.h, getattr(self, "_radix_blocks", 0), C.byref(a), C.byref(b)))
        return dict(first=a.value, last=b.value)

    def _debug_read(self, what, dtype):
        need = C.c_size_t()
        self._chk(self.L.trgl_debug_read(self.h, what, None, 0, C.byref(need)))
        out = np.zeros(need.value // np.dtype(dtype).itemsize, dtype)
        if need.value:
            self._chk(self.L.trgl_debug_read(self.h, what, out.ctypes.data, out.nbytes, None))
        return out

    def debug_snapshot(self):
        """The intermediate buffers of the flush begun with flush_begin() (which stays pending: this call does not complete
        it) or of the last complete flush (until the next draw or clear): what k_setup and the binning left for k_raster.
        recs [N + 1] TRI_REC (rows of triangles without pairs are not written; row N exists after the complete flush), cnt [N],
        tilebox [N, 2], vals / bmask [P] (the side k_raster reads), tile_start / tile_end [tiles], info: dict of DBG_INFO_FIELDS.
        Raises TrglError where no flush can be read."""
        info = dict(zip(DBG_INFO_FIELDS, (int(v) for v in self._debug_read(DBG_INFO, np.int64))))
        return dict(info=info, recs=self._debug_read(DBG_RECS, TRI_REC), cnt=self._debug_read(DBG_CNT, np.uint32),
                    tilebox=self._debug_read(DBG_TILEBOX, np.uint32).reshape(-1, 2), vals=self._debug_read(DBG_VALS, np.uint32),
                    bmask=self._debug_read(DBG_BMASK, np.uint16), tile_start=self._debug_read(DBG_TILE_START, np.uint32),
                    tile_end=self._debug_read(DBG_TILE_END, np.uint32))
