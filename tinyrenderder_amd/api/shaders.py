"""Shaders: user fragment and vertex shaders compiled at run time, and the vertex stage on its own."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import PHONG, SHADER_MAY_DISCARD, SHADER_NO_DEPTH_WRITE, SHADER_READS_DEST, VARY, load_library
from .marshal import _device_ptr, _dp, _failure, _mem, _ref


def shader_flags(may_discard=False, reads_dest=False, depth_write=True) -> int:
    """The flag word of trgl_shader_compile_ex / trgl_register_shader_ex; which words are valid is the library's decision."""
    return ((SHADER_MAY_DISCARD if may_discard else 0) | (SHADER_READS_DEST if reads_dest else 0)
            | (0 if depth_write else SHADER_NO_DEPTH_WRITE))


def _compiled(name, rc, log):
    """(ok, compiler log) of a compile call: -1 is a shader that does not compile, any other failure raises with the log"""
    if rc not in (0, -1):
        raise _failure(name, rc, log.value.decode(errors="replace"))
    return rc == 0, log.value.decode(errors="replace")


def shader_compile(source: str, n_varyings: int, may_discard: bool = False, *, reads_dest: bool = False, depth_write: bool = True):
    """trgl_shader_compile_ex: compile a user shader (include/trgl.h, "User shaders") without a GPU or a context; may_discard: one
    whose trgl_fragment returns trgl_frag_out (TRGL_SHADER_MAY_DISCARD).  reads_dest: in.dst is the pixel under the fragment
    (TRGL_SHADER_READS_DEST); depth_write=False: TRGL_SHADER_NO_DEPTH_WRITE.  Both need may_discard.
    Returns (ok, compiler log); raises when user shaders are unavailable (no hiprtc)."""
    L = load_library()
    log = C.create_string_buffer(16384)
    rc = L.trgl_shader_compile_ex(source.encode(), int(n_varyings), shader_flags(may_discard, reads_dest, depth_write), log, len(log))
    return _compiled("trgl_shader_compile", rc, log)


def vertex_shader_compile(source: str, n_varyings: int):
    """trgl_vertex_shader_compile: compile a user vertex shader (include/trgl.h, "User vertex shaders") without a GPU or a context.
    Returns (ok, compiler log); raises when user shaders are unavailable (no hiprtc)."""
    L = load_library()
    log = C.create_string_buffer(16384)
    rc = L.trgl_vertex_shader_compile(source.encode(), int(n_varyings), log, len(log))
    return _compiled("trgl_vertex_shader_compile", rc, log)


class _ShaderCalls:
    """The user shader methods of Context (context.py: L, h, _chk, _hold, _mesh_ptrs and the two tables of registered shaders are
    its own); draw() and draw_indexed() take the numbers these hand out."""

    def register_shader(self, source: str, n_varyings: int, may_discard: bool = False, *, reads_dest: bool = False,
                        depth_write: bool = True) -> int:
        """trgl_register_shader_ex: compile (or take from the process cache) a user shader and load it on this context; returns its
        kind, for draw() with n x n_varyings varyings.  may_discard: its trgl_fragment returns trgl_frag_out and runs for every
        z-pass in order (TRGL_SHADER_MAY_DISCARD).  With it, reads_dest: in.dst is the pixel the fragment is drawn over
        (TRGL_SHADER_READS_DEST); depth_write=False: a drawn fragment leaves the depth alone (TRGL_SHADER_NO_DEPTH_WRITE)."""
        kind = C.c_int(-1)
        self._chk(self.L.trgl_register_shader_ex(self.h, source.encode(), int(n_varyings), shader_flags(may_discard, reads_dest, depth_write), C.byref(kind)))
        self._user_vary[kind.value] = int(n_varyings)
        return kind.value

    def register_vertex_shader(self, source: str, n_varyings: int) -> int:
        """trgl_register_vertex_shader: compile (or take from the process cache) a user vertex shader and load it on this context;
        returns its number (from 0, apart from the fragment kinds), for draw_indexed(vertex_shader=) and vertex_stage()."""
        vs = C.c_int(-1)
        self._chk(self.L.trgl_register_vertex_shader(self.h, source.encode(), int(n_varyings), C.byref(vs)))
        self._vertex_vary[vs.value] = int(n_varyings)
        return vs.value

    def vertex_stage(self, vertex_shader, uniforms, projection, vertices, indices, device=False, out=None):
        """trgl_vertex_stage: the vertex stage alone.  vertex_shader: a number from register_vertex_shader, or -1 for the built-in
        stage of draw_indexed (K = 24).  Host arrays: returns (clip [nf, 12], varyings [nf, K]) as numpy arrays.  device=True:
        vertices, indices and out = (clip, varyings) are device tensors (varyings may be None when K = 0), 16-byte aligned outputs
        that the stage fills on the context's stream; returns out."""
        vs = int(vertex_shader)
        K = VARY[PHONG] if vs < 0 else getattr(self, "_vertex_vary", {}).get(vs, 0)   # (an unknown number goes to the library, which refuses it)
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, indices, _, ptrs = self._mesh_ptrs(vertices, indices, None, device)
        nv, stride = vertices.shape
        nf = indices.shape[0]
        if device:
            clip, vary = out
            optrs = (_device_ptr(clip, "clip"), _device_ptr(vary, "varyings"))
            self._hold(True, (vertices, indices, clip, vary))
        else:
            assert out is None, "out: only with device=True"
            clip, vary = np.zeros((nf, 12), np.float64), np.zeros((nf, K), np.float64)
            optrs = (clip.ctypes.data, vary.ctypes.data if K else None)
        self._chk(self.L.trgl_vertex_stage(self.h, vs, _ref(uniforms), _dp(pj), ptrs[0], stride, nv, ptrs[1], nf, optrs[0], optrs[1], _mem(device)))
        return clip, vary
