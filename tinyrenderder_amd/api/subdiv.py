"""Subdivision: Loop and linear refinement of an indexed mesh from its edge list."""
import ctypes as C

import numpy as np

from .loader import SUBDIV_LOOP, load_library
from .marshal import _check, _count, _dp, _empty, _mem, _ptr_of, _ref, _vertices_f64, _words32


class SubdivParams(C.Structure):
    """trgl_subdiv_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("smooth", C.c_int32), ("mode", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


def make_subdiv_params(vertex_stride, mode=SUBDIV_LOOP, smooth=3):
    """trgl_subdiv_params: records of vertex_stride doubles; mode SUBDIV_LOOP - the first `smooth` doubles of a record get the Loop
    weights, the rest midpoints and copies - or SUBDIV_LINEAR (midpoints and copies throughout; smooth is ignored)."""
    return SubdivParams(int(vertex_stride), int(smooth), int(mode), 0, 0)


def subdiv_stencil_words(n_vertices, n_edges):
    """trgl_subdiv_stencil_words: 6 * n_edges + 4 * n_vertices, the uint32 words of a stencil array"""
    return 6 * int(n_edges) + 4 * int(n_vertices)


def _subdiv_topology(L, handle, indices, n_vertices, edges, n_edges, device, out):
    """Returns (arrays to keep alive, refined indices [4 n_faces, 3], stencils [subdiv_stencil_words]); out: the two, or None."""
    indices = _words32(indices, device, "indices", 3)
    edges = _words32(edges, device, "edges", 4)
    nf = _count(indices) // 3
    n = _count(edges) // 4 if n_edges is None else int(n_edges)
    words = subdiv_stencil_words(n_vertices, n)
    if out is None:
        out = (_empty((4 * nf, 3), np.uint32, device, indices), _empty(words, np.uint32, device, indices))
    p = _ptr_of(device)
    _check(L, handle, "trgl_subdiv_topology",
           L.trgl_subdiv_topology(handle, p(indices) if nf else None, nf, int(n_vertices), p(edges) if n else None, n, _mem(device),
                                  p(out[0]) if nf else None, p(out[1]) if words else None))
    return (indices, edges), out[0], out[1]


def _subdiv_inputs(vertices, stencils, n_edges, device):
    """(vertices [n, stride], stencils, n_edges): n_edges from the stencil array's size when not given"""
    vertices = _vertices_f64(vertices, device)
    stencils = _words32(stencils, device, "stencils")
    if n_edges is None:
        words = _count(stencils) - 4 * int(vertices.shape[0])
        if words < 0 or words % 6:
            raise ValueError("stencils must hold 6 * n_edges + 4 * n_vertices words")
        n_edges = words // 6
    return vertices, stencils, int(n_edges)


def _subdiv_vertices(L, handle, params, vertices, stencils, n_edges, device, out):
    """Returns (arrays to keep alive, refined vertices [n_vertices + n_edges, stride])."""
    vertices, stencils, n_edges = _subdiv_inputs(vertices, stencils, n_edges, device)
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    if out is None:
        out = _empty((nv + n_edges, stride), np.float64, device, vertices)
    p = _ptr_of(device)
    _check(L, handle, "trgl_subdiv_vertices", L.trgl_subdiv_vertices(handle, C.byref(params), p(vertices), nv, p(stencils), n_edges, _mem(device), p(out)))
    return (vertices, stencils), out


def subdiv_topology(indices, n_vertices, edges, n_edges=None):
    """trgl_subdiv_topology for host arrays without a context: from the faces indices [n_faces, 3] and the records mesh_edges made for
    them - n_edges the count, or None for the whole capacity - the refined faces [4 n_faces, 3] over the vertices 0 .. n_vertices - 1
    (even) and n_vertices + e (odd, one per record), and the stencil array subdiv_vertices takes.  Needs no GPU."""
    _, refined, stencils = _subdiv_topology(load_library(), None, indices, n_vertices, edges, n_edges, False, None)
    return refined, stencils


def subdiv_vertices(params, vertices, stencils, n_edges=None):
    """trgl_subdiv_vertices for host arrays without a context: the refined vertices [n_vertices + n_edges, stride] of vertices
    [n_vertices, stride] under params (make_subdiv_params) and the stencils of subdiv_topology.  Normals are not part of the rule:
    smooth = 3 and mesh_normals on the result.  Needs no GPU."""
    return _subdiv_vertices(load_library(), None, params, vertices, stencils, n_edges, False, None)[1]


class _SubdivCalls:
    """The subdivision methods of Context (context.py: L, h, _chk, _hold and _mesh_ptrs are its own)."""

    def subdiv_topology(self, indices, n_vertices, edges, n_edges=None, device=False, out=None):
        """trgl_subdiv_topology (see the module's subdiv_topology).  device=True: indices and edges are 32-bit device tensors - edges as
        mesh_edges(device=True) left them; n_edges=None passes the capacity, so no count has to visit the host -, out = (refined indices
        [4 n_faces, 3], stencils [subdiv_stencil_words]) device tensors (allocated with torch when None); queued on the context's
        stream without waiting.  Returns (refined indices, stencils)."""
        keep, refined, stencils = _subdiv_topology(self.L, self.h, indices, n_vertices, edges, n_edges, device, out)
        self._hold(device, (keep, refined, stencils))
        return refined, stencils

    def subdiv_vertices(self, params, vertices, stencils, n_edges=None, device=False, out=None):
        """trgl_subdiv_vertices (see the module's subdiv_vertices).  device=True: vertices [n, stride] f64 - one pose of skin_stage's
        output, say - and stencils are device tensors, out [n + n_edges, stride] a device tensor (allocated with torch when None); one
        kernel queued on the context's stream without waiting.  n_edges: the E the stencils were made with (None: from their size)."""
        keep, out = _subdiv_vertices(self.L, self.h, params, vertices, stencils, n_edges, device, out)
        self._hold(device, (keep, out))
        return out

    def draw_subdivided(self, kind, uniforms, projection, params, vertices, stencils, refined_indices, n_edges=None, device=False,
                        vertex_shader=None, colors=None):
        """trgl_draw_subdivided: subdiv_vertices into a buffer of the context's, then draw_indexed of it with the refined indices
        (vertex_shader= and colors= - one per refined face - as there).  device=True: every array is a device tensor; no wait."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, stencils, n_edges = _subdiv_inputs(vertices, stencils, n_edges, device)
        _, refined_indices, colors, ptrs = self._mesh_ptrs(vertices, refined_indices, colors, device)
        p = _ptr_of(device)
        self._hold(device, (vertices, stencils, refined_indices, colors))
        self._chk(self.L.trgl_draw_subdivided(self.h, -1 if vertex_shader is None else int(vertex_shader), kind, _ref(uniforms), _dp(pj), C.byref(params),
                                              p(vertices), int(vertices.shape[0]), p(stencils), n_edges, ptrs[1], int(refined_indices.shape[0]), ptrs[2],
                                              _mem(device)))
