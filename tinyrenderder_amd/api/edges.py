"""Edges: the edge list of an indexed mesh, its silhouette / crease / boundary classes, and outlines drawn from them."""
import ctypes as C

import numpy as np

from .loader import EDGE_ANY, load_library
from .marshal import _check, _count, _device_f64, _empty, _f64, _mem, _ptr_of, _ref, _vertices_f64, _words32


class EdgeParams(C.Structure):
    """trgl_edge_params"""
    _fields_ = [("eye", C.c_double * 4), ("crease_cos", C.c_double), ("class_color", C.c_uint32 * 4), ("select", C.c_uint32),
                ("compact", C.c_uint32), ("reserved", C.c_uint64)]


def make_edge_params(eye, crease_cos=-2.0, select=EDGE_ANY, class_color=(0, 0, 0, 0), compact=False):
    """trgl_edge_params: eye (x, y, z, w) in model space - w = 1 a camera position, w = 0 a direction toward the viewer; an edge is a
    crease when the dot product of its faces' unit normals is below crease_cos (-2: never); select: a mask of EDGE_ANY, EDGE_BOUNDARY,
    EDGE_SILHOUETTE, EDGE_CREASE; class_color: the colour of each of the four in that order; compact: selected segments to the front."""
    return EdgeParams((C.c_double * 4)(*_f64(eye, 4, "eye")), float(crease_cos), (C.c_uint32 * 4)(*[int(x) & 0xFFFFFFFF for x in class_color]),
                      int(select), 1 if compact else 0, 0)


def _mesh_edges(L, handle, indices, n_vertices, device, out, count):
    """Returns (arrays to keep alive, edges [3 n_faces, 4], n_edges or None)."""
    indices = _words32(indices, device, "indices", 3)
    nf = _count(indices) // 3
    if out is None:
        out = _empty((3 * nf, 4), np.uint32, device, indices)
    n = C.c_uint64(0)
    p = _ptr_of(device)
    _check(L, handle, "trgl_mesh_edges",
           L.trgl_mesh_edges(handle, p(indices) if nf else None, nf, int(n_vertices), _mem(device), p(out) if nf else None, C.byref(n) if count else None))
    return (indices,), out, (int(n.value) if count else None)


def _edge_select(L, handle, params, vertices, indices, edges, n_edges, device, out, count):
    """Returns (arrays to keep alive, (codes [n], segments [n, 2], colors [n]), n_selected or None); out: three arrays, each may be None
    (not written) - all three are allocated when out is None."""
    vertices = _vertices_f64(vertices, device)
    indices = _words32(indices, device, "indices", 3)
    edges = _words32(edges, device, "edges", 4)
    nf = _count(indices) // 3
    n = _count(edges) // 4 if n_edges is None else int(n_edges)
    if out is None:
        out = (_empty(n, np.uint8, device, vertices), _empty((n, 2), np.uint32, device, vertices), _empty(n, np.uint32, device, vertices))
    nsel = C.c_uint64(0)
    p = _ptr_of(device)
    _check(L, handle, "trgl_edge_select",
           L.trgl_edge_select(handle, C.byref(params), p(vertices), int(vertices.shape[1]), int(vertices.shape[0]), p(indices), nf, p(edges), n, _mem(device),
                              p(out[0]), p(out[1]), p(out[2]), C.byref(nsel) if count else None))
    return (vertices, indices, edges), out, (int(nsel.value) if count else None)


def mesh_edges(indices, n_vertices):
    """trgl_mesh_edges for host arrays without a context: the distinct edges of the faces indices [n_faces, 3] in ascending (lo, hi).
    Returns (edges [3 n_faces, 4] uint32 - records {lo, hi, f0, f1}, f1 = EDGE_NONE on a boundary, every word EDGE_NONE behind the last
    edge - and the number of edges).  Needs no GPU."""
    _, out, n = _mesh_edges(load_library(), None, indices, n_vertices, False, None, True)
    return out, n


def edge_select(params, vertices, indices, edges, n_edges=None):
    """trgl_edge_select for host arrays without a context: the code byte of every edge record under params (make_edge_params), the
    index pair of every selected one - what line_stage takes as indices - and its colour.  Returns (codes [n], segments [n, 2],
    colors [n], n_selected); with params.compact the selected pairs and colours come first.  Needs no GPU."""
    _, out, n = _edge_select(load_library(), None, params, vertices, indices, edges, n_edges, False, None, True)
    return out[0], out[1], out[2], n


class _EdgeCalls:
    """The edge methods of Context (context.py: L, h, _chk and _hold are its own)."""

    def mesh_edges(self, indices, n_vertices, device=False, out=None, count=True):
        """trgl_mesh_edges (see the module's mesh_edges).  device=True: indices [n_faces, 3] is a 32-bit device tensor and the records
        come back as a device tensor [3 n_faces, 4] (`out` when given); an index >= n_vertices makes no edge.  count=True waits once for
        the 8-byte count; count=False queues the kernels without waiting and returns None for it.  Returns (edges, n_edges)."""
        keep, out, n = _mesh_edges(self.L, self.h, indices, n_vertices, device, out, count)
        self._hold(device, (keep, out))
        return out, n

    def edge_select(self, params, vertices, indices, edges, n_edges=None, device=False, out=None, count=None):
        """trgl_edge_select (see the module's edge_select).  device=True: vertices [n, stride] f64, indices and edges (32-bit) are device
        tensors - vertices may be one pose of skin_stage's output -, out = (codes uint8, segments, colors) device tensors, each may be
        None (allocated with torch when out is None); queued on the context's stream.  count (default: params.compact): wait once for
        the 8-byte count of selected records.  Returns (codes, segments, colors, n_selected or None): segments and colors are what
        draw_lines takes as indices and colors."""
        if count is None:
            count = bool(params.compact) or not device
        keep, out, n = _edge_select(self.L, self.h, params, vertices, indices, edges, n_edges, device, out, count)
        self._hold(device, (keep, out))
        return out[0], out[1], out[2], n

    def draw_outline(self, kind, line_params, edge_params, vertices, indices, edges, n_edges=None, uniforms=None, device=False):
        """trgl_draw_outline: edge_select with compaction into buffers of the context's, then draw_lines of the selected segments in
        their class colours with the mesh's vertices as points; the kind takes 6 varyings or none.  device=True: every array is a
        device tensor, and the call waits once for the count.  A line lies in the surface: bias the depth in line_params.projection."""
        # (host vertices of another rank than 2 are not refused here, as they are by edge_select: the library sees their first two sizes)
        vertices = _device_f64(vertices, 2, "vertices") if device else np.ascontiguousarray(vertices, np.float64)
        indices = _words32(indices, device, "indices", 3)
        edges = _words32(edges, device, "edges", 4)
        nf = _count(indices) // 3
        n = _count(edges) // 4 if n_edges is None else int(n_edges)
        p = _ptr_of(device)
        self._hold(device, (vertices, indices, edges))
        self._chk(self.L.trgl_draw_outline(self.h, kind, _ref(uniforms), C.byref(line_params), C.byref(edge_params), p(vertices), int(vertices.shape[1]),
                                           int(vertices.shape[0]), p(indices), nf, p(edges), n, _mem(device)))
