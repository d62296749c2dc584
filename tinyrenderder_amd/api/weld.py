"""Weld and levels of detail: identical vertices joined, faces cleaned up, and one level of vertex clustering."""
import ctypes as C

import numpy as np

from .loader import load_library
from .marshal import _check, _count, _mem, _named_outputs, _ptr, _ptr_of, _vertices_f64, _words32


class WeldParams(C.Structure):
    """trgl_weld_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("key_offset", C.c_int32), ("key_count", C.c_int32), ("reserved32", C.c_int32), ("cell", C.c_double),
                ("reserved", C.c_uint64)]


def make_weld_params(vertex_stride, key_offset=0, key_count=3, cell=0.0):
    """trgl_weld_params: records of vertex_stride doubles, compared by the key_count doubles from key_offset on - the values themselves
    (cell = 0.0: IEEE ==, so -0.0 joins +0.0 and a NaN joins nothing), or their grid cells floor(x / cell + 0.5) (a grid weld: two values
    on either side of a cell border do not join)."""
    return WeldParams(int(vertex_stride), int(key_offset), int(key_count), 0, float(cell), 0)


WELD_OUTPUTS = ("remap", "firsts", "vertices", "indices")


def _mesh_weld(L, handle, params, vertices, indices, device, out, count):
    """Returns (arrays to keep alive, dict(remap [n], firsts [n], vertices [n, stride], indices [n_faces, 3] or None), n_unique or
    None).  out: None - every output is allocated (indices only with `indices`) - or a dict naming the outputs to write, each an array
    or None to allocate it; an output that is not named is not written (NULL)."""
    vertices = _vertices_f64(vertices, device)
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    nf = 0
    if indices is not None:
        indices = _words32(indices, device, "indices", 3)
        nf = _count(indices) // 3
    if out is None:
        out = {k: None for k in WELD_OUTPUTS if k != "indices" or indices is not None}
    res = _named_outputs(WELD_OUTPUTS, out, dict(remap=(nv,), firsts=(nv,), vertices=(nv, stride), indices=(nf, 3)), device, vertices, "mesh_weld")
    n = C.c_uint64(0)
    p = _ptr_of(device)
    _check(L, handle, "trgl_mesh_weld",
           L.trgl_mesh_weld(handle, C.byref(params), p(vertices) if nv else None, nv, p(indices) if nf else None, nf, _mem(device), p(res["remap"]),
                            p(res["firsts"]), p(res["vertices"]), p(res["indices"]) if nf or indices is None else None, C.byref(n) if count else None))
    return (vertices, indices), res, (int(n.value) if count else None)


def mesh_weld(params, vertices, indices=None):
    """trgl_mesh_weld for host arrays without a context: the vertices [n, stride] whose keys (params: make_weld_params) are identical
    joined.  Returns (dict(remap [n] - the new number of every old vertex -, firsts [n] - the old number of every new vertex, EDGE_NONE
    behind the last -, vertices [n, stride] - the kept records, zeros behind the last -, indices [n_faces, 3] - `indices` renumbered, or
    None without them), n_unique).  For a triangle soup remap.reshape(-1, 3) is the index array.  Needs no GPU."""
    _, out, n = _mesh_weld(load_library(), None, params, vertices, indices, False, None, True)
    return out, n


def weld_hashes(params, vertices):
    """Test hook (trgl_debug_weld_hash): the 64-bit hash the device path of mesh_weld sorts by, per vertex of a host array."""
    L = load_library()
    vertices = np.ascontiguousarray(vertices, np.float64)
    out = np.empty(vertices.shape[0], np.uint64)
    _check(L, None, "trgl_debug_weld_hash", L.trgl_debug_weld_hash(C.addressof(params), _ptr(vertices), int(vertices.shape[0]), _ptr(out)))
    return out


class CleanParams(C.Structure):
    """trgl_clean_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("flags", C.c_uint32), ("fill", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


class SimplifyParams(C.Structure):
    """trgl_simplify_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("mean_count", C.c_int32), ("fill", C.c_uint32), ("reserved32", C.c_uint32), ("cell", C.c_double),
                ("reserved", C.c_uint64)]


CLEAN_DUPLICATES, CLEAN_VERTICES = 1, 2
CLEAN_FILL_NONE, CLEAN_FILL_ZERO = 0, 1


def make_clean_params(vertex_stride=0, flags=CLEAN_DUPLICATES | CLEAN_VERTICES, fill=CLEAN_FILL_NONE):
    """trgl_clean_params: flags - CLEAN_DUPLICATES drops a face whose canonical triple an earlier face has, CLEAN_VERTICES renumbers the
    vertices that kept faces name -; fill - what stands behind the kept faces in indices: CLEAN_FILL_NONE (no vertex) or CLEAN_FILL_ZERO
    (faces (0, 0, 0), which a draw drops); vertex_stride is read only when records are written."""
    return CleanParams(int(vertex_stride), int(flags), int(fill), 0, 0)


def make_simplify_params(vertex_stride, cell, mean_count=3, fill=CLEAN_FILL_NONE):
    """trgl_simplify_params: one level of vertex clustering over records of vertex_stride >= 3 doubles whose first three are the position;
    cell - the width of the grid (0: the positions themselves); the first mean_count doubles of a kept record become the mean of the
    cell's referenced members; fill as make_clean_params."""
    return SimplifyParams(int(vertex_stride), int(mean_count), int(fill), 0, float(cell), 0)


CLEAN_OUTPUTS = ("indices", "face_firsts", "vremap", "vfirsts", "vertices")
SIMPLIFY_OUTPUTS = ("remap", "firsts", "vertices", "indices", "face_firsts")


def _mesh_clean(L, handle, params, indices, vertices, n_vertices, device, out, count):
    """Returns (arrays to keep alive, dict(indices [n_faces, 3], face_firsts [n_faces], vremap [n], vfirsts [n], vertices [n, stride] - the
    last three None without CLEAN_VERTICES, the last without `vertices`), (kept faces, kept vertices) or None)."""
    indices = _words32(indices, device, "indices", 3)
    nf = _count(indices) // 3
    stride = 0
    if vertices is not None:
        vertices = _vertices_f64(vertices, device, "mesh_clean: vertices")
        nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
        if n_vertices is not None and int(n_vertices) != nv:
            raise ValueError("mesh_clean: n_vertices differs from the vertex array")
        if params.vertex_stride != stride and (params.flags & CLEAN_VERTICES):
            raise ValueError("mesh_clean: params.vertex_stride differs from the vertex array")
    elif n_vertices is None:
        raise ValueError("mesh_clean: n_vertices is needed without a vertex array")
    else:
        nv = int(n_vertices)
    names = CLEAN_OUTPUTS if params.flags & CLEAN_VERTICES else CLEAN_OUTPUTS[:2]
    if vertices is None:
        names = tuple(k for k in names if k != "vertices")
    res = _named_outputs(names, out, dict(indices=(nf, 3), face_firsts=(nf,), vremap=(nv,), vfirsts=(nv,), vertices=(nv, stride)), device, indices,
                         "mesh_clean")
    res.update({k: None for k in CLEAN_OUTPUTS if k not in res})
    n = (C.c_uint64 * 2)(0, 0)
    p = _ptr_of(device)
    _check(L, handle, "trgl_mesh_clean",
           L.trgl_mesh_clean(handle, C.byref(params), p(indices) if nf else None, nf, p(vertices) if vertices is not None and nv else None, nv, _mem(device),
                             p(res["indices"]) if nf else None, p(res["face_firsts"]) if nf else None, p(res["vremap"]), p(res["vfirsts"]),
                             p(res["vertices"]), n if count else None))
    return (indices, vertices), res, ((int(n[0]), int(n[1])) if count else None)


def mesh_clean(params, indices, vertices=None, n_vertices=None):
    """trgl_mesh_clean for host arrays without a context: the faces [n_faces, 3] that draw nothing - two equal indices; with
    CLEAN_DUPLICATES the canonical triple of an earlier face - dropped, the kept ones in their order; with CLEAN_VERTICES the vertices they
    name renumbered in ascending old number.  Returns (dict(indices [n_faces, 3] - the fill behind the kept faces -, face_firsts [n_faces]
    - the old number of every kept face, EDGE_NONE behind -, vremap [n], vfirsts [n], vertices [n, stride] as mesh_weld's remap, firsts and
    vertices), (kept faces, kept vertices)).  Without `vertices` pass n_vertices.  Needs no GPU."""
    _, out, n = _mesh_clean(load_library(), None, params, indices, vertices, n_vertices, False, None, True)
    return out, n


def _mesh_simplify(L, handle, params, vertices, indices, device, out, count):
    """Returns (arrays to keep alive, dict(remap [n], firsts [n], vertices [n, stride], indices [n_faces, 3], face_firsts [n_faces]),
    (kept faces, kept vertices) or None)."""
    vertices = _vertices_f64(vertices, device, "mesh_simplify: vertices")
    nv, stride = int(vertices.shape[0]), int(vertices.shape[1])
    indices = _words32(indices, device, "indices", 3)
    nf = _count(indices) // 3
    res = _named_outputs(SIMPLIFY_OUTPUTS, out, dict(remap=(nv,), firsts=(nv,), vertices=(nv, stride), indices=(nf, 3), face_firsts=(nf,)), device,
                         vertices, "mesh_simplify")
    n = (C.c_uint64 * 2)(0, 0)
    p = _ptr_of(device)
    _check(L, handle, "trgl_mesh_simplify",
           L.trgl_mesh_simplify(handle, C.byref(params), p(vertices) if nv else None, nv, p(indices) if nf else None, nf, _mem(device), p(res["remap"]),
                                p(res["firsts"]), p(res["vertices"]), p(res["indices"]) if nf else None, p(res["face_firsts"]) if nf else None,
                                n if count else None))
    return (vertices, indices), res, ((int(n[0]), int(n[1])) if count else None)


def mesh_simplify(params, vertices, indices):
    """trgl_mesh_simplify for host arrays without a context: one level of vertex clustering - a grid weld by position (params:
    make_simplify_params), the mean of every cell's referenced members, then mesh_clean with both flags.  Returns (dict(remap [n] - the new
    number of every old vertex, EDGE_NONE when its cluster left -, firsts [n] - the lowest old vertex of every new one -, vertices
    [n, stride], indices [n_faces, 3], face_firsts [n_faces]), (kept faces, kept vertices)).  Needs no GPU."""
    _, out, n = _mesh_simplify(load_library(), None, params, vertices, indices, False, None, True)
    return out, n


def lod_face_hashes(indices, n_vertices):
    """Test hook (trgl_debug_lod_face_hash): the 64-bit value the device path of mesh_clean sorts every face of a host array by."""
    L = load_library()
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    out = np.empty(indices.shape[0], np.uint64)
    _check(L, None, "trgl_debug_lod_face_hash", L.trgl_debug_lod_face_hash(_ptr(indices), int(indices.shape[0]), int(n_vertices), _ptr(out)))
    return out


class _WeldCalls:
    """The weld and level-of-detail methods of Context (context.py: L, h, _chk and _hold are its own)."""

    def mesh_weld(self, params, vertices, indices=None, device=False, out=None, count=True):
        """trgl_mesh_weld (see the module's mesh_weld).  device=True: vertices [n, stride] f64 and indices [n_faces, 3] (32-bit, or None)
        are device tensors and so are the outputs; out: None for all of them, or a dict naming those to write - "remap", "firsts",
        "vertices", "indices", each a device tensor or None to allocate it.  count=True waits once for the 8-byte count; count=False
        queues the kernels without waiting and returns None for it: later calls take the capacity n.  Returns (dict, n_unique)."""
        keep, out, n = _mesh_weld(self.L, self.h, params, vertices, indices, device, out, count)
        self._hold(device, (keep, out))
        return out, n

    def mesh_clean(self, params, indices, vertices=None, n_vertices=None, device=False, out=None, count=True):
        """trgl_mesh_clean (see the module's mesh_clean).  device=True: indices [n_faces, 3] (32-bit) and vertices [n, stride] f64 (or None
        with n_vertices) are device tensors and so are the outputs; out: None for all of them, or a dict naming those to write -
        "indices", "face_firsts", "vremap", "vfirsts", "vertices", each a device tensor or None to allocate it.  count=True waits once for
        the 16 bytes of the counts; count=False queues the kernels without waiting and returns None for them: later calls take the
        capacities.  Returns (dict, (kept faces, kept vertices))."""
        keep, out, n = _mesh_clean(self.L, self.h, params, indices, vertices, n_vertices, device, out, count)
        self._hold(device, (keep, out))
        return out, n

    def mesh_simplify(self, params, vertices, indices, device=False, out=None, count=True):
        """trgl_mesh_simplify (see the module's mesh_simplify).  device=True: device tensors in and out; out: None for all outputs, or a
        dict naming those to write - "remap", "firsts", "vertices", "indices", "face_firsts".  count=False queues without waiting: with
        fill CLEAN_FILL_NONE a second level takes the outputs at their capacities.  Returns (dict, (kept faces, kept vertices))."""
        keep, out, n = _mesh_simplify(self.L, self.h, params, vertices, indices, device, out, count)
        self._hold(device, (keep, out))
        return out, n

    def debug_lod_hash_bits(self, bits=64):
        """Test hook (trgl_debug_lod_hash_bits): later device cleans and simplifies keep the low `bits` bits of the face hash (0 .. 64) and
        sort over them.  Small values force the walk through colliding triples; 0 is one run.  The outputs do not change with it."""
        self._chk(self.L.trgl_debug_lod_hash_bits(self.h, int(bits)))

    def debug_lod_sort(self, n_faces, n_vertices):
        """Diagnostic (trgl_debug_lod_sort): the sort of the last device clean of these counts again, over the pairs it left; no wait."""
        self._chk(self.L.trgl_debug_lod_sort(self.h, int(n_faces), int(n_vertices)))

    def debug_weld_hash_bits(self, bits=64):
        """Test hook (trgl_debug_weld_hash_bits): later device welds keep the low `bits` bits of the hash (0 .. 64) and sort over them.
        Small values force the walk through colliding keys; 0 is one run.  The outputs do not change with it."""
        self._chk(self.L.trgl_debug_weld_hash_bits(self.h, int(bits)))

    def debug_weld_sort(self, n_vertices):
        """Diagnostic (trgl_debug_weld_sort): the sort of the last device weld of n_vertices again, over the pairs it left; no wait."""
        self._chk(self.L.trgl_debug_weld_sort(self.h, int(n_vertices)))
