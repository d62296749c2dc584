"""Sprites and lines: points and segments expanded to quads of two triangles."""
import ctypes as C

import numpy as np

from .loader import SPRITE_VIEW, load_library
from .marshal import _check, _count, _f64, _is_device_tensor, _mem, _ptr_of, _ref, _triangle_outputs, _vertices_f64


class SpriteParams(C.Structure):
    """trgl_sprite_params"""
    _fields_ = [("model_view", C.c_double * 16), ("projection", C.c_double * 16), ("size", C.c_double), ("scale", C.c_double * 2),
                ("mode", C.c_int32), ("size_offset", C.c_int32), ("attr_offset", C.c_int32), ("n_attr", C.c_int32)]


class LineParams(C.Structure):
    """trgl_line_params"""
    _fields_ = [("model_view", C.c_double * 16), ("projection", C.c_double * 16), ("width", C.c_double), ("half_extent", C.c_double * 2),
                ("w_min", C.c_double)]


def make_sprite_params(model_view, projection, size=1.0, scale=(0.0, 0.0), mode=SPRITE_VIEW, size_offset=-1, attr_offset=0, n_attr=0):
    """trgl_sprite_params: row-major 4x4 matrices; size is used when size_offset < 0, else the point's size is column size_offset of its
    row; scale = (2 / w, 2 / h) gives SPRITE_SCREEN sizes in pixels of a w x h viewport; n_attr columns from attr_offset on follow the
    uv pairs in the varyings of both triangles."""
    return SpriteParams((C.c_double * 16)(*_f64(model_view, 16, "model_view")), (C.c_double * 16)(*_f64(projection, 16, "projection")),
                        float(size), (C.c_double * 2)(*_f64(scale, 2, "scale")), int(mode), int(size_offset), int(attr_offset), int(n_attr))


def make_line_params(model_view, projection, width, half_extent, w_min):
    """trgl_line_params: width in the units of half_extent (pixels with half_extent = (w / 2, h / 2) of the viewport); the segment is cut
    where its clip w falls below w_min > 0."""
    return LineParams((C.c_double * 16)(*_f64(model_view, 16, "model_view")), (C.c_double * 16)(*_f64(projection, 16, "projection")),
                      float(width), (C.c_double * 2)(*_f64(half_extent, 2, "half_extent")), float(w_min))


def _quad_inputs(points, indices, colors, device):
    """(points, indices, colors) as the sprite and line calls take them, checked: device tensors with device=True, else numpy arrays."""
    points = _vertices_f64(points, device, "points")
    if device:
        for a, what in ((indices, "indices"), (colors, "colors")):
            if a is not None and (not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous()):
                raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor")
        return points, indices, colors
    return (points, None if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1),
            None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(-1))


def _sprite_stage(L, handle, params, points, colors, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - two rows per point."""
    points, _, colors = _quad_inputs(points, None, colors, device)
    n, stride = int(points.shape[0]), int(points.shape[1])
    if colors is not None and int(colors.shape[0]) != n:
        raise ValueError("colors: one per point")
    if out is None:
        out = _triangle_outputs(2 * n, 6 + max(int(params.n_attr), 0), True, colors, device, points)
    p = _ptr_of(device)
    _check(L, handle, "trgl_sprite_stage",
           L.trgl_sprite_stage(handle, C.byref(params), p(points), stride, p(colors), n, _mem(device), p(out[0]), p(out[1]), p(out[2])))
    return (points, colors), out


def _line_segments(points, indices, n_segments):
    if n_segments is not None:
        return int(n_segments)
    return int(points.shape[0]) // 2 if indices is None else _count(indices) // 2


def _line_stage(L, handle, params, points, indices, colors, n_segments, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - two rows per segment."""
    points, indices, colors = _quad_inputs(points, indices, colors, device)
    n_points, stride = int(points.shape[0]), int(points.shape[1])
    n = _line_segments(points, indices, n_segments)
    if colors is not None and int(colors.shape[0]) != n:
        raise ValueError("colors: one per segment")
    if out is None:
        out = _triangle_outputs(2 * n, 6, True, colors, device, points)
    p = _ptr_of(device)
    _check(L, handle, "trgl_line_stage",
           L.trgl_line_stage(handle, C.byref(params), p(points), stride, n_points, p(indices), p(colors), n, _mem(device), p(out[0]), p(out[1]), p(out[2])))
    return (points, indices, colors), out


def sprite_stage(params, points, colors=None):
    """trgl_sprite_stage for host arrays without a context: every point [n, stride >= 3] becomes a quad of two triangles that faces the
    camera (params: make_sprite_params).  Returns (clip [2 n, 12], varyings [2 n, 6 + n_attr], colors [2 n] or None).  Needs no GPU."""
    return _sprite_stage(load_library(), None, params, points, colors, False, None)[1]


def line_stage(params, points, indices=None, colors=None, n_segments=None):
    """trgl_line_stage for host arrays without a context: every segment - a pair of `indices` into points [n_points, stride >= 3], or
    points 2 j and 2 j + 1 - becomes a quad of params.width (params: make_line_params), cut at clip w = w_min.  Returns (clip [2 n, 12],
    varyings [2 n, 6], colors [2 n] or None).  Needs no GPU."""
    return _line_stage(load_library(), None, params, points, indices, colors, n_segments, False, None)[1]


class _QuadCalls:
    """The sprite and line methods of Context (context.py: L, h, _chk and _hold are its own)."""

    def sprite_stage(self, params, points, colors=None, device=False, out=None):
        """trgl_sprite_stage: two triangles per point (see the module's sprite_stage).  Host arrays: numpy, no GPU work.  device=True:
        points [n, stride] f64 and colors [n] (32-bit) or None are device tensors, out = (clip_out, varyings_out, colors_out) device
        tensors with 2 n rows (allocated with torch when not given); the stage is queued on the context's stream without waiting.
        Returns (clip_out, varyings_out, colors_out) - what triangle_depths(group=2), order_stage and draw(device=True) take."""
        keep, out = _sprite_stage(self.L, self.h, params, points, colors, device, out)
        self._hold(device, (keep, out))
        return out

    def line_stage(self, params, points, indices=None, colors=None, n_segments=None, device=False, out=None):
        """trgl_line_stage: two triangles per segment (see the module's line_stage).  device=True: points [n_points, stride] f64, indices
        [2 n] and colors [n] (32-bit) or None are device tensors; an index that names no point gives all-zero rows; queued on the
        context's stream without waiting.  Returns (clip_out, varyings_out, colors_out)."""
        keep, out = _line_stage(self.L, self.h, params, points, indices, colors, n_segments, device, out)
        self._hold(device, (keep, out))
        return out

    def draw_sprites(self, kind, params, points, colors=None, uniforms=None, device=False):
        """trgl_draw_sprites: draw() of the rows sprite_stage makes; the kind takes 6 + n_attr varyings, or none.  device=True: the
        points are expanded on the context's stream into buffers of the context's (no wait); they are read then, not at the flush."""
        points, _, colors = _quad_inputs(points, None, colors, device)
        p = _ptr_of(device)
        self._hold(device, (points, colors))
        self._chk(self.L.trgl_draw_sprites(self.h, kind, _ref(uniforms), C.byref(params), p(points), int(points.shape[1]), p(colors), int(points.shape[0]),
                                           _mem(device)))

    def draw_lines(self, kind, params, points, indices=None, colors=None, n_segments=None, uniforms=None, device=False):
        """trgl_draw_lines: draw() of the rows line_stage makes; the kind takes 6 varyings - (t, side) per vertex - or none."""
        points, indices, colors = _quad_inputs(points, indices, colors, device)
        p = _ptr_of(device)
        self._hold(device, (points, indices, colors))
        self._chk(self.L.trgl_draw_lines(self.h, kind, _ref(uniforms), C.byref(params), p(points), int(points.shape[1]), int(points.shape[0]), p(indices),
                                         p(colors), _line_segments(points, indices, n_segments), _mem(device)))
