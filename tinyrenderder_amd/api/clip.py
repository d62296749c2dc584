"""Clip: triangles cut against a plane before rasterize(), and the attribute layouts the cut interpolates."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import MAX_CLIP_ATTRS, ClipAttr, load_library
from .marshal import _check, _device_ptr, _dp, _f64, _mem, _ptr, _triangle_outputs


def clip_layout(kind: int):
    """trgl_clip_layout: the built-in clip attribute layout of a built-in kind as a list of (offset, components).  Needs no GPU."""
    L = load_library()
    attrs, n = (ClipAttr * MAX_CLIP_ATTRS)(), C.c_int(0)
    _check(L, None, "trgl_clip_layout", L.trgl_clip_layout(int(kind), attrs, C.byref(n)))
    return [(attrs[i].offset, attrs[i].components) for i in range(n.value)]


def _clip_attrs(attrs):
    """(ctypes array or None, count) of a list of (offset, components); None stands for the kind's built-in layout (-1)."""
    if attrs is None:
        return None, -1
    attrs = [(int(o), int(k)) for o, k in attrs]
    arr = (ClipAttr * max(len(attrs), 1))()
    for i, (o, k) in enumerate(attrs):
        arr[i].offset, arr[i].components = o, k
    return arr, len(attrs)


def _clip_stage(L, handle, plane, attrs, K, ptrs, n, optrs, device):
    arr, na = _clip_attrs([] if attrs is None else attrs)
    n_out = C.c_uint64(0)
    _check(L, handle, "trgl_clip_stage",
           L.trgl_clip_stage(handle, _dp(_f64(plane, 4, "plane")), arr, na, int(K), ptrs[0], ptrs[1], ptrs[2], int(n), optrs[0], optrs[1], optrs[2],
                             C.byref(n_out), _mem(device)))
    return int(n_out.value)


def _host_clip_stage(L, handle, plane, attrs, clip, varyings, colors):
    clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
    n = clip.shape[0]
    vary = None if varyings is None else np.ascontiguousarray(varyings, np.float64).reshape(n, np.shape(varyings)[-1] if np.ndim(varyings) == 2 else -1)
    K = 0 if vary is None else vary.shape[1]
    col = None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(n)
    oclip, ovary, ocol = _triangle_outputs(2 * n, K, True, col, False, None)
    m = _clip_stage(L, handle, plane, attrs, K, (_ptr(clip), _ptr(vary) if K else None, _ptr(col)), n,
                    (_ptr(oclip), _ptr(ovary) if K else None, _ptr(ocol)), False)
    return oclip[:m].copy(), (ovary[:m].copy() if K else None), (None if ocol is None else ocol[:m].copy())


def clip_stage(plane, clip, varyings=None, colors=None, attrs=None):
    """trgl_clip_stage for host arrays without a context (include/trgl.h writes the operation down): clip [n, 12], varyings [n, K] or
    None, colors [n] or None, attrs a list of (offset, components) (None: no attributes, every varying is a per-triangle constant).
    Returns (clip, varyings, colors) of the output triangles.  Needs no GPU."""
    return _host_clip_stage(load_library(), None, plane, attrs, clip, varyings, colors)


class _ClipCalls:
    """The clip method of Context (context.py: L and h are its own); draw() and draw_indexed() take a clip plane themselves."""

    def clip_stage(self, plane, clip, varyings=None, colors=None, attrs=None, device=False, out=None):
        """trgl_clip_stage.  Host arrays: as the module's clip_stage.  device=True: clip [n, 12] f64, varyings [n, K] f64 or None and
        colors [n] (32-bit) or None are device tensors, out = (clip_out, varyings_out, colors_out) device tensors with room for 2 n
        triangles (allocated with torch when not given); the stage runs on the context's stream and the call waits for the count.
        Returns (clip_out, varyings_out, colors_out, n_out) - only the first n_out triangles of the outputs were written."""
        if not device:
            return _host_clip_stage(self.L, self.h, plane, attrs, clip, varyings, colors)
        n = int(clip.shape[0])
        K = 0 if varyings is None else int(varyings.shape[1])
        if out is None:
            out = _triangle_outputs(2 * n, K, varyings is not None, colors, True, clip)
        ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings"), _device_ptr(colors, "colors"))
        optrs = (_device_ptr(out[0], "clip_out"), _device_ptr(out[1], "varyings_out"), _device_ptr(out[2], "colors_out"))
        m = _clip_stage(self.L, self.h, plane, attrs, K, ptrs, n, optrs, True)
        return out[0], out[1], out[2], m
