"""Triangle order: a depth per group of triangles and the gather that puts their rows in a drawing order."""
from __future__ import annotations

import numpy as np

from .loader import TRI_DEPTH_CENTROID, load_library
from .marshal import _check, _device_ptr, _empty, _is_device_tensor, _mem, _ptr, _triangle_outputs


def _triangle_depths(L, handle, clip, group, mode, device):
    """Returns (the clip array to keep alive, depths [n / group])."""
    group = int(group)
    if device:
        if not _is_device_tensor(clip) or str(clip.dtype) != "torch.float64" or not clip.is_contiguous() or clip.numel() % 12:
            raise ValueError("device=True: clip must be a contiguous float64 device tensor [n, 12]")
        n = clip.numel() // 12
        out = _empty(n // max(group, 1), np.float64, True, clip)
        ptrs = (clip.data_ptr() if n else None, out.data_ptr() if out.numel() else None)
    else:
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n = clip.shape[0]
        out = np.empty(n // max(group, 1), np.float64)
        ptrs = (clip.ctypes.data, out.ctypes.data)
    _check(L, handle, "trgl_triangle_depths", L.trgl_triangle_depths(handle, ptrs[0], n, group, int(mode), _mem(device), ptrs[1]))
    return clip, out


def _order_stage(L, handle, clip, varyings, colors, order, group, device, out):
    """Returns (arrays to keep alive, (clip_out, varyings_out, colors_out)) - n_order * group rows each."""
    group = int(group)
    if device:
        for a, what in ((clip, "clip"), (varyings, "varyings")):
            if a is not None and (not _is_device_tensor(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.dim() != 2):
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor with 2 dimensions")
        for a, what in ((colors, "colors"), (order, "order")):
            if a is not None and (not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous() or a.dim() != 1):
                raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor with 1 dimension")
        n, n_order = int(clip.shape[0]), int(order.shape[0])
        K = 0 if varyings is None else int(varyings.shape[1])
        if out is None:
            out = _triangle_outputs(n_order * group, K, K != 0, colors, True, clip)
        ptrs = (_device_ptr(clip, "clip"), _device_ptr(varyings, "varyings") if K else None, _device_ptr(colors, "colors"), _device_ptr(order, "order"))
        optrs = (_device_ptr(out[0], "clip_out"), _device_ptr(out[1], "varyings_out") if K else None, _device_ptr(out[2], "colors_out"))
    else:
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n = clip.shape[0]
        varyings = None if varyings is None else np.ascontiguousarray(varyings, np.float64).reshape(n, -1)
        K = 0 if varyings is None else varyings.shape[1]
        colors = None if colors is None else np.ascontiguousarray(colors, np.uint32).reshape(n)
        order = np.ascontiguousarray(order, np.uint32).reshape(-1)
        n_order = order.shape[0]
        if out is None:
            out = _triangle_outputs(n_order * group, K, K != 0, colors, False, None)
        ptrs = (_ptr(clip), _ptr(varyings) if K else None, _ptr(colors), _ptr(order))
        optrs = (_ptr(out[0]), _ptr(out[1]) if K else None, _ptr(out[2]))
    _check(L, handle, "trgl_order_stage",
           L.trgl_order_stage(handle, K, ptrs[0], ptrs[1], ptrs[2], n, ptrs[3], n_order, group, _mem(device), optrs[0], optrs[1], optrs[2]))
    return (clip, varyings, colors, order), out


def triangle_depths(clip, group=1, mode=TRI_DEPTH_CENTROID) -> np.ndarray:
    """trgl_triangle_depths for a host array without a context: one depth per group of `group` consecutive triangles of clip [n, 12],
    from the clip w of the group's vertices - their sum (CENTROID), their smallest (NEAREST) or their largest (FARTHEST), negated, so
    that depth_order's default direction draws the farthest group first.  Needs no GPU."""
    return _triangle_depths(load_library(), None, clip, group, mode, False)[1]


def order_stage(clip, varyings=None, colors=None, order=(), group=1):
    """trgl_order_stage for host arrays without a context: the rows of the groups that `order` names, in that order - output group p is
    input group order[p].  Returns (clip, varyings, colors) with len(order) * group rows (None where the input is None).  Needs no GPU."""
    return _order_stage(load_library(), None, clip, varyings, colors, order, group, False, None)[1]


class _OrderCalls:
    """The triangle order methods of Context (context.py: L, h and _hold are its own); draw(order=) is the fused call."""

    def triangle_depths(self, clip, group=1, mode=TRI_DEPTH_CENTROID, device=False):
        """trgl_triangle_depths: one depth per group of `group` consecutive triangles of clip [n, 12] (see the module's triangle_depths).
        Host array: a numpy array, no GPU work.  device=True: clip is a contiguous float64 device tensor; the depths come back as a
        device tensor, queued on the context's stream without waiting - pass them to depth_order(device=True)."""
        clip, out = _triangle_depths(self.L, self.h, clip, group, mode, device)
        self._hold(device, (clip, out))
        return out

    def order_stage(self, clip, varyings=None, colors=None, order=(), group=1, device=False, out=None):
        """trgl_order_stage: the rows of the groups that `order` names, in that order.  Host arrays: as the module's order_stage.
        device=True: clip [n, 12] f64, varyings [n, K] f64 or None, colors [n] (32-bit) or None and order [n_order] (32-bit) are device
        tensors, out = (clip_out, varyings_out, colors_out) device tensors with len(order) * group rows (allocated with torch when not
        given); the gather is queued on the context's stream without waiting, and an entry of the list that names no group gives
        all-zero rows.  Returns (clip_out, varyings_out, colors_out)."""
        keep, out = _order_stage(self.L, self.h, clip, varyings, colors, order, group, device, out)
        self._hold(device, (keep, out))
        return out
