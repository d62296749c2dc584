"""The one copy of what every family does on the way into the library: failures into TrglError, addresses of host and device
arrays, the checks and coercions of the common array kinds, and the allocation of outputs where the inputs are."""
import ctypes as C

import numpy as np

from .loader import MEM_DEVICE, MEM_HOST, TrglError


# ---- failures ----
def _failure(name, rc, detail=None):
    """The TrglError of a call that returned rc: `<name> failed (<rc>)`, then `: <detail>` when there is one."""
    return TrglError(f"{name} failed ({rc})" + ("" if detail is None else f": {detail}"))


def _check(L, handle, name, rc):
    """Raise for rc != 0 with the library's last error: that of the context `handle`, or with None that of the calling thread."""
    if rc != 0:
        raise _failure(name, rc, L.trgl_last_error(handle).decode())


# ---- addresses ----
def _mem(device):
    return MEM_DEVICE if device else MEM_HOST


def _ptr(a):
    """host numpy array, or an object with a device pointer (torch tensor / int)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


def _device_ptr(a, what="array"):
    """The address of an array handed over with device=True: an int (a raw device pointer), or an object with data_ptr() whose
    is_cuda is true (a torch CUDA tensor); None stays None.  Anything else - a numpy array, a CPU tensor - raises TypeError
    before the library is called: its address would reach a kernel as it is."""
    if a is None:
        return None
    if isinstance(a, int) and not isinstance(a, bool):
        return a
    if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) is True:
        return a.data_ptr()
    raise TypeError(f"device=True: {what} must be a device tensor or an int device pointer, not {type(a).__name__}"
                    + (" in host memory" if hasattr(a, "data_ptr") else ""))


def _ptr_of(device):
    """The address function of a call's arrays: _device_ptr with device=True, so that a host array among them is a TypeError."""
    return _device_ptr if device else _ptr


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ref(struct):
    """A structure by reference; None stays None (NULL: the call's default)."""
    return None if struct is None else C.byref(struct)


# ---- array kinds ----
def _f64(a, n, what):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{what}: {n} doubles expected, got {a.size}")
    return a


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) is True


def _device_f64(t, ndim, what):
    if not _is_device_tensor(t) or str(t.dtype) != "torch.float64" or not t.is_contiguous() or t.dim() != ndim:
        raise ValueError(f"{what} must be a contiguous float64 device tensor with {ndim} dimensions (the other arrays are in device memory)")
    return t


def _device_f64_any(t, what):
    """The older check of the shadow and occlusion calls: any rank, and a tensor in host memory passes - it is _device_ptr's
    TypeError afterwards."""
    if not hasattr(t, "data_ptr") or str(t.dtype) != "torch.float64" or not t.is_contiguous():
        raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor")
    return t


def _vertices_f64(vertices, device, what="vertices"):
    """Records [n, stride] of doubles: a device tensor with device=True, else a contiguous numpy array."""
    if device:
        return _device_f64(vertices, 2, what)
    vertices = np.ascontiguousarray(vertices, np.float64)
    if vertices.ndim != 2:
        raise ValueError(f"{what} must have 2 dimensions [n, stride]")
    return vertices


def _words32(a, device, what, cols=None):
    """A 32-bit array as the edge calls take it: a contiguous device tensor with device=True, else a numpy uint32 array."""
    if device:
        if not _is_device_tensor(a) or a.element_size() != 4 or not a.is_contiguous():
            raise ValueError(f"device=True: {what} must be a contiguous 32-bit device tensor")
        return a
    a = np.ascontiguousarray(a, np.uint32)
    return a if cols is None else a.reshape(-1, cols)


def _image_dims(img, what):
    if len(img.shape) != 3 or img.shape[2] not in (1, 3, 4):
        raise ValueError(f"{what}: the image must be [h, w, bpp] with bpp in (1, 3, 4)")
    return int(img.shape[0]), int(img.shape[1]), int(img.shape[2])


def _device_image(img, what):
    """The address of a device image: a contiguous uint8 CUDA tensor (its shape says w, h and bpp, so a bare pointer will not do)."""
    if not hasattr(img, "data_ptr"):
        raise TypeError(f"device=True: {what} must be a device tensor, not {type(img).__name__}")
    if str(img.dtype) != "torch.uint8" or not img.is_contiguous():
        raise ValueError(f"device=True: {what} must be a contiguous uint8 tensor")
    return _device_ptr(img, what)


def _boxes_count(boxes):
    if len(boxes.shape) != 2 or boxes.shape[1] != 6:
        raise ValueError("occlusion: boxes must be [n, 6] (min.xyz, max.xyz)")
    return int(boxes.shape[0])


def _count(a):
    """The elements of a numpy array or a tensor."""
    return int(a.numel() if hasattr(a, "numel") else a.size)


# ---- outputs ----
_TORCH_DTYPE = {np.float64: "float64", np.uint32: "int32", np.uint8: "uint8"}      # (torch has no uint32 arithmetic: the bits are uint32)


def _empty(shape, dtype, device, where=None):
    """A new array where a call's inputs are: np.empty, or with device=True torch.empty on the device of the tensor `where` (or on
    `where` itself, a device name).  dtype is numpy's - uint32 is torch.int32 there - or, for a device array, already torch's."""
    if not device:
        return np.empty(shape, dtype)
    import torch
    name = _TORCH_DTYPE.get(dtype)
    return torch.empty(shape, dtype=dtype if name is None else getattr(torch, name), device=getattr(where, "device", where))


def _triangle_outputs(rows, K, with_varyings, colors, device, where):
    """(clip_out [rows, 12], varyings_out [rows, K] or None, colors_out [rows] with the 32-bit type of `colors`, or None)"""
    return (_empty((rows, 12), np.float64, device, where), _empty((rows, K), np.float64, device, where) if with_varyings else None,
            None if colors is None else _empty(rows, colors.dtype if device else np.uint32, device, where))


def _named_outputs(names, out, shapes, device, where, what):
    """The outputs of a weld, clean or simplify call as a dict over `names`: out - None for all of them, or a dict naming those to
    write, each an array or None to allocate it; one that is not named is not written (NULL)."""
    if out is None:
        out = {k: None for k in names}
    unknown = set(out) - set(names)
    if unknown:
        raise ValueError(f"{what}: unknown outputs {sorted(unknown)}")
    res = {}
    for k in names:
        if k not in out:
            res[k] = None
        elif out[k] is not None:
            res[k] = out[k]
        else:
            res[k] = _empty(shapes[k], np.float64 if k == "vertices" else np.uint32, device, where)
    return res
