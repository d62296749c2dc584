"""TGA and OBJ: the reference's file formats, read and written on the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import TrglError, load_library
from .marshal import _check, _failure


def tga_encode(img, vflip: bool = True, rle: bool = True) -> bytes:
    """The bytes the reference's TGAImage::write_tga_file would write for an [h,w,bpp] uint8 image (host only)."""
    L = load_library()
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    h, w, bpp = img.shape
    out = np.empty(L.trgl_tga_max_size(w, h, bpp), np.uint8)
    n = C.c_size_t()
    rc = L.trgl_tga_encode(img.ctypes.data, w, h, bpp, int(vflip), int(rle), out.ctypes.data, C.byref(n))
    if rc != 0:
        raise _failure("trgl_tga_encode", rc)
    return out[:n.value].tobytes()


def tga_decode(file_bytes: bytes):
    """TGAImage::read_tga_file on a .tga file image: [h,w,bpp] uint8 in TGAImage::buffer() order (host only).
    Raises TrglError where the reference returns false."""
    L = load_library()
    buf = np.frombuffer(file_bytes, np.uint8)
    w, h, bpp = C.c_int(), C.c_int(), C.c_int()
    rc = L.trgl_tga_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(w), C.byref(h), C.byref(bpp))
    if rc != 0:
        raise TrglError(f"trgl_tga_info: not a TGA file the reference reads ({rc})")
    out = np.empty((h.value, w.value, bpp.value), np.uint8)
    rc = L.trgl_tga_decode(buf.ctypes.data, len(buf), out.ctypes.data)
    if rc != 0:
        raise _failure("trgl_tga_decode", rc)
    return out


def load_obj(path: str):
    """Wavefront OBJ -> (vertices [nv,14] f64 in the reference's Vertex layout, indices [nf,3] u32).  Host only."""
    L = load_library()
    v, i = C.POINTER(C.c_double)(), C.POINTER(C.c_uint32)()
    nv, nf = C.c_uint64(), C.c_uint64()
    _check(L, None, "trgl_obj_load", L.trgl_obj_load(path.encode(), C.byref(v), C.byref(nv), C.byref(i), C.byref(nf)))
    try:
        verts = np.ctypeslib.as_array(v, shape=(nv.value, 14)).copy() if nv.value else np.zeros((0, 14))
        idx = np.ctypeslib.as_array(i, shape=(nf.value, 3)).copy() if nf.value else np.zeros((0, 3), np.uint32)
    finally:
        L.trgl_obj_free(v, i)
    return verts, idx
