"""Images, resolve and mip chains: blur, scale, box filter, frames as textures, mip levels and their level-of-detail stage."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import MAX_MIP_LEVELS, MEM_DEVICE, MEM_HOST, SAMPLE_TRILINEAR, load_library
from .marshal import _check, _device_image, _dp, _empty, _image_dims, _is_device_tensor, _mem


def gaussian_kernel(radius: int) -> np.ndarray:
    """trgl_gaussian_kernel: the 2 * radius + 1 float32 weights of TGAImage::gaussian_blur (tgaimage.cpp:275-284), computed on the host as
    the reference computes them.  Needs no GPU."""
    L = load_library()
    out = np.empty(2 * max(int(radius), 0) + 1, np.float32)
    _check(L, None, "trgl_gaussian_kernel", L.trgl_gaussian_kernel(int(radius), out.ctypes.data))
    return out


def _image_blur(L, handle, ptr, img, radius, device):
    h, w, bpp = _image_dims(img, "image_blur")
    _check(L, handle, "trgl_image_blur", L.trgl_image_blur(handle, ptr, w, h, bpp, int(radius), _mem(device)))


def _image_scale(L, handle, sptr, img, dptr, w2, h2, device):
    h, w, bpp = _image_dims(img, "image_scale")
    _check(L, handle, "trgl_image_scale", L.trgl_image_scale(handle, sptr, w, h, bpp, dptr, int(w2), int(h2), _mem(device)))


def _image_downsample(L, handle, sptr, img, factor, dptr, device):
    h, w, bpp = _image_dims(img, "image_downsample")
    _check(L, handle, "trgl_image_downsample", L.trgl_image_downsample(handle, sptr, w, h, bpp, int(factor), dptr, _mem(device)))


def _box_shape(img, factor):
    """[h2, w2, bpp] of the box filter's result; zeros where the library will refuse the factor."""
    f = int(factor)
    ok = len(img.shape) == 3 and f >= 1
    return (int(img.shape[0]) // f if ok else 0, int(img.shape[1]) // f if ok else 0, int(img.shape[2]) if len(img.shape) == 3 else 0)


def _host_image_downsample(L, handle, img, factor, out=None):
    src = np.ascontiguousarray(img, np.uint8)
    shape = _box_shape(src, factor)
    if out is None:
        out = np.empty(shape, np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != shape:
        raise ValueError("image_downsample: out must be a contiguous uint8 array [h // factor, w // factor, bpp]")
    _image_downsample(L, handle, src.ctypes.data, src, factor, out.ctypes.data, False)
    return out


def image_blur(img, radius: int) -> np.ndarray:
    """trgl_image_blur for a host array without a context: TGAImage::gaussian_blur (tgaimage.cpp:271-324) on a copy of img [h, w, bpp] uint8;
    returns the copy.  radius <= 0 returns it unchanged, as the reference does.  Needs no GPU."""
    out = np.array(img, np.uint8, order="C")
    _image_blur(load_library(), None, out.ctypes.data, out, radius, False)
    return out


def image_scale(img, w2: int, h2: int) -> np.ndarray:
    """trgl_image_scale for a host array without a context: TGAImage::scale (tgaimage.cpp:246-267) of img [h, w, bpp] uint8 into a new
    [h2, w2, bpp] array.  Raises where the reference returns false (a size <= 0, an empty image).  Needs no GPU."""
    src = np.ascontiguousarray(img, np.uint8)
    out = np.empty((max(int(h2), 0), max(int(w2), 0), src.shape[2] if len(src.shape) == 3 else 0), np.uint8)
    _image_scale(load_library(), None, src.ctypes.data, src, out.ctypes.data, w2, h2, False)
    return out


def image_downsample(img, factor: int) -> np.ndarray:
    """trgl_image_downsample for a host array without a context: the exact box filter (new work, include/trgl.h) of img [h, w, bpp] uint8
    into a new [h // factor, w // factor, bpp] array: (sum of factor x factor bytes + factor * factor // 2) // (factor * factor) per
    channel.  Raises for a factor outside 1..16 or above w or h.  Needs no GPU."""
    return _host_image_downsample(load_library(), None, img, factor)


def mip_layout(w: int, h: int, bpp: int):
    """trgl_mip_layout: (widths, heights, offsets, total) of the mip chain of a w x h image - the sizes of all L levels, the byte offsets of
    levels 1 .. L-1 in the packed buffer (offsets[0] is 0 and names nothing) and that buffer's bytes.  Needs no GPU."""
    L = load_library()
    n, total = C.c_int(), C.c_size_t()
    ws, hs, offs = (C.c_int * MAX_MIP_LEVELS)(), (C.c_int * MAX_MIP_LEVELS)(), (C.c_size_t * MAX_MIP_LEVELS)()
    _check(L, None, "trgl_mip_layout", L.trgl_mip_layout(int(w), int(h), int(bpp), C.byref(n), ws, hs, offs, C.byref(total)))
    return list(ws[:n.value]), list(hs[:n.value]), list(offs[:n.value]), int(total.value)


def _image_mipmaps(L, handle, sptr, img, dptr, device):
    h, w, bpp = _image_dims(img, "image_mipmaps")
    _check(L, handle, "trgl_image_mipmaps", L.trgl_image_mipmaps(handle, sptr, w, h, bpp, dptr, _mem(device)))


def _host_image_mipmaps(L, handle, img, out=None):
    src = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = _image_dims(src, "image_mipmaps")
    total = mip_layout(w, h, bpp)[3]
    if out is None:
        out = np.zeros(total, np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (total,):
        raise ValueError("image_mipmaps: out must be a contiguous uint8 array of mip_layout(w, h, bpp)[3] bytes")
    _image_mipmaps(L, handle, src.ctypes.data, src, out.ctypes.data, False)
    return out


def image_mipmaps(img) -> np.ndarray:
    """trgl_image_mipmaps for a host array without a context: levels 1 .. L-1 of img [h, w, bpp] uint8 as one packed uint8 array in the
    layout of mip_layout (the padding between levels is zero here: the array is new).  Needs no GPU."""
    return _host_image_mipmaps(load_library(), None, img)


def image_sample(img, chain, uv, lod, mode=SAMPLE_TRILINEAR, levels=None) -> np.ndarray:
    """trgl_image_sample: the filtered samplers of the user shaders on the host, over img [h, w, bpp] uint8 and its packed chain (None:
    one level) at uv [n, 2] and lod [n]; mode SAMPLE_LEVEL / SAMPLE_LINEAR (lod converted to int) / SAMPLE_TRILINEAR.  Returns [n, 5]
    uint8 = bgra[4], bytespp, as selftest_sampler does.  Needs no GPU."""
    L = load_library()
    src = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = _image_dims(src, "image_sample")
    chain = None if chain is None else np.ascontiguousarray(chain, np.uint8)
    if levels is None:
        levels = 1 if chain is None else MAX_MIP_LEVELS
    if chain is not None and int(levels) > 1 and chain.size < mip_layout(w, h, bpp)[3]:
        raise ValueError("image_sample: chain is shorter than mip_layout(w, h, bpp)[3] bytes")
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    lod = np.ascontiguousarray(np.broadcast_to(np.asarray(lod, np.float64), (uv.shape[0],)))
    out = np.zeros((uv.shape[0], 5), np.uint8)
    _check(L, None, "trgl_image_sample",
           L.trgl_image_sample(src.ctypes.data, None if chain is None else chain.ctypes.data, w, h, bpp, int(levels), uv.ctypes.data, lod.ctypes.data,
                               int(mode), uv.shape[0], out.ctypes.data))
    return out


def mip_lod(bar, k, tex_w: int, tex_h: int) -> np.ndarray:
    """trgl_selftest_mip_lod: the host's compile of the user shaders' trgl_mip_lod over bar [n, 3] and k [n, 4]; returns [n] float64 levels
    of detail for a tex_w x tex_h texture.  Needs no GPU."""
    L = load_library()
    bar = np.ascontiguousarray(bar, np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.float64), (bar.shape[0], 4)))
    out = np.zeros(bar.shape[0], np.float64)
    _check(L, None, "trgl_selftest_mip_lod", L.trgl_selftest_mip_lod(bar.ctypes.data, k.ctypes.data, int(tex_w), int(tex_h), bar.shape[0], out.ctypes.data))
    return out


def _lod_stage(L, handle, viewport, clip, varyings, uv_offset, out_offset, device):
    """In place on `varyings`; returns the arrays to keep alive."""
    vp_m = np.ascontiguousarray(viewport, np.float64).reshape(16)
    if device:
        for a, what in ((clip, "clip"), (varyings, "varyings")):
            if not _is_device_tensor(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.dim() != 2:
                raise ValueError(f"device=True: {what} must be a contiguous float64 device tensor with 2 dimensions")
        n, K = int(clip.shape[0]), int(varyings.shape[1])
        if int(clip.shape[1]) != 12 or int(varyings.shape[0]) != n:
            raise ValueError("lod_stage: clip must be [n, 12] and varyings [n, K]")
        ptrs = (clip.data_ptr() if n else None, varyings.data_ptr() if n else None)
    else:
        if not isinstance(varyings, np.ndarray) or varyings.dtype != np.float64 or not varyings.flags.c_contiguous or varyings.ndim != 2:
            raise ValueError("lod_stage: varyings must be a contiguous float64 array [n, K] (it is rewritten in place)")
        clip = np.ascontiguousarray(clip, np.float64).reshape(-1, 12)
        n, K = clip.shape[0], varyings.shape[1]
        if varyings.shape[0] != n:
            raise ValueError("lod_stage: clip must be [n, 12] and varyings [n, K]")
        ptrs = (clip.ctypes.data if n else None, varyings.ctypes.data if n else None)
    _check(L, handle, "trgl_lod_stage", L.trgl_lod_stage(handle, _dp(vp_m), ptrs[0], ptrs[1], n, K, int(uv_offset), int(out_offset), _mem(device)))
    return clip, varyings


def lod_stage(viewport, clip, varyings, uv_offset=0, out_offset=6):
    """trgl_lod_stage for host arrays without a context: for every triangle of clip [n, 12] the four level-of-detail doubles
    (c, W0, W1, W2) from its clip row, the Viewport [4, 4] and its six uv doubles at varyings[:, uv_offset:uv_offset + 6], written in place
    at varyings[:, out_offset:out_offset + 4] (a contiguous float64 array [n, K]); returns varyings.  Needs no GPU."""
    return _lod_stage(load_library(), None, viewport, clip, varyings, uv_offset, out_offset, False)[1]


class _ImageCalls:
    """The image, resolve and mip methods of Context (context.py: L, h, _chk and _hold are its own)."""

    def image_blur(self, img, radius, device=False):
        """trgl_image_blur: TGAImage::gaussian_blur (tgaimage.cpp:271-324); returns the blurred image.  Host array: computed on a copy, no
        GPU work.  device=True: a contiguous uint8 device tensor [h, w, bpp], blurred in place on the context's stream in order with
        everything else (nothing is flushed, the call does not wait); the tensor is kept alive until the next sync."""
        if not device:
            out = np.array(img, np.uint8, order="C")
            _image_blur(self.L, self.h, out.ctypes.data, out, radius, False)
            return out
        ptr = _device_image(img, "img")
        self._hold(True, (img,))
        _image_blur(self.L, self.h, ptr, img, radius, True)
        return img

    def image_scale(self, img, w2, h2, device=False, out=None):
        """trgl_image_scale: TGAImage::scale (tgaimage.cpp:246-267) of img [h, w, bpp] into [h2, w2, bpp]; returns the result.  device=True:
        contiguous uint8 device tensors, gathered on the context's stream (nothing is flushed, the call does not wait); `out` (must not
        overlap img) is allocated with torch when not given.  Raises where the reference returns false."""
        if not device:
            src = np.ascontiguousarray(img, np.uint8)
            if out is None:
                out = np.empty((max(int(h2), 0), max(int(w2), 0), src.shape[2] if len(src.shape) == 3 else 0), np.uint8)
            if out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (int(h2), int(w2), src.shape[2]):
                raise ValueError("image_scale: out must be a contiguous uint8 array [h2, w2, bpp]")
            _image_scale(self.L, self.h, src.ctypes.data, src, out.ctypes.data, w2, h2, False)
            return out
        sptr = _device_image(img, "img")
        if out is None:
            out = _empty((max(int(h2), 0), max(int(w2), 0), int(img.shape[2])), np.uint8, True, img)
        elif tuple(out.shape) != (int(h2), int(w2), int(img.shape[2])):
            raise ValueError("image_scale: out must be [h2, w2, bpp]")
        self._hold(True, (img, out))
        _image_scale(self.L, self.h, sptr, img, _device_image(out, "out"), w2, h2, True)
        return out

    def image_downsample(self, img, factor, device=False, out=None):
        """trgl_image_downsample: the exact box filter of img [h, w, bpp] into [h // factor, w // factor, bpp]; returns the result.
        Host array: no GPU work.  device=True: contiguous uint8 device tensors at any address, filtered on the context's stream (nothing is
        flushed, the call does not wait); `out` (must not overlap img) is allocated with torch when not given; both are kept alive until
        the next sync."""
        if not device:
            return _host_image_downsample(self.L, self.h, img, factor, out)
        sptr = _device_image(img, "img")
        shape = _box_shape(img, factor)
        if out is None:
            out = _empty(shape, np.uint8, True, img)
        elif tuple(out.shape) != shape:
            raise ValueError("image_downsample: out must be [h // factor, w // factor, bpp]")
        self._hold(True, (img, out))
        _image_downsample(self.L, self.h, sptr, img, factor, _device_image(out, "out"), True)
        return out

    def framebuffer_resolve(self, factor, device=False, out=None):
        """trgl_framebuffer_resolve: the SSAA resolve - flushes what is queued (a pending clear included), then box-filters the resident
        frame into [H // factor, W // factor, bpp]; the frame, the z-buffer and the stats stay as they are.  device=False: a numpy array,
        the call waits for the small image.  device=True: a uint8 tensor on the context's device (allocated with torch when `out` is
        not given), queued without waiting and kept alive until the next sync.  Not on a strip / band context."""
        f = int(factor)
        shape = (self.height // f if f >= 1 else 0, self.width // f if f >= 1 else 0, self.bpp)
        if not device:
            if out is None:
                out = np.empty(shape, np.uint8)
            elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != shape:
                raise ValueError("framebuffer_resolve: out must be a contiguous uint8 array [H // factor, W // factor, bpp]")
            self._chk(self.L.trgl_framebuffer_resolve(self.h, f, out.ctypes.data, MEM_HOST))
            return out
        if out is None:
            out = _empty(shape, np.uint8, True, f"cuda:{self.device}")
        elif tuple(out.shape) != shape:
            raise ValueError("framebuffer_resolve: out must be [H // factor, W // factor, bpp]")
        ptr = _device_image(out, "out")
        self._hold(True, (out,))
        self._chk(self.L.trgl_framebuffer_resolve(self.h, f, ptr, MEM_DEVICE))
        return out

    def texture_from_image(self, slot, img, factor=1, device=False):
        """trgl_texture_from_image: the box filter of img [h, w, bpp] (a [h, w] image counts as bpp 1) becomes the texture of `slot`, ordered
        like upload_texture: draws submitted earlier sample the old texture.  device=True: a contiguous uint8 device tensor, filtered in
        HBM without a host wait when the slot is empty or holds a texture of the same size; kept alive until the next sync."""
        if not device:
            t = np.ascontiguousarray(img, np.uint8)
            if t.ndim == 2:
                t = t[..., None]
            h, w, bpp = _image_dims(t, "texture_from_image")
            self._chk(self.L.trgl_texture_from_image(self.h, int(slot), t.ctypes.data, w, h, bpp, int(factor), MEM_HOST))
            return
        ptr = _device_image(img, "img")
        h, w, bpp = _image_dims(img, "texture_from_image")
        self._hold(True, (img,))
        self._chk(self.L.trgl_texture_from_image(self.h, int(slot), ptr, w, h, bpp, int(factor), MEM_DEVICE))

    def texture_from_framebuffer(self, slot, factor=1):
        """trgl_texture_from_framebuffer: render-to-texture - flushes what is queued, then the box filter of the resident frame becomes the
        texture of `slot` [H // factor, W // factor, bpp], a snapshot that later clears and draws do not change.  No host wait when the
        slot is empty or holds a texture of that size.  Not on a strip / band context."""
        self._chk(self.L.trgl_texture_from_framebuffer(self.h, int(slot), int(factor)))

    def texture_mipmaps(self, slot):
        """trgl_texture_mipmaps: builds the mip chain of the texture in `slot`, ordered like the other texture calls (draws submitted earlier
        sample one level).  Every call that replaces the slot's texels drops the chain; a rebuild on a slot that has held one of this size
        is kernels on the stream without a host wait."""
        self._chk(self.L.trgl_texture_mipmaps(self.h, int(slot)))

    def image_mipmaps(self, img, device=False, out=None):
        """trgl_image_mipmaps: levels 1 .. L-1 of img [h, w, bpp] as one packed uint8 array (see mip_layout); returns it.  Host array: no
        GPU work.  device=True: contiguous uint8 device tensors at any address, built on the context's stream (nothing is flushed, the call
        does not wait); `out` (1-D, mip_layout(w, h, bpp)[3] bytes, not overlapping img; only the levels' bytes are written) is allocated
        zeroed with torch when not given; both are kept alive until the next sync."""
        if not device:
            return _host_image_mipmaps(self.L, self.h, img, out)
        sptr = _device_image(img, "img")
        h, w, bpp = _image_dims(img, "image_mipmaps")
        total = mip_layout(w, h, bpp)[3]
        if out is None:
            import torch
            out = torch.zeros(total, dtype=torch.uint8, device=img.device)      # (zeroed: the padding between the levels is not written)
        elif tuple(out.shape) != (total,):
            raise ValueError("image_mipmaps: out must be 1-D with mip_layout(w, h, bpp)[3] bytes")
        self._hold(True, (img, out))
        _image_mipmaps(self.L, self.h, sptr, img, _device_image(out, "out") if total else None, True)
        return out

    def lod_stage(self, viewport, clip, varyings, uv_offset=0, out_offset=6, device=False):
        """trgl_lod_stage (see the module's lod_stage): in place on varyings [n, K]; returns it.  device=True: contiguous float64 device
        tensors, queued on the context's stream in order with the draws (no wait, no flush), kept alive until the next sync."""
        clip, varyings = _lod_stage(self.L, self.h, viewport, clip, varyings, uv_offset, out_offset, device)
        self._hold(device, (clip, varyings))
        return varyings

    def framebuffer_blur(self, radius):
        """trgl_framebuffer_blur: framebuffer.gaussian_blur(radius) on the resident frame (flushes what is queued, does not wait); the
        z-buffer and the stats stay as they are.  Not on a strip / band context."""
        self._chk(self.L.trgl_framebuffer_blur(self.h, int(radius)))
