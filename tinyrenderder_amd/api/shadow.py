"""Shadow and occlusion: masks of depths against a light's depth map, the multiply by a mask, boxes against depths, and the
z-buffer snapshots both read."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import MEM_DEVICE, MEM_HOST, ShadowParams, load_library
from .marshal import _boxes_count, _check, _device_f64_any, _device_image, _device_ptr, _dp, _empty, _f64, _image_dims, _mem


def make_shadow_params(screen_to_light, bias=1e-3, darkness=0.5, pcf_radius=0) -> ShadowParams:
    """trgl_shadow_params from a row-major 4x4 (shadow_matrix), the depth bias, how much a shadowed pixel loses and the PCF radius."""
    p = ShadowParams()
    p.screen_to_light[:] = np.asarray(screen_to_light, np.float64).reshape(16).tolist()
    p.bias, p.darkness, p.pcf_radius, p.reserved = float(bias), float(darkness), int(pcf_radius), 0
    return p


def shadow_matrix(light_mv, light_proj, light_vp, cam_mv, cam_proj, cam_vp) -> np.ndarray:
    """trgl_shadow_matrix: (Lvp * Lproj * Lmv) * inverse(Cvp * Cproj * Cmv) as a row-major [4, 4] - ShadowParams.screen_to_light.
    Raises where the camera's matrix is singular.  Needs no GPU."""
    L = load_library()
    ms = [_f64(m, 16, "shadow_matrix") for m in (light_mv, light_proj, light_vp, cam_mv, cam_proj, cam_vp)]
    out = np.empty(16, np.float64)
    _check(L, None, "trgl_shadow_matrix", L.trgl_shadow_matrix(*[_dp(m) for m in ms], _dp(out)))
    return out.reshape(4, 4)


def _depth_dims(a, what):
    if len(a.shape) != 2:
        raise ValueError(f"{what} must be [h, w]")
    return int(a.shape[0]), int(a.shape[1])


def _shadow_mask_image(L, handle, params, dptr, depth, mptr, zmap, optr, device):
    h, w = _depth_dims(depth, "shadow_mask_image: depth")
    mh, mw = _depth_dims(zmap, "shadow_mask_image: map")
    _check(L, handle, "trgl_shadow_mask_image", L.trgl_shadow_mask_image(handle, C.byref(params), dptr, w, h, mptr, mw, mh, optr, _mem(device)))


def _image_modulate(L, handle, ptr, img, mptr, mask, device):
    h, w, bpp = _image_dims(img, "image_modulate")
    if tuple(mask.shape[:2]) != (h, w) or int(np.prod(tuple(mask.shape))) != h * w:
        raise ValueError("image_modulate: the mask must be [h, w] (or [h, w, 1]) like the image")
    _check(L, handle, "trgl_image_modulate", L.trgl_image_modulate(handle, ptr, w, h, bpp, mptr, _mem(device)))


def _host_shadow_mask_image(L, handle, params, depth, zmap):
    depth, zmap = np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(zmap, np.float64)
    out = np.empty(depth.shape, np.uint8)
    _shadow_mask_image(L, handle, params, depth.ctypes.data, depth, zmap.ctypes.data, zmap, out.ctypes.data, False)
    return out


def _host_image_modulate(L, handle, img, mask):
    out, mask = np.array(img, np.uint8, order="C"), np.ascontiguousarray(mask, np.uint8)
    _image_modulate(L, handle, out.ctypes.data, out, mask.ctypes.data, mask, False)
    return out


def shadow_mask_image(params: ShadowParams, depth, zmap) -> np.ndarray:
    """trgl_shadow_mask_image for host arrays without a context: the [h, w] uint8 mask of the depths [h, w] against the light's depth map
    [map_h, map_w] (the steps are written down in include/trgl.h).  Needs no GPU."""
    return _host_shadow_mask_image(load_library(), None, params, depth, zmap)


def image_modulate(img, mask) -> np.ndarray:
    """trgl_image_modulate for host arrays without a context: a copy of img [h, w, bpp] uint8 with its colour channels multiplied by
    mask [h, w] / 255 (main.cpp:775-781); alpha stays.  Needs no GPU."""
    return _host_image_modulate(load_library(), None, img, mask)


def _occlusion_boxes_image(L, handle, dptr, depth, viewport, view_proj, bptr, n, optr, device):
    h, w = _depth_dims(depth, "occlusion_boxes_image: depth")
    _check(L, handle, "trgl_occlusion_boxes_image",
           L.trgl_occlusion_boxes_image(handle, dptr, w, h, _dp(_f64(viewport, 16, "viewport")), _dp(_f64(view_proj, 16, "view_proj")), bptr, n, optr,
                                        _mem(device)))


def _host_occlusion_boxes_image(L, handle, depth, viewport, view_proj, boxes):
    depth, boxes = np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(boxes, np.float64)
    out = np.empty(_boxes_count(boxes), np.uint8)
    _occlusion_boxes_image(L, handle, depth.ctypes.data, depth, viewport, view_proj, boxes.ctypes.data, out.size, out.ctypes.data, False)
    return out


def occlusion_boxes_image(depth, viewport, view_proj, boxes) -> np.ndarray:
    """trgl_occlusion_boxes_image for host arrays without a context: one OCCL_* code (uint8) per box [n, 6] = (min.xyz, max.xyz) against
    the depths [h, w] under the row-major viewport and view_proj = Perspective * ModelView (the steps are written down in include/trgl.h).
    Bit 0 of a code set: draw the model.  Needs no GPU."""
    return _host_occlusion_boxes_image(load_library(), None, depth, viewport, view_proj, boxes)


class _ShadowCalls:
    """The shadow, occlusion and depth snapshot methods of Context (context.py: L, h, _chk and _hold are its own)."""

    def shadow_mask_image(self, params, depth, zmap, device=False, out=None):
        """trgl_shadow_mask_image; returns the [h, w] uint8 mask.  Host arrays: no GPU work.  device=True: contiguous float64 device tensors
        [h, w] and [map_h, map_w], masked on the context's stream in order with everything else (nothing is flushed, the call does not
        wait); `out` is allocated with torch when not given."""
        if not device:
            return _host_shadow_mask_image(self.L, self.h, params, depth, zmap)
        _device_f64_any(depth, "depth"); _device_f64_any(zmap, "zmap")
        if out is None:
            out = _empty(tuple(depth.shape), np.uint8, True, depth)
        elif tuple(out.shape) != tuple(depth.shape):
            raise ValueError("shadow_mask_image: out must be [h, w]")
        self._hold(True, (depth, zmap, out))
        _shadow_mask_image(self.L, self.h, params, _device_ptr(depth, "depth"), depth, _device_ptr(zmap, "zmap"), zmap, _device_image(out, "out"), True)
        return out

    def image_modulate(self, img, mask, device=False):
        """trgl_image_modulate; returns the multiplied image.  Host arrays: computed on a copy.  device=True: contiguous uint8 device tensors
        [h, w, bpp] and [h, w], img multiplied in place on the context's stream (nothing is flushed, the call does not wait)."""
        if not device:
            return _host_image_modulate(self.L, self.h, img, mask)
        ptr, mptr = _device_image(img, "img"), _device_image(mask, "mask")
        self._hold(True, (img, mask))
        _image_modulate(self.L, self.h, ptr, img, mptr, mask, True)
        return img

    def shadow_mask(self, params, slot=0, out=None, device=False):
        """trgl_shadow_mask: the mask of the resident z-buffer against the depths of snapshot `slot` (flushes what is queued).  Returns a
        [H, W] uint8 numpy array (the call waits for it), or with device=True a device tensor (allocated with torch when `out` is not
        given; the call does not wait).  Not on a strip / band context."""
        if device:
            if out is None:
                out = _empty((self.height, self.width), np.uint8, True, f"cuda:{self.device}")
            ptr = _device_image(out, "out")
            self._hold(True, (out,))
        else:
            if out is None:
                out = np.empty((self.height, self.width), np.uint8)
            if out.dtype != np.uint8 or not out.flags.c_contiguous:
                raise ValueError("shadow_mask: out must be a contiguous uint8 array")
            ptr = out.ctypes.data
        if int(np.prod(tuple(out.shape))) != self.width * self.height:
            raise ValueError("shadow_mask: out must hold W * H bytes")
        self._chk(self.L.trgl_shadow_mask(self.h, C.byref(params), int(slot), ptr, _mem(device)))
        return out

    def framebuffer_modulate(self, mask, device=False):
        """trgl_framebuffer_modulate: the resident frame multiplied by mask [H, W] / 255 in place (flushes what is queued, does not wait);
        the z-buffer and the stats stay as they are.  mask: a host array, or with device=True a contiguous uint8 device tensor."""
        if device:
            ptr = _device_image(mask, "mask")
            self._hold(True, (mask,))
        else:
            mask = np.ascontiguousarray(mask, np.uint8)
            ptr = mask.ctypes.data
        if int(np.prod(tuple(mask.shape))) != self.width * self.height:
            raise ValueError("framebuffer_modulate: the mask must hold W * H bytes")
        self._chk(self.L.trgl_framebuffer_modulate(self.h, ptr, _mem(device)))

    def occlusion_boxes_image(self, depth, viewport, view_proj, boxes, device=False, out=None):
        """trgl_occlusion_boxes_image; returns the [n] uint8 codes.  Host arrays: no GPU work.  device=True: depth [h, w] and boxes [n, 6] are
        contiguous float64 device tensors, queried on the context's stream in order with everything else (nothing is flushed, the call
        does not wait); `out` (uint8 [n], any alignment) is allocated with torch when not given."""
        if not device:
            return _host_occlusion_boxes_image(self.L, self.h, depth, viewport, view_proj, boxes)
        _device_f64_any(depth, "depth"); _device_f64_any(boxes, "boxes")
        n = _boxes_count(boxes)
        if out is None:
            out = _empty(n, np.uint8, True, boxes)
        elif tuple(out.shape) != (n,):
            raise ValueError("occlusion_boxes_image: out must be [n]")
        self._hold(True, (depth, boxes, out))
        _occlusion_boxes_image(self.L, self.h, _device_ptr(depth, "depth"), depth, viewport, view_proj, _device_ptr(boxes, "boxes"), n,
                               _device_image(out, "out"), True)
        return out

    def occlusion_boxes(self, view_proj, boxes, snapshot=None, device=False):
        """trgl_occlusion_boxes: one OCCL_* code per box [n, 6] against the resident z-buffer (snapshot=None) or the depths of a snapshot
        slot, under the context's viewport (flushes what is queued).  Host boxes give a uint8 numpy array (the call waits for it);
        device=True takes a contiguous float64 device tensor and returns a device tensor without waiting.  Not on a strip / band context."""
        if not device:
            boxes = np.ascontiguousarray(boxes, np.float64)
        n = _boxes_count(boxes)
        m = _dp(_f64(view_proj, 16, "view_proj"))
        slot = -1 if snapshot is None else int(snapshot)
        if device:
            _device_f64_any(boxes, "boxes")
            out = _empty(n, np.uint8, True, boxes)
            self._hold(True, (boxes, out))
            self._chk(self.L.trgl_occlusion_boxes(self.h, m, _device_ptr(boxes, "boxes"), n, MEM_DEVICE, slot, _device_ptr(out, "out"), MEM_DEVICE))
            return out
        out = np.empty(n, np.uint8)
        self._chk(self.L.trgl_occlusion_boxes(self.h, m, boxes.ctypes.data, n, MEM_HOST, slot, out.ctypes.data, MEM_HOST))
        return out

    def zbuffer_snapshot(self, slot=0):
        """trgl_zbuffer_snapshot: main.cpp:700 as one device-to-device copy (flushes what is queued, does not wait)."""
        self._chk(self.L.trgl_zbuffer_snapshot(self.h, int(slot)))

    def zbuffer_restore(self, slot=0):
        """trgl_zbuffer_restore: main.cpp:730 likewise; the framebuffer and the stats stay as they are."""
        self._chk(self.L.trgl_zbuffer_restore(self.h, int(slot)))

    def zbuffer_snapshot_free(self, slot=0):
        self._chk(self.L.trgl_zbuffer_snapshot_free(self.h, int(slot)))
