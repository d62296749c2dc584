"""Instances, boxes and depth order: instanced draws of an indexed mesh, their world boxes and frustum codes, and the order
that draws them by depth."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import FRUSTUM_MERGE, FRUSTUM_SET, ORDER_BACK_TO_FRONT, ORDER_FRONT_TO_BACK, PHONG, VARY, load_library
from .marshal import _boxes_count, _check, _device_f64, _device_ptr, _dp, _empty, _f64, _is_device_tensor, _mem, _ptr, _ref


def _instance_depths(L, handle, model_view, point, instances, device):
    mv, pt = _f64(model_view, 16, "model_view"), _f64(point, 3, "point")
    if device:
        if not hasattr(instances, "data_ptr") or str(instances.dtype) != "torch.float64" or not instances.is_contiguous() or instances.dim() != 2:
            raise ValueError("device=True: instances must be a contiguous float64 device tensor [n, stride]")
        out = _empty(int(instances.shape[0]), np.float64, True, instances)
        ptrs = (_device_ptr(instances, "instances") if out.numel() else None, out.data_ptr() if out.numel() else None)
    else:
        instances = np.ascontiguousarray(instances, np.float64)
        if instances.ndim != 2:
            raise ValueError("instances: [n, stride] expected")
        out = np.empty(instances.shape[0], np.float64)
        ptrs = (instances.ctypes.data, out.ctypes.data)
    _check(L, handle, "trgl_instance_depths",
           L.trgl_instance_depths(handle, _dp(mv), _dp(pt), ptrs[0], int(instances.shape[1]), int(instances.shape[0]), _mem(device), ptrs[1]))
    return instances, out


def _depth_order(L, handle, depths, front_to_back, device):
    if device:
        if not hasattr(depths, "data_ptr") or str(depths.dtype) != "torch.float64" or not depths.is_contiguous() or depths.dim() != 1:
            raise ValueError("device=True: depths must be a contiguous float64 device tensor [n]")
        out = _empty(int(depths.shape[0]), np.uint32, True, depths)
        ptrs = (_device_ptr(depths, "depths") if out.numel() else None, out.data_ptr() if out.numel() else None)
    else:
        depths = np.ascontiguousarray(depths, np.float64).reshape(-1)
        out = np.empty(depths.shape[0], np.uint32)
        ptrs = (depths.ctypes.data, out.ctypes.data)
    _check(L, handle, "trgl_depth_order",
           L.trgl_depth_order(handle, ptrs[0], int(depths.shape[0]), ORDER_FRONT_TO_BACK if front_to_back else ORDER_BACK_TO_FRONT, _mem(device), ptrs[1]))
    return depths, out


def instance_depths(model_view, point, instances) -> np.ndarray:
    """trgl_instance_depths for host arrays without a context: the view-space z of `point` (model space) under every instance [n, stride
    >= 16] - element 2 of (model_view * M_i) * (point, 1), summed as the reference's geometry.h sums it.  Needs no GPU."""
    return _instance_depths(load_library(), None, model_view, point, instances, False)[1]


def depth_order(depths, front_to_back=False) -> np.ndarray:
    """trgl_depth_order for a host array without a context: the uint32 permutation that draws the depths farthest first (under a view
    matrix that looks down -z: ascending), or nearest first; ties in ascending number either way.  The order is that of the doubles' bit
    patterns as include/trgl.h defines it (-0.0 before +0.0, NaNs at the ends by their sign).  Needs no GPU."""
    return _depth_order(load_library(), None, depths, front_to_back, False)[1]


def _instance_boxes(L, handle, local, instances, out):
    """Returns (arrays to keep alive, boxes [n, 6]).  Device memory when `instances` is a device tensor."""
    device = _is_device_tensor(instances)
    one = not _is_device_tensor(local) and np.ndim(local) == 1          # one local box for every instance: always host memory
    if device:
        _device_f64(instances, 2, "instance_boxes: instances")
        if not one:
            _device_f64(local, 2, "instance_boxes: local")
    else:
        instances = np.ascontiguousarray(instances, np.float64)
        if instances.ndim != 2:
            raise ValueError("instance_boxes: instances must be [n, stride]")
        if not one:
            local = np.ascontiguousarray(local, np.float64)
    n = int(instances.shape[0])
    if one:
        local, local_stride = _f64(local, 6, "instance_boxes: local"), 0
        lptr = local.ctypes.data
    else:
        if len(local.shape) != 2 or int(local.shape[0]) != n:
            raise ValueError("instance_boxes: local must be [6] (one box for every instance) or [n, stride >= 6]")
        local_stride = int(local.shape[1])
        if local_stride == 0:
            raise ValueError("instance_boxes: a strided local array needs stride >= 6")
        lptr = _device_ptr(local, "local") if device else local.ctypes.data
    if out is None:
        out = _empty((n, 6), np.float64, device, instances)
    else:
        if device:
            _device_f64(out, 2, "instance_boxes: out")
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous):
            raise ValueError("instance_boxes: out must be a contiguous float64 numpy array (the other arrays are in host memory)")
        if tuple(out.shape) != (n, 6):
            raise ValueError("instance_boxes: out must be [n, 6]")
    iptr, optr = (_device_ptr(instances, "instances"), _device_ptr(out, "out")) if device else (instances.ctypes.data, out.ctypes.data)
    if n == 0:
        iptr = optr = None
        lptr = lptr if one else None
    _check(L, handle, "trgl_instance_boxes", L.trgl_instance_boxes(handle, lptr, local_stride, iptr, int(instances.shape[1]), n, _mem(device), optr))
    return (local, instances, out), out


def _frustum_boxes(L, handle, planes, boxes, codes, merge):
    """Returns (arrays to keep alive, codes [n] uint8).  Device memory when `boxes` is a device tensor."""
    planes = _f64(planes, 24, "frustum_boxes: planes")
    device = _is_device_tensor(boxes)
    if device:
        _device_f64(boxes, 2, "frustum_boxes: boxes")
    else:
        boxes = np.ascontiguousarray(boxes, np.float64)
    n = _boxes_count(boxes)
    if codes is None:
        if merge:
            raise ValueError("frustum_boxes: merge=True needs the codes to merge into")
        codes = _empty(n, np.uint8, device, boxes)
    else:
        if device:
            if not _is_device_tensor(codes) or str(codes.dtype) != "torch.uint8" or not codes.is_contiguous():
                raise ValueError("frustum_boxes: codes must be a contiguous uint8 device tensor (the boxes are in device memory)")
        elif not (isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.flags.c_contiguous and codes.flags.writeable):
            raise ValueError("frustum_boxes: codes must be a contiguous writable uint8 numpy array (the boxes are in host memory)")
        if tuple(codes.shape) != (n,):
            raise ValueError("frustum_boxes: codes must be [n]")
    bptr, cptr = (_device_ptr(boxes, "boxes"), _device_ptr(codes, "codes")) if device else (boxes.ctypes.data, codes.ctypes.data)
    if n == 0:
        bptr = cptr = None
    _check(L, handle, "trgl_frustum_boxes", L.trgl_frustum_boxes(handle, _dp(planes), bptr, n, FRUSTUM_MERGE if merge else FRUSTUM_SET, _mem(device), cptr))
    return (boxes, codes), codes


def instance_boxes(local, instances, out=None) -> np.ndarray:
    """trgl_instance_boxes for host arrays without a context: the world box [n, 6] = (min.xyz, max.xyz) of every instance [n, stride >= 16]
    - AABB::transform (geometry.h:297-327) of `local` under the instance's row-major matrix, bit for bit trgl_aabb_transform.  local: [6],
    one box for every instance (mesh_bounds' two halves concatenated), or [n, stride >= 6], one per instance.  Needs no GPU."""
    if _is_device_tensor(instances):
        raise TypeError("instance_boxes: device tensors need a context (Context.instance_boxes)")
    return _instance_boxes(load_library(), None, local, instances, out)[1]


def frustum_boxes(planes, boxes, codes=None, merge=False) -> np.ndarray:
    """trgl_frustum_boxes for host arrays without a context: one code byte per box [n, 6] from Frustum::intersects (our_gl.cpp:264-280)
    against planes [6, 4] (frustum_from_matrix).  merge=False: OCCL_VISIBLE or OCCL_OUTSIDE, into `codes` or a new array.  merge=True:
    `codes` (uint8 [n], occlusion codes for instance) is changed in place - OCCL_OUTSIDE where the frustum culls, untouched elsewhere.
    Needs no GPU."""
    if _is_device_tensor(boxes):
        raise TypeError("frustum_boxes: device tensors need a context (Context.frustum_boxes)")
    return _frustum_boxes(load_library(), None, planes, boxes, codes, merge)[1]


class _InstanceCalls:
    """The instance, box and depth order methods of Context (context.py: L, h, _chk, _hold, _mesh_ptrs and _order_args are its own)."""

    def _instance_args(self, vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device):
        """The mesh and instance arguments of trgl_draw_instanced / trgl_instance_stage as (ctypes arguments, n_faces, n_instances,
        has_colors, arrays to keep alive).  Host arrays are made contiguous; device arrays are checked by _device_ptr."""
        vertices, indices, face_colors, mp = self._mesh_ptrs(vertices, indices, face_colors, device)
        nv, stride = vertices.shape
        nf = indices.shape[0]
        if instances is None:
            inst_stride = 0
            n_inst = None
        else:
            if not instances_device:
                instances = np.ascontiguousarray(instances, np.float64)
                if instances.ndim != 2:
                    instances = instances.reshape(instances.shape[0], -1)
            n_inst, inst_stride = int(instances.shape[0]), int(instances.shape[1])
        for a, what in ((instance_colors, "instance_colors"), (visible, "visible")):
            if a is not None:
                if n_inst is None:
                    n_inst = int(a.shape[0])
                elif int(a.shape[0]) != n_inst:
                    raise ValueError(f"{what}: one entry per instance expected")
        if n_inst is None:
            raise ValueError("the number of instances comes from instances, instance_colors or visible: all three are None")
        if instances_device:
            ip = (_device_ptr(instances, "instances"), _device_ptr(instance_colors, "instance_colors"), _device_ptr(visible, "visible"))
        else:
            if instance_colors is not None:
                instance_colors = np.ascontiguousarray(instance_colors, np.uint32)
            if visible is not None:
                visible = np.ascontiguousarray(visible, np.uint8)
            ip = (_ptr(instances), _ptr(instance_colors), _ptr(visible))
        args = [mp[0], stride, nv, mp[1], nf, mp[2], _mem(device),
                ip[0], inst_stride, n_inst, ip[1], ip[2], _mem(instances_device)]
        return args, nf, n_inst, face_colors is not None or instance_colors is not None, (vertices, indices, face_colors, instances, instance_colors, visible)

    def instance_depths(self, model_view, point, instances, device=False):
        """trgl_instance_depths: the view-space z of `point` (a point of the mesh in model space) under every instance [n, stride >= 16].
        Host arrays: a numpy array, no GPU work.  device=True: instances is a contiguous float64 device tensor; the depths come back
        as a device tensor, queued on the context's stream without waiting."""
        instances, out = _instance_depths(self.L, self.h, model_view, point, instances, device)
        self._hold(device, (instances, out))
        return out

    def depth_order(self, depths, front_to_back=False, device=False):
        """trgl_depth_order: the order in which to draw instances of these depths - farthest first, or with front_to_back nearest first;
        ties ascend either way.  Host array: a uint32 numpy array.  device=True: depths is a contiguous float64 device tensor; the
        order comes back as an int32 device tensor (its bits are the uint32 numbers), sorted on the context's stream without waiting.
        Pass it to draw_instanced / instance_stage as order=..., order_device=True."""
        depths, out = _depth_order(self.L, self.h, depths, front_to_back, device)
        self._hold(device, (depths, out))
        return out

    def instance_boxes(self, local, instances, out=None):
        """trgl_instance_boxes: the world box [n, 6] = (min.xyz, max.xyz) of every instance [n, stride >= 16], AABB::transform of `local`
        under the instance's matrix.  local: [6] in host memory (one box for every instance: mesh_bounds' halves concatenated) or
        [n, stride >= 6] where the instances are.  numpy instances: a numpy array, no GPU work.  A contiguous float64 device tensor: the
        boxes come back as a device tensor (`out` when given), queued on the context's stream without waiting - the input of
        occlusion_boxes(device=True) and frustum_boxes."""
        keep, out = _instance_boxes(self.L, self.h, local, instances, out)
        self._hold(_is_device_tensor(out), keep)
        return out

    def frustum_boxes(self, planes, boxes, codes=None, merge=False):
        """trgl_frustum_boxes: one code byte per box [n, 6] from Frustum::intersects against planes [6, 4] (host memory).  merge=False
        writes OCCL_VISIBLE / OCCL_OUTSIDE into `codes` (allocated when None); merge=True writes OCCL_OUTSIDE into the given codes where
        the frustum culls and leaves every other byte as it is - over the codes of occlusion_boxes that makes the `visible` array of
        draw_instanced.  numpy boxes: no GPU work.  Device tensors (boxes float64, codes uint8 at any address): queued on the context's
        stream without waiting."""
        keep, codes = _frustum_boxes(self.L, self.h, planes, boxes, codes, merge)
        self._hold(_is_device_tensor(codes), keep)
        return codes

    def draw_instanced(self, kind, uniforms, projection, vertices, indices, instances=None, vertex_shader=None, face_colors=None,
                       instance_colors=None, visible=None, device=False, instances_device=False, order=None, order_device=False):
        """trgl_draw_instanced: the mesh (vertices [nv, stride], indices [nf, 3]) once per instance whose `visible` byte has bit 0 set
        (visible None: every instance), in ascending instance order.  instances [n, stride]: with the built-in stage (vertex_shader None)
        the first 16 doubles are a row-major model matrix M and the stage runs under uniforms.model_view * M; a user vertex shader
        reads them as in.inst.  Colours: instance_colors [n] or face_colors [nf], not both.  device: the mesh arrays are device
        tensors; instances_device: instances, instance_colors and visible are (the codes of occlusion_boxes(device=True) are a valid
        `visible`; the call then waits once for the count of drawn instances).  order (trgl_draw_instanced_ordered): the instances
        are visited in the order this list of numbers names them - the result of depth_order, or any list; an instance named twice
        is drawn twice, one that is not named is not drawn, an empty list draws nothing; order_device: the list is a device tensor (entries out of range are
        skipped, and the call waits once for the count)."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        args, _, _, _, keep = self._instance_args(vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device)
        vs = -1 if vertex_shader is None else int(vertex_shader)
        if order is None:
            self._hold(device or instances_device, keep)
            self._chk(self.L.trgl_draw_instanced(self.h, vs, kind, _ref(uniforms), _dp(pj), *args))
            return
        oargs, n_order, okeep = self._order_args(order, order_device)
        if n_order == 0:                     # no position to visit: nothing is drawn (the C call takes a null list for "no list")
            return
        self._hold(device or instances_device or order_device, keep + (okeep,))
        self._chk(self.L.trgl_draw_instanced_ordered(self.h, vs, kind, _ref(uniforms), _dp(pj), *args, *oargs))

    def instance_stage(self, vertex_shader, uniforms, projection, vertices, indices, instances=None, face_colors=None, instance_colors=None,
                       visible=None, device=False, instances_device=False, out=None, order=None, order_device=False):
        """trgl_instance_stage: the stages of draw_instanced alone; returns (clip, varyings, colors, n_out) with n_out = drawn instances
        * nf rows written.  vertex_shader: a number from register_vertex_shader, or -1 / None for the built-in stage (K = 24).
        Host instances: numpy arrays cut to n_out rows (varyings [n_out, K]; colors None when the call has none).  instances_device=True:
        out = (clip, varyings, colors) are 16-byte aligned device tensors with room for n * nf rows (varyings may be None when K = 0,
        colors when the call has none); they come back as they are.  order / order_device: as for draw_instanced
        (trgl_instance_stage_ordered); the outputs then need room for len(order) * nf rows."""
        vs = -1 if vertex_shader is None else int(vertex_shader)
        K = VARY[PHONG] if vs < 0 else getattr(self, "_vertex_vary", {}).get(vs, 0)
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        args, nf, n_inst, has_colors, keep = self._instance_args(vertices, indices, instances, face_colors, instance_colors, visible, device, instances_device)
        n_out = C.c_uint64(0)
        oargs, n_order, okeep = (None, n_inst, None) if order is None else self._order_args(order, order_device)
        self._hold(order_device, (okeep,))
        if instances_device:
            clip, vary, col = out
            optrs = (_device_ptr(clip, "clip"), _device_ptr(vary, "varyings"), _device_ptr(col, "colors"))
            self._hold(True, keep + (clip, vary, col))
        else:
            assert out is None, "out: only with instances_device=True"
            rows = n_order * nf
            clip, vary = np.zeros((rows, 12), np.float64), np.zeros((rows, K), np.float64)
            col = np.zeros(rows, np.uint32) if has_colors else None
            optrs = (clip.ctypes.data, vary.ctypes.data if K else None, col.ctypes.data if has_colors else None)
            self._hold(device, keep)
        if order is not None and n_order == 0:
            pass                             # no position to visit: no rows (the C call takes a null list for "no list")
        elif order is None:
            self._chk(self.L.trgl_instance_stage(self.h, vs, _ref(uniforms), _dp(pj), *args, optrs[0], optrs[1], optrs[2], C.byref(n_out)))
        else:
            self._chk(self.L.trgl_instance_stage_ordered(self.h, vs, _ref(uniforms), _dp(pj), *args, *oargs, optrs[0], optrs[1], optrs[2], C.byref(n_out)))
        n = int(n_out.value)
        if instances_device:
            return clip, vary, col, n
        return clip[:n], vary[:n], None if col is None else col[:n], n
