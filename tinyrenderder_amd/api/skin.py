"""Skin: joint palettes composed along a skeleton, and linear blend skinning of a mesh under them."""
import ctypes as C

import numpy as np

from .loader import load_library
from .marshal import _check, _device_f64, _dp, _empty, _is_device_tensor, _mem, _ptr_of, _ref


class SkinParams(C.Structure):
    """trgl_skin_params"""
    _fields_ = [("vertex_stride", C.c_int32), ("n_influences", C.c_int32), ("n_joints", C.c_uint32), ("flags", C.c_uint32),
                ("n_poses", C.c_uint64), ("palette_stride", C.c_uint64), ("reserved", C.c_uint64)]


def _skin_inputs(vertices, joints, weights, palette, device):
    """(vertices [n, stride], joints [n, k] uint16, weights [n, k], palette [n_poses, n_joints, 16] or [n_joints, 16]) as the skinning
    calls take them, checked: device tensors with device=True, else numpy arrays."""
    if device:
        _device_f64(vertices, 2, "vertices"); _device_f64(weights, 2, "weights")
        if not _is_device_tensor(palette) or str(palette.dtype) != "torch.float64" or palette.dim() not in (2, 3) or palette.stride(-1) != 1 or \
                palette.stride(-2) != 16 or int(palette.shape[-1]) != 16:
            raise ValueError("device=True: palette must be a float64 device tensor [n_poses, n_joints, 16] or [n_joints, 16] with packed matrices")
        if not _is_device_tensor(joints) or joints.element_size() != 2 or not joints.is_contiguous() or joints.dim() != 2:
            raise ValueError("device=True: joints must be a contiguous 16-bit device tensor [n, n_influences]")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        joints = np.ascontiguousarray(joints, np.uint16)
        weights = np.ascontiguousarray(weights, np.float64)
        palette = np.asarray(palette, np.float64)
        # (poses may lie further apart than a palette is long - palette_stride -, the matrices of one pose are packed)
        if palette.ndim != 3 or palette.strides[1:] != (128, 8) or palette.strides[0] % 8 or palette.strides[0] < 128 * palette.shape[1]:
            palette = np.ascontiguousarray(palette)
        if vertices.ndim != 2 or joints.ndim != 2 or weights.ndim != 2 or palette.ndim not in (2, 3) or palette.shape[-1] != 16:
            raise ValueError("vertices [n, stride], joints and weights [n, n_influences], palette [n_poses, n_joints, 16] or [n_joints, 16]")
    if tuple(joints.shape) != tuple(weights.shape) or int(joints.shape[0]) != int(vertices.shape[0]):
        raise ValueError("joints and weights: one row of n_influences per vertex")
    return vertices, joints, weights, palette


def _skin_params(vertices, joints, palette, flags):
    """trgl_skin_params of checked arrays; a 3-dimensional palette's first stride is the palette_stride."""
    poses = int(palette.shape[0]) if len(palette.shape) == 3 else 1
    if len(palette.shape) == 3 and poses > 1:
        pstride = int(palette.stride(0)) if hasattr(palette, "data_ptr") else int(palette.strides[0]) // 8
    else:
        pstride = 0
    return SkinParams(int(vertices.shape[1]), int(joints.shape[1]), int(palette.shape[-2]), int(flags), poses, pstride, 0)


def _skin_stage(L, handle, vertices, joints, weights, palette, flags, device, out):
    """Returns (arrays to keep alive, out [n_poses, n, stride])."""
    vertices, joints, weights, palette = _skin_inputs(vertices, joints, weights, palette, device)
    P = _skin_params(vertices, joints, palette, flags)
    n, stride = int(vertices.shape[0]), int(vertices.shape[1])
    if out is None:
        out = _empty((int(P.n_poses), n, stride), np.float64, device, vertices)
    p = _ptr_of(device)
    _check(L, handle, "trgl_skin_stage", L.trgl_skin_stage(handle, C.byref(P), p(vertices), n, p(joints), p(weights), p(palette), _mem(device), p(out)))
    return (vertices, joints, weights, palette), out


def _pose_palette(L, handle, parents, local, inverse_bind, device, out):
    """Returns (arrays to keep alive, palette [n_poses, n_joints, 16]); local: [n_poses, n_joints, 16]."""
    if device:
        _device_f64(local, 3, "local")
        if inverse_bind is not None:
            _device_f64(inverse_bind, 2, "inverse_bind")
        if not _is_device_tensor(parents) or parents.element_size() != 4 or not parents.is_contiguous():
            raise ValueError("device=True: parents must be a contiguous 32-bit device tensor")
    else:
        local = np.ascontiguousarray(local, np.float64)
        parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
        inverse_bind = None if inverse_bind is None else np.ascontiguousarray(inverse_bind, np.float64)
        if local.ndim != 3:
            raise ValueError("local must be [n_poses, n_joints, 16]")
    poses, nj = int(local.shape[0]), int(local.shape[1])
    if int(local.shape[2]) != 16 or int(parents.shape[0]) != nj or (inverse_bind is not None and tuple(inverse_bind.shape) != (nj, 16)):
        raise ValueError("local [n_poses, n_joints, 16], parents [n_joints], inverse_bind [n_joints, 16] or None")
    if out is None:
        out = _empty((poses, nj, 16), np.float64, device, local)
    if device:
        pstride = int(out.stride(0)) if poses > 1 else 16 * nj
    else:
        pstride = int(out.strides[0]) // 8 if poses > 1 else 16 * nj
    p = _ptr_of(device)
    _check(L, handle, "trgl_pose_palette",
           L.trgl_pose_palette(handle, p(parents), p(inverse_bind), nj, p(local), 16 * nj, poses, _mem(device), p(out), pstride))
    return (parents, local, inverse_bind), out


def skin_stage(vertices, joints, weights, palette, flags=0):
    """trgl_skin_stage for host arrays without a context: linear blend skinning of vertices [n, stride >= 3] (the reference's Vertex
    layout) by joints [n, k] (uint16) and weights [n, k], k = 1 .. 8, under palette [n_poses, n_joints, 16] (or [n_joints, 16]: one pose)
    of row-major matrices; flags: SKIN_NORMAL | SKIN_TANGENT | SKIN_BITANGENT.  Returns [n_poses, n, stride].  Needs no GPU."""
    return _skin_stage(load_library(), None, vertices, joints, weights, palette, flags, False, None)[1]


def pose_palette(parents, local, inverse_bind=None):
    """trgl_pose_palette for host arrays without a context: local [n_poses, n_joints, 16] joint matrices composed along parents
    [n_joints] (-1: a root; else a joint below) and multiplied by inverse_bind [n_joints, 16] when given.  Returns the palettes
    [n_poses, n_joints, 16].  Needs no GPU."""
    return _pose_palette(load_library(), None, parents, local, inverse_bind, False, None)[1]


class _SkinCalls:
    """The skinning methods of Context (context.py: L, h, _chk, _hold and _mesh_ptrs are its own)."""

    def skin_stage(self, vertices, joints, weights, palette, flags=0, device=False, out=None):
        """trgl_skin_stage (see the module's skin_stage).  Host arrays: numpy, no GPU work.  device=True: vertices [n, stride] f64,
        joints [n, k] (16-bit), weights [n, k] f64 and palette [n_poses, n_joints, 16] f64 are device tensors, out [n_poses, n, stride]
        a device tensor (allocated with torch when not given); the stage is queued on the context's stream without waiting.  Returns
        out: out[q] is what draw_indexed, mesh_bounds, mesh_normals and mesh_tangents take with device=True."""
        keep, out = _skin_stage(self.L, self.h, vertices, joints, weights, palette, flags, device, out)
        self._hold(device, (keep, out))
        return out

    def pose_palette(self, parents, local, inverse_bind=None, device=False, out=None):
        """trgl_pose_palette (see the module's pose_palette).  device=True: parents [n_joints] (32-bit), local [n_poses, n_joints, 16] f64
        and inverse_bind [n_joints, 16] f64 or None are device tensors; queued on the context's stream without waiting.  Returns the
        palettes [n_poses, n_joints, 16] - what skin_stage takes."""
        keep, out = _pose_palette(self.L, self.h, parents, local, inverse_bind, device, out)
        self._hold(device, (keep, out))
        return out

    def draw_skinned(self, kind, uniforms, projection, vertices, joints, weights, palette, indices, flags=0, device=False,
                     vertex_shader=None, colors=None):
        """trgl_draw_skinned: skin_stage with one pose into a buffer of the context's, then draw_indexed of it (vertex_shader= and
        colors= as there).  device=True: every array is a device tensor; no wait."""
        pj = np.ascontiguousarray(projection, np.float64).reshape(16)
        vertices, joints, weights, palette = _skin_inputs(vertices, joints, weights, palette, device)
        P = _skin_params(vertices, joints, palette, flags)
        _, indices, colors, ptrs = self._mesh_ptrs(vertices, indices, colors, device)
        p = _ptr_of(device)
        self._hold(device, (vertices, joints, weights, palette, indices, colors))
        self._chk(self.L.trgl_draw_skinned(self.h, -1 if vertex_shader is None else int(vertex_shader), kind, _ref(uniforms), _dp(pj), C.byref(P),
                                           p(vertices), int(vertices.shape[0]), p(joints), p(weights), p(palette), ptrs[1], int(indices.shape[0]), ptrs[2],
                                           _mem(device)))
