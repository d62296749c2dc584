"""Mesh attributes and bounds: the model's box, its smooth normals and tangent frames, and the box and frustum tests of a scene."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .loader import load_library
from .marshal import _check, _device_ptr, _dp, _f64, _failure, _mem


def _mesh_bounds(L, handle, vertices, device):
    lo, hi = np.empty(3, np.float64), np.empty(3, np.float64)
    if device:
        ptr = _device_ptr(vertices, "vertices")
    else:
        vertices = np.ascontiguousarray(vertices, np.float64)
        ptr = vertices.ctypes.data
    if len(vertices.shape) != 2:
        raise ValueError("mesh_bounds: vertices must be [n, stride]")
    nv, stride = vertices.shape
    _check(L, handle, "trgl_mesh_bounds", L.trgl_mesh_bounds(handle, ptr, int(stride), int(nv), _mem(device), _dp(lo), _dp(hi)))
    return lo, hi


def mesh_bounds(vertices):
    """trgl_mesh_bounds for a host array without a context: Model::computeAABB (model.cpp:15-40) of vertices [n, stride >= 3] with the
    position at +0; returns (min[3], max[3]) with the reference's 1 % margin.  Needs no GPU."""
    return _mesh_bounds(load_library(), None, vertices, False)


def _mesh_attr(L, handle, name, ptrs, vertices, indices, device, wait):
    if len(vertices.shape) != 2 or len(indices.shape) != 2 or indices.shape[1] != 3:
        raise ValueError(f"{name}: vertices must be [n, stride] and indices [n_faces, 3]")
    nv, stride = vertices.shape
    generated = C.c_int(0)
    entry = getattr(L, "trgl_" + name)
    _check(L, handle, "trgl_" + name,
           entry(handle, ptrs[0], int(stride), int(nv), ptrs[1], int(indices.shape[0]), _mem(device), C.byref(generated) if wait else None))
    return bool(generated.value) if wait else None


def _host_mesh(vertices, indices):
    """A private, writable, contiguous copy of the vertices, and the indices as [n_faces, 3] uint32."""
    return np.array(vertices, np.float64, order="C"), np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)


def mesh_normals(vertices, indices):
    """trgl_mesh_normals for host arrays without a context: Model::generateNormalsIfNeeded (model.cpp:269-316) on a copy of vertices
    [n, stride >= 6] (normal at +3) with indices [n_faces, 3]; returns (vertices, generated).  Needs no GPU."""
    v, i = _host_mesh(vertices, indices)
    return v, _mesh_attr(load_library(), None, "mesh_normals", (v.ctypes.data, i.ctypes.data), v, i, False, True)


def mesh_tangents(vertices, indices):
    """trgl_mesh_tangents likewise: Model::computeTangentsIfNeeded (model.cpp:318-388) on a copy of vertices [n, stride >= 14]
    (texcoord +6, tangent +8, bitangent +11); returns (vertices, generated).  Needs no GPU."""
    v, i = _host_mesh(vertices, indices)
    return v, _mesh_attr(load_library(), None, "mesh_tangents", (v.ctypes.data, i.ctypes.data), v, i, False, True)


def aabb_transform(bmin, bmax, m):
    """trgl_aabb_transform: AABB::transform (geometry.h:297-327) of the box by the row-major 4x4 m; returns (min[3], max[3])."""
    lo, hi = np.empty(3, np.float64), np.empty(3, np.float64)
    rc = load_library().trgl_aabb_transform(_dp(_f64(bmin, 3, "bmin")), _dp(_f64(bmax, 3, "bmax")), _dp(_f64(m, 16, "m")), _dp(lo), _dp(hi))
    if rc != 0:
        raise _failure("trgl_aabb_transform", rc)
    return lo, hi


def frustum_from_matrix(m):
    """trgl_frustum_from_matrix: Frustum::createFromMatrix (our_gl.cpp:212-262); returns planes [6, 4] = nx, ny, nz, d in the order
    FRUSTUM_LEFT .. FRUSTUM_FAR."""
    planes = np.empty((6, 4), np.float64)
    rc = load_library().trgl_frustum_from_matrix(_dp(_f64(m, 16, "m")), _dp(planes))
    if rc != 0:
        raise _failure("trgl_frustum_from_matrix", rc)
    return planes


def frustum_intersects(planes, bmin, bmax) -> bool:
    """trgl_frustum_intersects: Frustum::intersects (our_gl.cpp:264-280)."""
    rc = load_library().trgl_frustum_intersects(_dp(_f64(planes, 24, "planes")), _dp(_f64(bmin, 3, "bmin")), _dp(_f64(bmax, 3, "bmax")))
    if rc < 0:
        raise _failure("trgl_frustum_intersects", rc)
    return rc == 1


class _MeshCalls:
    """The mesh attribute and bounds methods of Context (context.py: L, h, _hold and _mesh_ptrs are its own)."""

    def mesh_bounds(self, vertices, device=False):
        """trgl_mesh_bounds: Model::computeAABB (model.cpp:15-40) of vertices [n, stride >= 3]; returns (min[3], max[3]).  device=True:
        a device tensor, reduced on the context's stream in order with the draws (nothing is flushed); the call waits for the result."""
        return _mesh_bounds(self.L, self.h, vertices, device)

    def _mesh_attr(self, name, vertices, indices, device, wait):
        if not device:
            vertices, indices = _host_mesh(vertices, indices)
        vertices, indices, _, ptrs = self._mesh_ptrs(vertices, indices, None, device)
        self._hold(device and not wait, (vertices, indices))
        return vertices, _mesh_attr(self.L, self.h, name, ptrs, vertices, indices, device, wait or not device)

    def mesh_normals(self, vertices, indices, device=False, wait=True):
        """trgl_mesh_normals: Model::generateNormalsIfNeeded (model.cpp:269-316); returns (vertices, generated).  Host arrays: computed
        on a copy.  device=True: device tensors [n, stride >= 6] f64 and [n_faces, 3] u32, rewritten in place on the context's stream in
        order with the draws (nothing is flushed); wait=False queues without waiting and returns generated = None."""
        return self._mesh_attr("mesh_normals", vertices, indices, device, wait)

    def mesh_tangents(self, vertices, indices, device=False, wait=True):
        """trgl_mesh_tangents: Model::computeTangentsIfNeeded (model.cpp:318-388) likewise, vertices [n, stride >= 14]."""
        return self._mesh_attr("mesh_tangents", vertices, indices, device, wait)
