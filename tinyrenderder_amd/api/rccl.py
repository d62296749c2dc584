"""RCCL: the communicator of a render split over several contexts, and the gather that joins their rows."""
from __future__ import annotations

import ctypes as C

from .loader import load_library
from .marshal import _check


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI: 128 bytes that rank 0 hands to the other ranks."""
    L = load_library()
    buf = (C.c_uint8 * 128)()
    _check(L, None, "trgl_rccl_unique_id", L.trgl_rccl_unique_id(buf))
    return bytes(buf)


def rccl_comm_create(unique_id: bytes, rank: int, world: int, device: int = 0):
    """ncclCommInitRank through the C ABI; returns the communicator handle for Context.gather()."""
    L = load_library()
    comm = C.c_void_p()
    buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
    _check(L, None, "trgl_rccl_comm_create", L.trgl_rccl_comm_create(buf, rank, world, device, C.byref(comm)))
    return comm


def rccl_comm_destroy(comm):
    load_library().trgl_rccl_comm_destroy(comm)


class _RcclCalls:
    """The gather of Context (context.py: L, h and _chk are its own)."""

    def gather(self, comm, rank, world, with_z=False):
        """trgl_gather: join the rows of the `world` contexts of a render into this context's framebuffer (and z-buffer) with
        in-place RCCL all-gathers queued on the context's stream; `comm` is an ncclComm_t (rccl_comm_create)."""
        self._chk(self.L.trgl_gather(self.h, comm, rank, world, int(bool(with_z))))
