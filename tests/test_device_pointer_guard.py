"""api._device_ptr: what Context.draw(device=True) and Context.draw_indexed(device=True) accept as an array.  With TRGL_MEM_DEVICE
the library hands the caller's pointers to its kernels as they are (include/trgl.h), so a host address must be stopped in the
binding, before the library is called: on a GPU it would be a memory fault, not an error code.  No GPU is needed here, and no GPU
test relies on this guard."""
import numpy as np
import pytest
import torch

from tinyrenderder_amd import api


class _FakeCuda:
    """What the guard looks at in a torch CUDA tensor."""
    is_cuda = True
    shape = (2, 12)

    def data_ptr(self):
        return 0x7F0000001000


def test_device_ptr_accepts_ints_device_tensors_and_none():
    assert api._device_ptr(None) is None
    assert api._device_ptr(0x7F0000000008) == 0x7F0000000008
    assert api._device_ptr(_FakeCuda()) == 0x7F0000001000


@pytest.mark.parametrize("bad", [np.zeros((2, 12)), np.zeros(2, np.uint32), torch.zeros(2, 12, dtype=torch.float64),
                                 torch.zeros(2, dtype=torch.int32), [0.0] * 12, 1.5, True, np.zeros((2, 12)).ctypes],
                         ids=["numpy_f64", "numpy_u32", "cpu_tensor_f64", "cpu_tensor_i32", "list", "float", "bool", "ctypes"])
def test_device_ptr_refuses_host_arrays(bad):
    with pytest.raises(TypeError, match="device=True"):
        api._device_ptr(bad, "clip")


class _Recorder:
    """Stands in for the loaded library: any call is recorded (and would 'succeed')."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


def _context(lib):
    ctx = object.__new__(api.Context)
    ctx.L, ctx.h, ctx._keep, ctx._user_vary = lib, None, [], {api.SHADER_USER_FIRST: 5}
    return ctx


@pytest.mark.parametrize("which", ["clip", "varyings", "colors"])
@pytest.mark.parametrize("kind", [api.FLAT, api.GOURAUD, api.PHONG, api.SHADER_USER_FIRST])
def test_draw_refuses_a_host_array_before_the_library_is_called(kind, which):
    """Each argument on its own, the others being device tensors - also varyings handed to a kind that takes none (K = 0)."""
    lib = _Recorder()
    ctx = _context(lib)
    args = dict(clip=_FakeCuda(), varyings=_FakeCuda(), colors=_FakeCuda())
    for bad in (np.zeros((2, 24)), torch.zeros(2, 24, dtype=torch.float64)):
        with pytest.raises(TypeError, match=which):
            ctx.draw(kind, uniforms=api.make_uniforms(), device=True, n=2, **dict(args, **{which: bad}))
    assert lib.calls == [] and ctx._keep == []
    ctx.draw(kind, uniforms=api.make_uniforms(), device=True, **args)          # ... and the guard lets device arrays through
    assert lib.calls == ["trgl_draw"] and len(ctx._keep) == 1


@pytest.mark.parametrize("which", ["vertices", "indices"])
def test_draw_indexed_refuses_a_host_array_before_the_library_is_called(which):
    lib = _Recorder()
    ctx = _context(lib)
    args = dict(vertices=_FakeCuda(), indices=_FakeCuda())
    for bad in (np.zeros((2, 12)), torch.zeros(2, 12, dtype=torch.float64)):
        with pytest.raises(TypeError, match=which):
            ctx.draw_indexed(api.PHONG, api.make_uniforms(), np.eye(4), device=True, **dict(args, **{which: bad}))
    assert lib.calls == [] and ctx._keep == []
    ctx.draw_indexed(api.PHONG, api.make_uniforms(), np.eye(4), device=True, **args)
    assert lib.calls == ["trgl_draw_indexed"]


def test_host_draws_still_take_numpy_arrays():
    lib = _Recorder()
    ctx = _context(lib)
    ctx.draw(api.GOURAUD, np.zeros((2, 12)), np.zeros((2, 3)), np.zeros(2, np.uint32))
    assert lib.calls == ["trgl_draw"] and ctx._keep == []
