"""trgl_mesh_normals / trgl_mesh_tangents in host memory, their Python wrappers and tests/mesh_attr_model.py, bit for bit against
tests/golden/mesh_attr_golden.json: results of the reference's own compiled Model::generateNormalsIfNeeded and
Model::computeTangentsIfNeeded (tests/golden/make_mesh_attr_golden.py).  No GPU is touched: the host entry points take a NULL context."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mesh_attr_model
from tinyrenderder_amd import api
from tinyrenderder_amd.api import Context

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_attr_golden.json")))
IDS = ["%s-%s" % (g["kind"], g["name"]) for g in GOLDEN]
FN = {"normals": api.mesh_normals, "tangents": api.mesh_tangents}
MODEL = {"normals": mesh_attr_model.generate_normals, "tangents": mesh_attr_model.compute_tangents}


load = mesh_attr_model.load_case


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_golden_file_holds_the_cases_the_tests_rely_on():
    names = {(g["kind"], g["name"]) for g in GOLDEN}
    assert {("normals", "fan_5000"), ("tangents", "fan_5000"), ("tangents", "r_at_the_threshold"), ("normals", "not_needed_nan_normal")} <= names
    assert {g["generated"] for g in GOLDEN} == {0, 1}
    assert {g["stride"] for g in GOLDEN if g["kind"] == "normals"} >= {6, 9} and {g["stride"] for g in GOLDEN if g["kind"] == "tangents"} >= {14, 17}


@pytest.mark.parametrize("g", GOLDEN, ids=IDS)
def test_host_entry_point_equals_the_reference(g):
    v, i, want = load(g)
    keep = v.copy()
    got, generated = FN[g["kind"]](v, i)
    assert generated == bool(g["generated"])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(v), bits(keep)), "the wrapper works on a copy"
    if not generated:
        assert np.array_equal(bits(got), bits(keep))
    cols = list(range(3, 6)) if g["kind"] == "normals" else list(range(8, 14))      # everything else keeps its bits
    rest = [c for c in range(g["stride"]) if c not in cols]
    assert np.array_equal(bits(got[:, rest]), bits(keep[:, rest]))


@pytest.mark.parametrize("g", GOLDEN, ids=IDS)
def test_python_model_equals_the_reference(g):
    v, i, want = load(g)
    got, generated = MODEL[g["kind"]](v, i)
    assert generated == bool(g["generated"]) and np.array_equal(bits(got), bits(want))


def test_order_of_the_faces_shows_in_the_fans():
    """What the ordering tests rest on: the same faces in reverse order give other bits at the fan's centre."""
    for g in GOLDEN:
        if g["name"].startswith("fan_"):
            v, i, want = load(g)
            got, _ = FN[g["kind"]](v, i[::-1].copy())
            assert not np.array_equal(bits(got[0]), bits(want[0])), (g["kind"], g["name"])


def raw(name, v, stride, nv, i, nf, mem=api.MEM_HOST, generated=None):
    L = api.load_library()
    return getattr(L, name)(None, None if v is None else v.ctypes.data, stride, nv, None if i is None else i.ctypes.data, nf, mem, generated)


@pytest.mark.parametrize("name,min_stride", [("trgl_mesh_normals", 6), ("trgl_mesh_tangents", 14)])
def test_invalid_arguments_are_refused_and_nothing_is_written(name, min_stride):
    v = np.zeros((4, 17)); i = np.array([[0, 1, 2], [1, 2, 3]], np.uint32)
    keep = v.copy()
    gen = C.c_int(7)
    assert raw(name, v, min_stride - 1, 4, i, 2) == -1                                  # too small a stride
    assert raw(name, None, 17, 4, i, 2) == -1                                           # null vertices
    assert raw(name, v, 17, 4, None, 2) == -1                                           # null indices with faces
    assert raw(name, v, 17, 4, i, 2, mem=5) == -1                                       # bad mem_kind
    assert raw(name, v, 17, 4, i, 2, mem=api.MEM_DEVICE) == -1                          # device memory needs a context
    assert raw(name, v, 17, 4, i, (1 << 32) // 3 + 1) == -1                             # 3 * n_faces does not fit in 32 bits
    bad = np.array([[0, 1, 2], [1, 4, 3]], np.uint32)
    assert raw(name, v, 17, 4, bad, 2, generated=C.byref(gen)) == -1 and gen.value in (0, 7)   # a host index >= n_vertices
    assert np.array_equal(bits(v), bits(keep))
    assert api.load_library().trgl_last_error(None).decode().startswith(name)
    # what is allowed: no vertices at all, no faces with null indices, no `generated`
    assert raw(name, None, 17, 0, None, 0, generated=C.byref(gen)) == 0 and gen.value == 0
    assert raw(name, v, 17, 0, bad, 2) == 0 and np.array_equal(bits(v), bits(keep))
    assert raw(name, v, 17, 4, None, 0) == 0
    assert not np.array_equal(bits(v), bits(keep))                                      # every vertex took the fallback


def test_null_context_and_null_generated_work_for_host_memory():
    g = next(x for x in GOLDEN if x["kind"] == "normals" and x["name"] == "fan_300")
    v, i, want = load(g)
    assert raw("trgl_mesh_normals", v, g["stride"], v.shape[0], i, i.shape[0]) == 0
    assert np.array_equal(bits(v), bits(want))
    gen = C.c_int(-1)
    assert raw("trgl_mesh_normals", v, g["stride"], v.shape[0], i, i.shape[0], generated=C.byref(gen)) == 0 and gen.value == 0
    assert np.array_equal(bits(v), bits(want)), "a second call finds nothing to do"


def test_host_arrays_are_refused_with_device_true():
    """Context.mesh_normals / mesh_tangents(device=True) take their addresses from Context._mesh_ptrs, which hands every array to
    _device_ptr: a numpy array raises there, before anything reaches the library.  _mesh_ptrs reads nothing of the context, so it is
    called unbound here; tests/test_mesh_attr_gpu.py makes the same calls on a live context."""
    v = np.zeros((3, 14)); i = np.array([[0, 1, 2]], np.uint32)
    with pytest.raises(TypeError, match="device=True: vertices"):
        Context._mesh_ptrs(None, v, i, None, True)
    with pytest.raises(TypeError, match="device=True: indices"):
        Context._mesh_ptrs(None, 4096, i, None, True)


def test_wrappers_refuse_wrong_shapes():
    with pytest.raises(ValueError):
        api.mesh_normals(np.zeros(12), np.array([[0, 1, 2]], np.uint32))
    with pytest.raises(api.TrglError, match="stride"):
        api.mesh_tangents(np.zeros((3, 13)), np.array([[0, 1, 2]], np.uint32))
