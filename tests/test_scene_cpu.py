"""The host-only scene entry points - trgl_aabb_transform, trgl_frustum_from_matrix, trgl_frustum_intersects and the host path of
trgl_mesh_bounds - and their Python wrappers, bit for bit against tests/golden/scene_golden.json: results of the reference's own
compiled Frustum::createFromMatrix / intersects (our_gl.cpp:212-280), AABB::transform (geometry.h:297-327), Camera (camera.h) and
Model::computeAABB (model.cpp:15-40), made by tests/golden/make_scene_golden.py.  tests/scene_model.py, the Python restatement the
GPU tests compare against, is held to the same goldens.

Model::computeAABB is private in the reference (model.h:130); the golden driver reaches the compiled member through model.h with
access control lifted (tests/host/scene_ref_driver.cpp), so it is pinned like the rest.  No GPU is needed for anything here."""
import json
import math
import os

import numpy as np
import pytest

import scene_model
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "scene_golden.json")) as _f:
    GOLDEN = json.load(_f)


def unhex(xs):
    return np.array([float.fromhex(x) for x in xs], np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


IMPLS = {"library": api, "model": scene_model}


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_frustum_planes_equal_the_reference(impl):
    assert len(GOLDEN["frustum"]) >= 30
    for i, c in enumerate(GOLDEN["frustum"]):
        got = IMPLS[impl].frustum_from_matrix(unhex(c["m"]))
        assert same_bits(got, unhex(c["planes"])), (i, got)


def test_main_cpp_camera_frustum():
    """Perspective * ModelView of main.cpp:585-594,610-623 is the first frustum case, and its planes cull what main.cpp would."""
    cam = {k: unhex(v).reshape(4, 4) for k, v in GOLDEN["camera"].items()}
    assert same_bits(cam["view_projection"], unhex(GOLDEN["frustum"][0]["m"]))
    vp = np.zeros((4, 4))
    for i in range(4):                                     # geometry.h:195-205
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc += cam["projection"][i, k] * cam["view"][k, j]
            vp[i, j] = acc
    assert same_bits(vp, cam["view_projection"])
    planes = api.frustum_from_matrix(vp)
    head_box = api.aabb_transform([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], cam["head_model"])
    assert api.frustum_intersects(planes, *head_box)                       # the head sits in front of main.cpp's camera
    assert not api.frustum_intersects(planes, [-60.0, 0.0, 0.0], [-50.0, 1.0, 1.0])   # far behind it


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_frustum_intersects_equals_the_reference(impl):
    assert {c["result"] for c in GOLDEN["intersect"]} == {0, 1}
    for i, c in enumerate(GOLDEN["intersect"]):
        got = IMPLS[impl].frustum_intersects(unhex(c["planes"]), unhex(c["min"]), unhex(c["max"]))
        assert bool(got) == bool(c["result"]), (i, c)


def test_corner_exactly_on_a_plane_intersects():
    """distance == 0 is not `< 0` (our_gl.cpp:275): the box touching the cube frustum's x = 1 face from outside intersects, the
    one an ulp further out does not."""
    planes = api.frustum_from_matrix(np.eye(4))
    assert api.frustum_intersects(planes, [1.0, -0.25, -0.25], [2.0, 0.25, 0.25])
    assert not api.frustum_intersects(planes, [math.nextafter(1.0, 2.0), -0.25, -0.25], [2.0, 0.25, 0.25])


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_aabb_transform_equals_the_reference(impl):
    assert len(GOLDEN["transform"]) >= 30
    for i, c in enumerate(GOLDEN["transform"]):
        lo, hi = IMPLS[impl].aabb_transform(unhex(c["min"]), unhex(c["max"]), unhex(c["m"]))
        assert same_bits(lo, unhex(c["out_min"])) and same_bits(hi, unhex(c["out_max"])), (i, lo, hi)


def _golden_meshes():
    for c in GOLDEN["bounds"]:
        yield unhex(c["v"]).reshape(c["n"], c["stride"]), unhex(c["out_min"]), unhex(c["out_max"])


@pytest.mark.parametrize("impl", ["library", "model"])
def test_mesh_bounds_equal_compute_aabb(impl):
    fn = api.mesh_bounds if impl == "library" else scene_model.compute_aabb
    n_seen = set()
    for v, want_lo, want_hi in _golden_meshes():
        lo, hi = fn(v)
        assert same_bits(lo, want_lo) and same_bits(hi, want_hi), (v.shape, lo, hi)
        n_seen.add(v.shape[0])
    assert {0, 1, 2, 1000} <= n_seen


def _mesh(n, stride, seed):
    return np.random.default_rng(seed).standard_normal((n, stride)) * 5.0


@pytest.mark.parametrize("stride", [3, 8, 14])
@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_host_mesh_bounds_equal_the_model(n, stride):
    v = _mesh(n, stride, 100 * n + stride)
    v[:, 3:] = 1e30                                        # what follows the position must not matter
    got, want = api.mesh_bounds(v), scene_model.compute_aabb(v)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def test_host_mesh_bounds_special_values():
    v = _mesh(64, 8, 5)
    v[3, 0] = math.nan; v[10, 1] = math.inf; v[20, 2] = -math.inf; v[0, :3] = math.nan; v[63, :3] = math.nan
    far = np.full((7, 3), 3e9); far[:, 1] = -3e9           # beyond the start values on both sides: the sentinels stay
    for mesh in (v, far):
        got, want = api.mesh_bounds(mesh), scene_model.compute_aabb(mesh)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    lo, hi = api.mesh_bounds(far)
    assert lo[0] == 1e9 - (3e9 - 1e9) * 0.01 and hi[0] == 3e9 + (3e9 - 1e9) * 0.01      # x: min kept 1e9, max took 3e9
    assert lo[1] == -3e9 - (-1e9 - -3e9) * 0.01 and hi[1] == -1e9 + (-1e9 - -3e9) * 0.01   # y: min took -3e9, max kept -1e9


def test_flat_mesh_at_zero_keeps_the_first_zero():
    """max - min is +-0 for a flat mesh at 0, so the bound's sign is the sign of the zero met first (std::min / std::max keep the
    earlier of equal values)."""
    a = _mesh(6, 3, 9); a[:, 1] = [0.0, -0.0, 0.0, -0.0, 0.0, 0.0]
    b = a.copy(); b[:, 1] = [-0.0, 0.0, 0.0, -0.0, 0.0, 0.0]
    ra, rb = api.mesh_bounds(a), api.mesh_bounds(b)
    for got, mesh in ((ra, a), (rb, b)):
        want = scene_model.compute_aabb(mesh)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert not math.copysign(1.0, ra[0][1]) == math.copysign(1.0, rb[0][1]), "the two vertex orders must differ in the sign of min.y"
    assert math.copysign(1.0, ra[0][1]) == 1.0 and math.copysign(1.0, rb[0][1]) == -1.0


def test_context_free_calls_reject_bad_arguments():
    L = api.load_library()
    out = (api.C.c_double * 3)()
    v = np.zeros((2, 3))
    assert L.trgl_mesh_bounds(None, v.ctypes.data, 2, 2, api.MEM_HOST, out, out) == -1         # stride < 3
    assert L.trgl_mesh_bounds(None, v.ctypes.data, 3, 2, api.MEM_DEVICE, out, out) == -1       # device memory needs a context
    assert L.trgl_mesh_bounds(None, None, 3, 2, api.MEM_HOST, out, out) == -1
    assert L.trgl_frustum_intersects(None, out, out) == -1
    assert L.trgl_frustum_from_matrix(None, None) == -1
    assert L.trgl_aabb_transform(out, out, None, out, out) == -1


def test_cull_scene_bookkeeping():
    """scene_model.cull_scene counts as main.cpp:647-736 does: rendered models add to total_triangles, culled ones to culled_triangles."""
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]) * 0.25
    away = np.eye(4); away[0, 3] = 10.0
    visible, stats = scene_model.cull_scene(np.eye(4), [(cube, 12, np.eye(4)), (cube, 7, away)])
    assert visible == [True, False]
    assert stats == dict(models_rendered=1, models_culled=1, total_triangles=12, culled_triangles=7)
