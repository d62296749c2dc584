"""trgl_mesh_bounds on meshes in device memory (k_mesh_bounds + k_mesh_bounds_fold) against its host path, bit for bit, and
trgl_zbuffer_snapshot / _restore / _snapshot_free against frames drawn without them.  tests/test_scene_cpu.py holds the host path to
the reference's own compiled Model::computeAABB.

The bounds kernel gives every block 4 x 256 vertices per round of its grid-stride loop and runs ceil(n / 1024) blocks (at most 1024):
the sizes below sit on both sides of a wave (64), of a block's threads (256) and of one block's round (1024), and 70 001 vertices are
69 blocks that each go round the loop four times, the last round partial."""
import math

import numpy as np
import pytest

import cases
import scene_model
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, Context, TrglError

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 70001]
BIG = 70001
STEP = 69 * 256          # vertices between a thread's visits when n = BIG


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def device_mesh(v):
    """The mesh on the device, its first double 8 bytes past a 16-byte boundary (vertices are only 8-byte aligned)."""
    import torch
    t = cases.device_array(v, off=8)
    assert t.data_ptr() % 16 == 8
    torch.cuda.synchronize()             # the upload ran on torch's stream; the context's own stream waits for nobody
    return t


def assert_device_equals_host(ctx, v, what=""):
    want = api.mesh_bounds(v)
    got = ctx.mesh_bounds(device_mesh(v), device=True)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (what, got, want)
    return got


@pytest.fixture(scope="module")
def ctx():
    with Context(64, 64, 3, device=0) as c:
        yield c


def random_mesh(n, stride, seed, sprinkle=True):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, stride)) * 4.0
    v[:, 3:] = 1e300                                     # what follows the position must not be read as one
    if sprinkle and n >= 8:
        k = rng.integers(0, n, max(3, n // 50))
        v[k[0::3], rng.integers(0, 3)] = math.nan
        v[k[1::3], rng.integers(0, 3)] = math.inf
        v[k[2::3], rng.integers(0, 3)] = -math.inf
    return v


@pytest.mark.parametrize("stride", [3, 8, 14])
@pytest.mark.parametrize("n", SIZES)
def test_device_bounds_equal_host_bounds(ctx, n, stride):
    assert_device_equals_host(ctx, random_mesh(n, stride, 1000 * stride + n))


def test_host_path_equals_the_model_on_the_big_mesh():
    v = random_mesh(BIG, 3, 77)
    got, want = api.mesh_bounds(v), scene_model.compute_aabb(v)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("n", [257, 1025, BIG])
def test_each_extreme_at_the_first_the_last_and_a_tail_vertex(ctx, n):
    """A vertex skipped at either end of the array, or in the partial last round of the loop, would hold the extreme."""
    base = random_mesh(n, 8, n, sprinkle=False)
    tail = n - 1 - (n % 256) // 2 if n % 256 > 1 else n - 2          # inside the last, partial block of the last round
    for where in (0, n - 1, tail):
        for axis in range(3):
            for value in (-50.0 - axis, 60.0 + axis):
                v = base.copy(); v[where, axis] = value
                got = assert_device_equals_host(ctx, v, (where, axis, value))
                margin = (v[:, axis].max() - v[:, axis].min()) * 0.01
                assert (got[0][axis] == value - margin) if value < 0 else (got[1][axis] == value + margin)


# (earlier vertex, later vertex) of n = BIG: the later one is met by a lower lane of the same wave, by a lower wave of the same block,
# and by a lower block than the earlier one, so an order of combining that ignores the vertex index keeps the wrong zero
TIE_PARTNERS = {"lanes": (40, STEP + 3), "waves": (200, STEP + 5), "blocks": (3 * 256 + 7, STEP + 10), "rounds": (STEP - 1, 2 * STEP)}


@pytest.mark.parametrize("first_zero", [0.0, -0.0])
@pytest.mark.parametrize("where", sorted(TIE_PARTNERS))
def test_flat_mesh_at_zero_keeps_the_earlier_zero(ctx, where, first_zero):
    """y is NaN (never a bound) except at two vertices holding +0.0 and -0.0: min.y = max.y = the EARLIER one, whose sign shows in
    min.y - (+0).  The two orders must differ, as scene_model says."""
    i1, i2 = TIE_PARTNERS[where]
    v = random_mesh(BIG, 3, 5, sprinkle=False)
    v[:, 1] = math.nan
    v[i1, 1], v[i2, 1] = first_zero, -first_zero
    got = assert_device_equals_host(ctx, v, where)
    want = scene_model.compute_aabb(v)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert got[0][1] == 0.0 and math.copysign(1.0, got[0][1]) == math.copysign(1.0, first_zero)


def test_flat_mesh_of_many_zeros(ctx):
    """Every y is a zero, the signs mixed, -0.000000 first as in a Blender export: the first vertex decides."""
    for first in (0.0, -0.0):
        v = random_mesh(BIG, 14, 6, sprinkle=False)
        v[:, 1] = np.where(np.random.default_rng(3).integers(0, 2, BIG) == 1, 0.0, -0.0)
        v[0, 1] = first
        got = assert_device_equals_host(ctx, v)
        assert math.copysign(1.0, got[0][1]) == math.copysign(1.0, first)


def test_all_beyond_the_start_values_and_empty(ctx):
    far = np.full((300, 3), 2e9); far[:, 2] = -2e9
    got = assert_device_equals_host(ctx, far)
    assert got[0][0] == 1e9 - 1e7 and got[1][2] == -1e9 + 1e7             # the start values stayed on the far side
    import torch
    lo, hi = ctx.mesh_bounds(torch.empty((0, 3), dtype=torch.float64, device="cuda"), device=True)
    assert not lo.any() and not hi.any()                                   # model.cpp:16-19


def test_two_calls_in_a_row_reuse_the_scratch():
    with Context(32, 32, 3, device=0) as c:
        a, b = random_mesh(BIG, 8, 1), random_mesh(1025, 3, 2)
        ra = assert_device_equals_host(c, a)
        rb = assert_device_equals_host(c, b)                               # fewer blocks than before: stale partials must not count
        assert not np.array_equal(bits(ra[0]), bits(rb[0]))
        assert_device_equals_host(c, a)


def test_bad_arguments(ctx):
    import torch
    t = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(TrglError):
        ctx.mesh_bounds(t, device=True)                                    # stride < 3
    with pytest.raises(TypeError):
        ctx.mesh_bounds(np.zeros((4, 3)), device=True)                     # a host array handed over as a device one
    for call in (ctx.zbuffer_snapshot, ctx.zbuffer_restore, ctx.zbuffer_snapshot_free):
        for slot in (-1, api.MAX_Z_SNAPSHOTS):
            with pytest.raises(TrglError, match=r"\(-1\)"):
                call(slot)                                                 # TRGL_E_INVALID


# ---- frames ------------------------------------------------------------------------------------------------------------

def _frame_inputs(W, H):
    a = scenes.random_triangles(700, W, H, seed=11, rmin=2, rmax=24)
    b_clip, b_col = scenes.random_triangles(500, W, H, seed=12, rmin=2, rmax=24)
    b_clip = b_clip.copy(); b_clip[:, 2::4] -= 1.5                         # in front of A (w = 1: z is the third of every four)
    return a, (b_clip, b_col ^ np.uint32(0x00a5a5a5))


_REF = {}


def reference_frames(W, H):
    """Frames drawn WITHOUT snapshots, once per size: after A alone, and after A then B."""
    if (W, H) not in _REF:
        (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
        out = {}
        with Context(W, H, 3, device=0) as c:
            c.draw(FLAT, a_clip, colors=a_col)
            out["A"] = dict(fb=c.read_framebuffer(), z=c.read_zbuffer(), stats=c.stats(), post=c.postprocess())
            c.draw(FLAT, b_clip, colors=b_col)
            out["AB"] = dict(fb=c.read_framebuffer(), z=c.read_zbuffer(), stats=c.stats())
        assert not np.array_equal(bits(out["A"]["z"]), bits(out["AB"]["z"]))
        for o in out.values():
            for k in ("fb", "z"):
                o[k].setflags(write=False)
        _REF[(W, H)] = out
    return _REF[(W, H)]


FRAME_SIZES = [(101, 67), (256, 256)]


@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_bounds_call_between_draw_and_flush_leaves_the_frame(W, H):
    ref = reference_frames(W, H)
    (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
    mesh = random_mesh(BIG, 8, 4)
    with Context(W, H, 3, device=0) as c:
        c.draw(FLAT, a_clip, colors=a_col)
        assert_device_equals_host(c, mesh)                                 # the draws stay queued
        c.draw(FLAT, b_clip, colors=b_col)
        c.flush_begin()
        assert_device_equals_host(c, mesh)                                 # completes the begun flush
        c.flush()
        assert np.array_equal(c.read_framebuffer(), ref["AB"]["fb"]) and np.array_equal(bits(c.read_zbuffer()), bits(ref["AB"]["z"]))
        assert c.stats() == ref["AB"]["stats"]


@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_snapshot_draw_restore(W, H):
    """main.cpp:700-730: depths of A, colours and counters of A + B; then main.cpp:751-763 on the restored depths."""
    ref = reference_frames(W, H)
    (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
    with Context(W, H, 3, device=0) as c:
        c.draw(FLAT, a_clip, colors=a_col)
        c.zbuffer_snapshot()                                               # flushes A first
        c.draw(FLAT, b_clip, colors=b_col)
        c.zbuffer_restore()                                                # flushes B first: it shows in the colours
        assert c.stats() == ref["AB"]["stats"]
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"]))
        assert np.array_equal(c.read_framebuffer(), ref["AB"]["fb"])
        post = c.postprocess()
        assert np.array_equal(post["zbuffer_image"], ref["A"]["post"]["zbuffer_image"])
        assert np.array_equal(post["ao"], ref["A"]["post"]["ao"])
        # the composite multiplies A + B's colours with the occlusion of A's depths: equal to A's wherever B drew nothing
        same_px = (ref["AB"]["fb"] == ref["A"]["fb"]).all(axis=-1)
        assert same_px.any() and np.array_equal(post["final"][same_px], ref["A"]["post"]["final"][same_px])


@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_postprocess_after_restore_equals_the_frame_without_the_second_draw(W, H):
    """B drawn and then undone entirely - depths restored, colours written back - post-processes byte for byte like A alone."""
    ref = reference_frames(W, H)
    (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
    with Context(W, H, 3, device=0) as c:
        c.draw(FLAT, a_clip, colors=a_col)
        c.zbuffer_snapshot(2)
        c.draw(FLAT, b_clip, colors=b_col)
        c.zbuffer_restore(2)
        c.write_framebuffer(ref["A"]["fb"])
        post = c.postprocess()
        for k in ("zbuffer_image", "ao", "final"):
            assert np.array_equal(post[k], ref["A"]["post"][k]), k


def test_stats_unchanged_and_two_slots_hold_two_states():
    W, H = FRAME_SIZES[0]
    ref = reference_frames(W, H)
    (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
    with Context(W, H, 3, device=0) as c:
        c.draw(FLAT, a_clip, colors=a_col)
        before = c.stats()
        c.zbuffer_snapshot(0)
        assert c.stats() == before == ref["A"]["stats"]
        c.draw(FLAT, b_clip, colors=b_col)
        c.zbuffer_snapshot(3)
        after = c.stats()
        c.zbuffer_restore(0)
        assert c.stats() == after == ref["AB"]["stats"]
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"]))
        c.zbuffer_restore(3)
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["AB"]["z"]))
        c.zbuffer_restore(0)
        c.zbuffer_snapshot(3)                                              # a slot in use is overwritten, not reallocated
        c.zbuffer_restore(3)
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"]))
        assert np.array_equal(c.read_framebuffer(), ref["AB"]["fb"]) and c.stats() == after


def test_empty_and_freed_slots_refuse_a_restore():
    W, H = FRAME_SIZES[0]
    ref = reference_frames(W, H)
    (a_clip, a_col), _ = _frame_inputs(W, H)
    with Context(W, H, 3, device=0) as c:
        c.draw(FLAT, a_clip, colors=a_col)
        with pytest.raises(TrglError, match=r"\(-4\)"):                    # TRGL_E_STATE
            c.zbuffer_restore(1)
        c.zbuffer_snapshot(1)
        c.zbuffer_restore(1)
        c.zbuffer_snapshot_free(1)
        c.zbuffer_snapshot_free(1)                                         # freeing an empty slot is not an error
        with pytest.raises(TrglError, match=r"\(-4\)"):
            c.zbuffer_restore(1)
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"])) and np.array_equal(c.read_framebuffer(), ref["A"]["fb"])


def test_snapshot_completes_a_begun_flush_and_a_pending_clear():
    W, H = FRAME_SIZES[0]
    ref = reference_frames(W, H)
    (a_clip, a_col), (b_clip, b_col) = _frame_inputs(W, H)
    with Context(W, H, 3, device=0) as c:
        c.zbuffer_snapshot(1)                                              # a new context: the pending clear runs first
        c.draw(FLAT, a_clip, colors=a_col)
        c.flush_begin()
        c.zbuffer_snapshot(0)                                              # between flush_begin and flush_end: A is in the snapshot
        c.draw(FLAT, b_clip, colors=b_col)
        c.flush_begin()
        c.zbuffer_restore(0)                                               # likewise: B is drawn before the depths are replaced
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"]))
        assert np.array_equal(c.read_framebuffer(), ref["AB"]["fb"]) and c.stats() == ref["AB"]["stats"]
        c.zbuffer_restore(1)
        assert np.isposinf(c.read_zbuffer()).all()
        c.clear()
        c.zbuffer_restore(0)                                               # the clear comes first and does not undo the restore
        assert np.array_equal(bits(c.read_zbuffer()), bits(ref["A"]["z"]))
