"""GPU tests of the tile binning (kernels_bin.hip: k_expand, the radix passes and the tile bounds the last pass leaves), each
frame checked against the CPU oracle: z bits, framebuffer bytes and stats exact.

The cases aim at what the binning has to get right: lists in submission order (equal depths make every tie go to the earlier
triangle), pairs staged in LDS and pairs written straight out by k_expand, lists that span radix blocks, wide (32-bit) tile
keys, pair buffers that grow behind an optimistic launch, and short lists after long ones on the same context.
"""
import numpy as np
import pytest

import cases
from oracle import orc
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT

check, same = cases.check_gpu, cases.assert_same_frame

pytestmark = pytest.mark.gpu


def _flat(W, H, clip, col):
    return cases.make_case(W, H, [(FLAT, None, clip, None, col)])


def _flat_z(clip, z):
    """The same triangles with every vertex at NDC depth z: each pixel keeps the first triangle that covers it."""
    c = clip.copy()
    c[:, [2, 6, 10]] = z * c[:, [3, 7, 11]]
    return c


def test_equal_depths_keep_submission_order_across_draws():
    """30 000 triangles at one depth in three draws: every covered pixel shows the FIRST triangle over it, so any pair that the
    sort moved ahead of an earlier one of its tile changes the image.  Small and large triangles mix (k_expand's per-thread
    and per-wave paths), and there are far more pairs than one radix block holds."""
    W = H = 512
    a, ca = scenes.random_triangles(20_000, W, H, seed=301, rmin=2, rmax=40)
    b, cb = scenes.random_triangles(2_000, W, H, seed=302, rmin=40, rmax=400)
    c, cc = scenes.random_triangles(8_000, W, H, seed=303, rmin=1, rmax=8)
    case = cases.make_case(W, H, [(FLAT, None, _flat_z(a, 0.25), None, ca), (FLAT, None, _flat_z(b, 0.25), None, cb),
                                  (FLAT, None, _flat_z(c, 0.25), None, cc)])
    got = check(case)
    assert got[2][0] == 30_000


def test_blocks_of_large_triangles_write_pairs_straight_out():
    """Blocks of 256 triangles with more pairs than k_expand stages in LDS write them straight to memory; at equal depths as well,
    with small triangles in between whose blocks are staged and whose runs start at every alignment."""
    W = H = 1024
    big, cbig = scenes.random_triangles(1_500, W, H, seed=311, rmin=200, rmax=900)
    small, csmall = scenes.random_triangles(3_001, W, H, seed=312, rmin=1, rmax=30)
    clip = _flat_z(np.concatenate([small[:1000], big, small[1000:]]), -0.5)
    col = np.concatenate([csmall[:1000], cbig, csmall[1000:]])
    check(_flat(W, H, clip, col))


def test_wide_keys_keep_submission_order():
    """More than 65536 tiles (8224x8224 = 257 x 257): 32-bit tile keys in three radix passes and the mask in a stream of its
    own.  Equal depths, and triangles in the last tile rows and columns (keys above 65535)."""
    W = H = 8224
    n = 4000
    clip, col = scenes.random_triangles(n, W, H, seed=321, rmin=8, rmax=300)
    clip = clip.copy()
    # half of them towards the far corner of the frame (NDC x and y near +1)
    clip[: n // 2, [0, 4, 8]] = clip[: n // 2, [0, 4, 8]] * 0.03 + 0.965 * clip[: n // 2, [3, 7, 11]]
    clip[: n // 2, [1, 5, 9]] = clip[: n // 2, [1, 5, 9]] * 0.03 + 0.965 * clip[: n // 2, [3, 7, 11]]
    check(_flat(W, H, _flat_z(clip, 0.0), col))


def test_wide_keys_in_eight_wave_radix_blocks():
    """Pair buffers of at least 4 M pairs sort in radix blocks of 8 waves (8192 pairs), smaller ones in blocks of 4: the same wide
    frame with 2.1 M small triangles (a first guess of 2 pairs per triangle) takes the 8-wave blocks with 32-bit keys."""
    W = H = 8224
    n = 2_100_000
    clip, col = scenes.random_triangles(n, W, H, seed=322, rmin=1, rmax=12)
    got = check(_flat(W, H, _flat_z(clip, 0.0), col))
    assert got[2][0] == n


def test_pair_buffers_grow_twice_with_equal_depths():
    """A small first flush sizes the pair buffers; the next needs several times that (the queued binning does nothing, the
    buffers grow and it is queued again), and the third more again.  Equal depths: the regrown lists must still be in order."""
    W = H = 512
    small, cs = scenes.random_triangles(500, W, H, seed=331, rmin=1, rmax=6)
    mid, cm = scenes.random_triangles(400, W, H, seed=332, rmin=300, rmax=900)
    big, cb = scenes.random_triangles(1_500, W, H, seed=333, rmin=300, rmax=900)
    o = orc.Oracle(W, H, 3)
    with Context(W, H, 3) as ctx:
        pairs = []
        for clip, col in ((small, cs), (mid, cm), (big, cb)):
            clip = _flat_z(clip, 0.5)
            ctx.draw(FLAT, clip, colors=col)
            o.draw(orc.FLAT, clip, colors=col)
            same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()), (o.fb, o.z, o.stats), what=f"frame {len(pairs)}")
            pairs.append(ctx.last_flush_info()["pairs"])
    assert pairs[1] > 2 * (2 * 500 + 4096) and pairs[2] > 2 * pairs[1], pairs       # beyond the first guess, then beyond + 25 %


def test_short_lists_after_long_ones_on_one_context():
    """A frame with long tile lists, then frames with a few short ones on the same context: the pair buffers still hold the old
    frame's words past the new pair count, and the tile bounds of the old frame must not survive (the empty flush of a clear
    in between takes the path without binning)."""
    W = H = 768
    big, cb = scenes.random_triangles(60_000, W, H, seed=341, rmin=4, rmax=120)
    few, cf = scenes.random_triangles(7, W, H, seed=342, rmin=2, rmax=20)
    o = orc.Oracle(W, H, 3)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, big, colors=cb)
        o.draw(orc.FLAT, big, colors=cb)
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()), (o.fb, o.z, o.stats), what="long lists")
        ctx.draw(FLAT, few, colors=cf)          # on top of the first frame
        o.draw(orc.FLAT, few, colors=cf)
        same((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()), (o.fb, o.z, o.stats), what="short lists on top")
        ctx.clear()
        ctx.read_framebuffer()                  # a flush without triangles
        ctx.draw(FLAT, few, colors=cf)
        fresh = orc.Oracle(W, H, 3)
        fresh.draw(orc.FLAT, few, colors=cf)
        same((ctx.read_framebuffer(), ctx.read_zbuffer()), (fresh.fb, fresh.z), stats=False, what="short lists after a clear")
