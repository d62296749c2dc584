"""The scenes of tests/frame_geometry.py reach what they claim - on the CPU oracle and tests/binning_model.py alone, no GPU.

test_frame_geometry_gpu.py runs every frame kernel on these frames; a scene that drew nothing, or left no cleared pixel, or never
touched the last column would let a wrong predicate in clear_rows, block-out or k_make_items pass unseen.  The crop identity at the
end licenses the device-against-device comparison that the GPU tests use for EYE colours on frames too small for the 0.1 % rule.
"""
import numpy as np
import pytest

import binning_model as bm
import cases
import frame_geometry as fg
from frame_geometry import FRAMES, KINDS, KIND_NAMES, LIMIT_FRAMES, SCENES, SMALL_FRAMES, frame_id
from tinyrenderder_amd.api import EYE, FLAT


def test_frames_cover_the_geometry_branches():
    """The predicates the kernels branch on, evaluated for FRAMES: clear_rows' full_x with (W & 1) == 0 and with odd W, full_x with
    every W & 3, frames with no full_x tile at all (W < 32); block-out's `whole` (X0 + 7 < W) true and false in one tile, and
    frames without a whole block (W < 8); k_make_items' row mask for tiles of which 1 to 7 rows exist; 1 and 2 tiles (the 1-bit
    sort key), 2048 x 1 and 1 x 2048 tiles; a coordinate of 65534 in either half of the packed pairs."""
    full_x = {(W & 3) for W, H in FRAMES if W >= 32}
    assert full_x == {0, 1, 2, 3}                                           # a full_x tile next to every W & 3
    assert {(W & 3) for W, H in FRAMES if W < 32} >= {1, 2, 3}             # ... and no full_x tile at all
    assert any(W < 32 and W & 1 == 0 for W, H in FRAMES) and any(W < 32 and W & 1 for W, H in FRAMES)
    assert any(8 <= W and W % 8 for W, H in FRAMES) and any(W < 8 for W, H in FRAMES) and (8, 8) in FRAMES
    assert {H % 32 for W, H in FRAMES if 0 < H % 32 < 8} >= {1, 2, 3, 5}   # partial last tile rows of fewer than 8 rows
    tiles = {((W + 31) // 32, (H + 31) // 32) for W, H in FRAMES}
    assert {(1, 1), (1, 2), (2, 1), (2048, 1), (1, 2048), (1, 3), (3, 1)} <= tiles
    assert (65535, 2) in LIMIT_FRAMES and (2, 65535) in LIMIT_FRAMES
    assert all(3 * W % 4 for W, H in FRAMES if W & 3)                       # block-out's RGB row dwords are unaligned on row 1


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_scenes_draw_and_reach_the_last_column_and_row(frame):
    """Every scene of every kind and pixel size draws fragments and covers a pixel in the last column and one in the last row; every
    sparse scene of a frame of two pixels or more also leaves a pixel at the clear colour and depth."""
    W, H = frame
    for which in SCENES:
        for kind in KINDS:
            for bpp in fg.BPPS:
                c = fg.case(W, H, which, kind, bpp)
                fb, z, st, _ = fg.oracle(W, H, which, kind, bpp)
                what = f"{frame_id(frame)} {which} {KIND_NAMES[kind]} bpp {bpp}"
                assert st[1] > 0, what
                cov = fg.covered(c, z)
                assert cov[:, W - 1].any() and cov[H - 1, :].any(), what
                if which == "sparse" and W * H >= 2:
                    clear = (fb == np.array(fg.CLEAR[:bpp], np.uint8)).all(-1) & ~cov
                    assert clear.any() and cov.any(), what
        assert sum(len(d[2]) for d in c["draws"]) >= 4 and all(len(d[2]) for d in c["draws"])       # MIXED: no empty draw


@pytest.mark.parametrize("frame", LIMIT_FRAMES, ids=frame_id)
@pytest.mark.parametrize("which", SCENES)
def test_limit_scenes_reach_tile_2047_and_coordinate_65534(frame, which):
    """The model of k_setup and the binning on 65535x2 / 2x65535: a pair in tile 2047, a record whose packed bbox holds 65534 (TriRec
    bx1 or by1), tiles without pairs (clear-only work items), pixel (0, 0) and pixel (W - 1, H - 1) covered, and a triangle whose
    tiles are the last two."""
    W, H = frame
    c = fg.case(W, H, which, FLAT, 3)
    m = bm.model(c)
    assert (m.tiles_x, m.tiles_y) == ((2048, 1) if W > H else (1, 2048))
    ps = bm.pairs(m)
    tiles = {t for t, _, _ in ps}
    assert 2047 in tiles and 0 in tiles and len(tiles) < 2048
    far = m.bx1 if W > H else m.by1
    assert (far[m.has_pairs] == 65534).any()
    by_tri = {}
    for t, i, _ in ps:
        by_tri.setdefault(i, set()).add(t)
    assert {2046, 2047} in by_tri.values()
    cov = fg.covered(c, fg.oracle(W, H, which, FLAT, 3)[1])
    assert cov[0, 0] and cov[H - 1, W - 1]
    assert cov[:, 2046 * 32:].any() if W > H else cov[2046 * 32:, :].any()


@pytest.mark.parametrize("frame,tiles", [((7, 5), 1), ((1, 1), 1), ((32, 32), 1), ((31, 33), 2), ((33, 31), 2), ((34, 30), 2), ((35, 29), 2)], ids=str)
def test_one_and_two_tile_frames_have_one_and_two_tiles(frame, tiles):
    """trgl_api.cpp sorts by a key of 1 bit where a frame has 1 or 2 tiles; the model has exactly that many, each with pairs."""
    W, H = frame
    m = bm.model(fg.case(W, H, "dense", FLAT, 3))
    assert m.tiles_x * m.tiles_y == tiles
    assert {t for t, _, _ in bm.pairs(m)} == set(range(tiles))


def _crop_identity(W, H, which, kind, bpp):
    c = fg.case(W, H, which, kind, bpp)
    small = fg.oracle(W, H, which, kind, bpp)
    big = cases.run_oracle(fg.big_frame(c))
    what = f"{W}x{H} {which} {KIND_NAMES[kind]} bpp {bpp}"
    assert np.array_equal(big[1][:H, :W].view(np.uint64), small[1].view(np.uint64)), what
    assert np.array_equal(big[0][:H, :W], small[0]), what
    assert big[2][0] == small[2][0]                                         # the same triangles pass the culling


@pytest.mark.parametrize("frame", SMALL_FRAMES, ids=frame_id)
def test_crop_identity_on_the_oracle(frame):
    """The same draws with the same viewport matrix in a frame of max(W, 128) x max(H, 128): framebuffer bytes and z bits at
    [0:H, 0:W] equal the small frame's, for every kind including EYE (our_gl.cpp:130-192: only the bbox clamp reads the frame
    size).  The GPU tests compare EYE colours of the small frames with the crop of the device's own large frame on this ground."""
    W, H = frame
    for which in SCENES:
        for kind in KINDS:
            for bpp in ((1, 3, 4) if kind in (FLAT, EYE) else (3,)):
                _crop_identity(W, H, which, kind, bpp)


@pytest.mark.parametrize("frame", LIMIT_FRAMES, ids=frame_id)
def test_crop_identity_on_the_limit_frames(frame):
    W, H = frame
    for kind in (FLAT, EYE):
        _crop_identity(W, H, "sparse", kind, 3)
