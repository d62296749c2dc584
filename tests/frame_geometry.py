"""Frames at the edges of what trgl_create accepts, and two scenes for each: shared by test_frame_geometry.py (CPU: the scenes
reach what they claim) and test_frame_geometry_gpu.py (every frame kernel on them).

The reference's rasterize() has no notion of a tile; the kernels have 32 x 32 tiles, one 8 x 8 block per wave, vector stores chosen
by W & 1 and W & 3, and 16-bit pixel coordinates packed into the records (TriRec bx0 | by0 << 16, BlockState::xy).  Each frame is
here for a branch:

  below one block   1x1, 2x3, 7x5        every lane of a block but a few is unowned; n < 4 tails of the post kernels; 1 tile
  one block, one    8x8, 9x9             block-out's `whole` (X0 + 7 < W) true and false in the same tile
  over
  around one tile   31x33 32x32 33x31    1 tile, 1 x 2 and 2 x 1 tiles (a 1-bit sort key); W & 3 = 3, 0, 1, 2, 3; clear_rows' full_x
                    34x30 35x29          true (32x32, and the first tile of 33.., 34.., 35..) and false; odd W at every bpp
  thin              1x70 70x1 5x40 40x5  row stride 1; 3 tiles in a row or a column; W < 8: no block is ever whole
  limits            65535x2, 2x65535     coordinate 65534, tile 2047, 2048 x 1 and 1 x 2048 tiles, mostly clear-only work items

Scenes (scene()): `dense` - random triangles with radii scaled to the frame and perspective w; `sparse` - few enough that cleared
pixels remain.  Both hold four hand-placed triangles at the corner (W - 1, H - 1), so that the last column and the last row are
always written; on the limit frames also one over pixel (0, 0) and one that straddles the boundary between the last two tiles
(random triangles alone leave the last column of 65535x2 empty).  The triangles are shuffled, so that a MIXED case (four draws of a
quarter each) has hand-placed and random ones in several kinds.
"""
import functools

import numpy as np

import cases
from test_raster_paths import KINDS, KIND_NAMES, MIXED, _kind_case      # noqa: F401  (re-exported for the tests)
from tinyrenderder_amd import scenes

FRAMES = [(1, 1), (2, 3), (7, 5), (8, 8), (9, 9), (31, 33), (32, 32), (33, 31), (34, 30), (35, 29), (1, 70), (70, 1), (5, 40), (40, 5),
          (65535, 2), (2, 65535)]
LIMIT_FRAMES = [f for f in FRAMES if max(f) == 65535]
SMALL_FRAMES = [f for f in FRAMES if f not in LIMIT_FRAMES]
BELOW_ONE_BLOCK = [(1, 1), (2, 3), (7, 5)]
THIN_FRAMES = [(1, 70), (70, 1), (5, 40), (40, 5)]
SCENES = ("dense", "sparse")
BPPS = (1, 3, 4)
CLEAR, ZCLEAR = (30, 20, 10, 200), 0.75          # not the defaults: a wrong clear byte or depth shows
TILE = 32


def frame_id(f):
    return f"{f[0]}x{f[1]}"


def px_triangle(W, H, pts, z):
    """One clip row (w = 1) for the default viewport of a W x H frame from three pixel-space points and their depths, wound
    counter-clockwise (our_gl.cpp:124-127 keeps it)."""
    pts, z = list(pts), list(z)
    (x0, y0), (x1, y1), (x2, y2) = pts
    if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) < 0:
        pts[1], pts[2], z[1], z[2] = pts[2], pts[1], z[2], z[1]
    row = []
    for (x, y), d in zip(pts, z):
        row += [x * 2.0 / W - 1.0, y * 2.0 / H - 1.0, d, 1.0]
    return row


# a triangle around the pixel centre (-0.5, -0.5) relative to a frame corner at (0, 0), inside by more than a pixel's third
_CORNER = ((-4.2, -1.8), (1.3, -1.8), (-0.2, 1.4))


def hand_placed(W, H):
    """Four triangles at the corner (W - 1, H - 1), each 0.6 px further left (the first covers the corner pixel; none reaches
    below row H - 2); on the limit frames one over pixel (0, 0) and one across the boundary of the last two tiles of the long axis."""
    rows = []
    for k in range(4):
        rows.append(px_triangle(W, H, [(W + x - 0.6 * k, H + y) for x, y in _CORNER], (0.3 - 0.2 * k, -0.4 + 0.25 * k, 0.1 * k - 0.2)))
    if (W, H) in LIMIT_FRAMES:
        rows.append(px_triangle(W, H, [(-x, -y) for x, y in _CORNER], (-0.3, 0.2, 0.1)))
        b = float(TILE * ((max(W, H) + TILE - 1) // TILE - 1))
        along = [(b - 9.3, -0.4), (b + 8.7, -0.3), (b + 0.4, 3.1)]
        rows.append(px_triangle(W, H, along if W > H else [(y, x) for x, y in along], (-0.6, 0.1, 0.4)))
    clip = np.array(rows, np.float64)
    col = (np.arange(len(rows), dtype=np.uint32) * np.uint32(0x3A5F17) + np.uint32(0x102030)) | np.uint32(0xFF000000)
    return clip, col


@functools.lru_cache(maxsize=None)
def scene(W, H, which):
    """(clip [n, 12], colours [n]) of the `dense` or the `sparse` scene of a frame; n >= 4."""
    limit = (W, H) in LIMIT_FRAMES
    seed = 7000 + 10 * FRAMES.index((W, H))
    if which == "dense":
        n, rmax = (400, 64.0) if limit else (40, max(2.0, min(max(W, H) / 2.0, 24.0)))
        rnd = scenes.random_triangles(n, W, H, seed=seed, rmin=1.0, rmax=rmax, perspective_w=True)
    else:
        n, rmax = (12, 32.0) if limit else (3 if W * H >= 64 else 0, max(2.0, min(max(W, H) / 8.0, 6.0)))
        rnd = scenes.random_triangles(n, W, H, seed=seed + 1, rmin=1.0, rmax=rmax)
    hc, hk = hand_placed(W, H)
    clip, col = np.concatenate([rnd[0], hc]), np.concatenate([rnd[1] | np.uint32(0x00404040), hk])
    order = np.argsort(scenes.SplitMix64(seed + 2).u64(len(clip)), kind="stable")
    clip, col = np.ascontiguousarray(clip[order]), np.ascontiguousarray(col[order])
    clip.setflags(write=False); col.setflags(write=False)
    return clip, col


@functools.lru_cache(maxsize=None)
def case(W, H, which, kind, bpp):
    """The scene drawn with `kind` (an entry of KINDS) into a W x H frame of bpp bytes per pixel, cleared to CLEAR / ZCLEAR."""
    clip, col = scene(W, H, which)
    c = _kind_case(kind, clip, col, W, H, bpp, seed=7500 + FRAMES.index((W, H)), clear=CLEAR)
    return dict(c, zclear=ZCLEAR)


def big_frame(c):
    """The same draws with the same viewport matrix in a frame of max(W, 128) x max(H, 128): our_gl.cpp:130-192 reads the frame size
    only in the bbox clamp, so rows [0, H) x columns [0, W) of this frame hold the small frame's bytes and depths (the crop
    identity; test_frame_geometry.py holds the oracle to it)."""
    return dict(c, width=max(c["width"], 128), height=max(c["height"], 128))


def _oracle(W, H, which, kind, bpp, strip, loaded):
    from oracle import orc
    start = cases.loaded_buffers(W, H, bpp) if loaded else None
    fb, z, st = cases.run_oracle(case(W, H, which, kind, bpp), strip=strip, start=start)
    fb.setflags(write=False); z.setflags(write=False)
    return fb, z, st, orc.format_stats_line(st)


_oracle_small = functools.lru_cache(maxsize=None)(_oracle)
_oracle_limit = functools.lru_cache(maxsize=96)(_oracle)          # (a limit frame's buffers take 1.5 MB)


def oracle(W, H, which, kind, bpp, strip=None, loaded=False):
    """cases.run_oracle of case(...) plus the stats line, computed once and shared (read-only)."""
    return (_oracle_limit if (W, H) in LIMIT_FRAMES else _oracle_small)(W, H, which, kind, bpp, strip, loaded)


def covered(c, z):
    """bool [H, W]: pixels whose depth is no longer the clear value"""
    return z.view(np.uint64) != np.float64(c["zclear"]).view(np.uint64)


def odd_cut(H):
    """The odd row at which two strip contexts cut a frame of H >= 2 rows: H // 2 | 1 where that is below H."""
    y = H // 2 | 1
    return y if y < H else 1
