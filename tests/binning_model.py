"""Host model of what k_setup and the binning leave for k_raster (csrc/trgl_device.h), in plain numpy fp64.

Written from our_gl.cpp:89-141 and the struct comments, not from the kernels: one product and one sum per operation, in the
reference's order (dot4 is a left-to-right sum from 0, geometry.h:122-127; no `@` / `dot`, which may fuse or reorder).
model(case, strip, interleave) returns a Model:
  per triangle of the flush (arrays of length N, submission order across the draws): accepted, bx0 by0 bx1 by1 (clamped bbox,
  our_gl.cpp:130-133), ax ay s0x s0y s1x s1y uz z0 z1 z2 (our_gl.cpp:78-80, 117-121, 156-158), color, draw, local, well_scaled
  (DESIGN.md "Exactness" / k_setup), has_pairs (accepted, |u.z| >= 1e-12, bbox reaches an owned row), cnt (owned tiles
  the clipped bbox touches), large (clipped bbox at least 64 pixels wide or high);
  pairs(): the expected set of (tile, triangle, 4x4 mask of exactly the 8x8 blocks that (bbox n strip) touches).
"""
import numpy as np

TILE, BLOCK = 32, 8
INT_MIN = -2147483648


def _dot4(m, v):
    s = 0.0 + m[0] * v[0]
    s = s + m[1] * v[1]
    s = s + m[2] * v[2]
    s = s + m[3] * v[3]
    return s


def _min3(a, b, c):
    m = np.where(b < a, b, a)
    return np.where(c < m, c, m)


def _max3(a, b, c):
    m = np.where(a < b, b, a)
    return np.where(m < c, c, m)


def _cvt(a):
    """(int)double as the reference's x86-64 build executes it: NaN and out of range give INT_MIN"""
    ok = (a > -2147483649.0) & (a < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, a, 0.0)), float(INT_MIN)).astype(np.int64)


def owned_tile_rows(H, strip=None, interleave=None):
    """bool per tile row: does the context own (part of) it.  strip = (y0, y1) rows; interleave = (band_rows, rank, world)."""
    tiles_y = (H + TILE - 1) // TILE
    ty = np.arange(tiles_y)
    if interleave is not None and interleave[2] > 1:
        band, rank, world = interleave
        return (ty // (band // TILE)) % world == rank
    y0, y1 = (0, H) if strip is None or interleave is not None else strip
    if y1 <= y0:
        return np.zeros(tiles_y, bool)
    return (ty >= y0 // TILE) & (ty < (y1 + TILE - 1) // TILE)


class Model:
    pass


def model(case, strip=None, interleave=None, draws=None):
    """draws: the (kind, uniforms, clip, varyings, colours) of ONE flush, by default all of the case's."""
    W, H = case["width"], case["height"]
    vp = np.asarray(case["viewport"], np.float64).reshape(4, 4)
    draws = [d for d in (case["draws"] if draws is None else draws) if len(d[2])]        # an empty draw queues nothing
    clip = np.concatenate([np.asarray(d[2], np.float64).reshape(-1, 12) for d in draws]) if draws else np.zeros((0, 12))
    N = len(clip)
    m = Model()
    m.N, m.W, m.H, m.clip = N, W, H, clip
    m.tiles_x, m.tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    m.draw = np.concatenate([np.full(len(d[2]), i, np.int64) for i, d in enumerate(draws)]) if draws else np.zeros(0, np.int64)
    m.local = np.concatenate([np.arange(len(d[2]), dtype=np.int64) for d in draws]) if draws else np.zeros(0, np.int64)
    m.color = np.concatenate([np.full(len(d[2]), 0xffffffff, np.uint32) if d[4] is None else np.asarray(d[4], np.uint32)
                              for d in draws]) if draws else np.zeros(0, np.uint32)
    y0s, y1s = (0, H) if strip is None or interleave is not None else strip
    m.strip = (y0s, y1s)
    m.owned_rows = owned_tile_rows(H, strip, interleave)
    with np.errstate(all="ignore"):
        w = [clip[:, 4 * q + 3] for q in range(3)]
        ok = ~((w[0] <= 1e-12) | (w[1] <= 1e-12) | (w[2] <= 1e-12))                              # :94
        ndc = [[clip[:, 4 * q + k] / w[q] for k in range(4)] for q in range(3)]                   # :101
        zo = [(ndc[q][2] < -1.0) | (ndc[q][2] > 1.0) for q in range(3)]
        ok &= ~(zo[0] & zo[1] & zo[2])                                                           # :103-106
        for q in range(3):
            for k in range(4):
                ok &= np.isfinite(ndc[q][k])                                                     # :109-114
        sx = [_dot4(vp[0], ndc[q]) for q in range(3)]                                            # :117-121
        sy = [_dot4(vp[1], ndc[q]) for q in range(3)]
        e1x, e1y, e2x, e2y = sx[1] - sx[0], sy[1] - sy[0], sx[2] - sx[0], sy[2] - sy[0]
        cross = e1x * e2y - e1y * e2x                                                            # :124-126
        ok &= ~(cross <= 0)                                                                      # :127
        bx0 = np.maximum(0, _cvt(np.floor(_min3(*sx))))                                          # :130-133
        bx1 = np.minimum(W - 1, _cvt(np.ceil(_max3(*sx))))
        by0 = np.maximum(0, _cvt(np.floor(_min3(*sy))))
        by1 = np.minimum(H - 1, _cvt(np.ceil(_max3(*sy))))
        ok &= ~((bx0 > bx1) | (by0 > by1))                                                       # :135
        m.accepted = ok
        m.bx0, m.by0, m.bx1, m.by1 = bx0, by0, bx1, by1
        m.ax, m.ay = sx[0], sy[0]
        m.s0x, m.s0y = sx[2] - sx[0], sx[1] - sx[0]                                              # :78
        m.s1x, m.s1y = sy[2] - sy[0], sy[1] - sy[0]                                              # :79
        m.uz = m.s0x * m.s1y - m.s0y * m.s1x                                                     # :80
        m.z0, m.z1, m.z2 = ndc[0][2], ndc[1][2], ndc[2][2]                                       # :156-158
        # "well scaled" (DESIGN.md "Exactness", k_setup)
        ws = (m.uz < 0.0) & ~(np.abs(m.uz) < 1e-12)
        for q in range(3):
            ws &= (np.abs(sx[q]) < 2.0 ** 200) & (np.abs(sy[q]) < 2.0 ** 200)
        for d in (m.s0x, m.s0y, m.s1x, m.s1y):
            ws &= (d == 0.0) | (np.abs(d) >= 2.0 ** -250)
        S = (np.abs(m.s0x) + np.abs(m.s0y)) + (np.abs(m.s1x) + np.abs(m.s1y))
        rx = np.fmax(np.abs(m.ax - (bx0 + 0.5)), np.abs(m.ax - (bx1 + 0.5)))
        ry = np.fmax(np.abs(m.ay - (by0 + 0.5)), np.abs(m.ay - (by1 + 0.5)))
        ws &= 2.0 ** -40 * (S * S) * (rx + ry + 17.0 + S) < np.abs(m.uz)
        m.well_scaled = ws & ok
    # the rows of the bbox inside the strip, and the tiles of owned rows it touches
    ylo, yhi = np.maximum(by0, y0s), np.minimum(by1, y1s - 1)
    m.ylo, m.yhi = ylo, yhi
    cand = ok & ~(np.abs(m.uz) < 1e-12) & (ylo <= yhi)
    below = np.concatenate([[0], np.cumsum(m.owned_rows)])          # owned tile rows below row r
    rows = np.where(cand, below[np.clip(yhi // TILE + 1, 0, m.tiles_y)] - below[np.clip(ylo // TILE, 0, m.tiles_y)], 0)
    m.cnt = np.where(cand, (bx1 // TILE - bx0 // TILE + 1) * rows, 0).astype(np.int64)
    m.has_pairs = m.cnt > 0
    m.large = m.has_pairs & ((bx1 - bx0 >= 64) | (yhi - ylo >= 64))
    m.literal = m.has_pairs & ~m.well_scaled
    return m


def triangle_tiles(m, i):
    """[(tile id, mask)] of triangle i in row-major tile order: bit 4 r + c of the mask = block (c, r) of the tile is touched by
    (bbox n strip)."""
    if not m.has_pairs[i]:
        return []
    qx0, qx1, qy0, qy1 = int(m.bx0[i]) // BLOCK, int(m.bx1[i]) // BLOCK, int(m.ylo[i]) // BLOCK, int(m.yhi[i]) // BLOCK
    out = []
    for ty in range(qy0 // 4, qy1 // 4 + 1):
        if not m.owned_rows[ty]:
            continue
        for tx in range(qx0 // 4, qx1 // 4 + 1):
            cols = sum(1 << (c - 4 * tx) for c in range(max(qx0, 4 * tx), min(qx1, 4 * tx + 3) + 1))     # blocks of one row
            mask = sum(cols << 4 * (r - 4 * ty) for r in range(max(qy0, 4 * ty), min(qy1, 4 * ty + 3) + 1))
            out.append((ty * m.tiles_x + tx, mask))
    return out


def pairs(m):
    """the expected pair set {(tile, triangle, mask)}"""
    return {(t, i, mk) for i in np.flatnonzero(m.has_pairs) for t, mk in triangle_tiles(m, int(i))}


def mask_pixels(m, i):
    """bool [H, W]: the pixels of the blocks that triangle i's masks name"""
    px = np.zeros((m.H, m.W), bool)
    for t, mk in triangle_tiles(m, i):
        ty, tx = divmod(t, m.tiles_x)
        for b in range(16):
            if mk >> b & 1:
                y, x = ty * TILE + (b // 4) * BLOCK, tx * TILE + (b % 4) * BLOCK
                px[y:y + BLOCK, x:x + BLOCK] = True
    return px


def flush_clip(case, draws=None):
    draws = [d for d in (case["draws"] if draws is None else draws) if len(d[2])]
    return np.concatenate([np.asarray(d[2], np.float64).reshape(-1, 12) for d in draws]) if draws else np.zeros((0, 12))


def single_triangle_depths(case, m, which=None):
    """For each triangle i of `which` (default: all accepted), drawn ALONE by the CPU oracle on a frame cleared to +inf: yields
    (i, ys, xs, z), the pixels it writes and exactly the depths our_gl.cpp:156-158 gives them.  The frame is searched in a
    window around the model's bbox; the oracle's fragment counter proves that nothing was written outside it."""
    from oracle import orc
    clip = m.clip
    o = orc.Oracle(m.W, m.H, 3, viewport=case["viewport"], z_clear=np.inf)
    for i in (np.flatnonzero(m.accepted) if which is None else which):
        i = int(i)
        before = o.stats[1]
        o.draw(orc.FLAT, clip[i:i + 1])
        n = o.stats[1] - before
        if m.accepted[i]:
            y0, y1, x0, x1 = max(int(m.by0[i]) - 2, 0), int(m.by1[i]) + 3, max(int(m.bx0[i]) - 2, 0), int(m.bx1[i]) + 3
        else:
            y0, y1, x0, x1 = 0, m.H, 0, m.W
        win = o.z[y0:y1, x0:x1]
        ys, xs = np.nonzero(np.isfinite(win))
        assert len(ys) == n, f"triangle {i}: the oracle wrote {n} pixels, {len(ys)} of them around the model's bbox"
        z = win[ys, xs].copy()
        win[ys, xs] = np.inf
        yield i, ys + y0, xs + x0, z
