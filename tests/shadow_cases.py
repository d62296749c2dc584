"""Inputs of the shadow post-pass that sit on its thresholds, shared by tests/test_shadow.py (host path, sanitizer program) and
tests/test_shadow_gpu.py (kernels).  A case is (name, depth [h, w], M [4, 4], zmap [map_h, map_w], bias, darkness, pcf_radius).

With M = I a pixel lands at s = (x + 0.5, y + 0.5, z), so the thresholds of steps 5-7 are hit exactly by choosing z; a last row
(0, 0, 0, k) sets q.w = k."""
import struct

import numpy as np

INF, NAN = np.inf, np.nan


def up(v):
    return np.nextafter(v, INF)


def down(v):
    return np.nextafter(v, -INF)


def _map(w, h, seed, holes=True):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (h, w))
    if holes:
        m[rng.random((h, w)) < 0.15] = INF
    return m


Z_RANGE_LIT = [False, True, False, False, True, False, False, True, True, True, False, False]
MAP_ENTRIES_R0 = [255, 0, 255, 255, 0, 255, 0, 0]       # +inf, -inf, NaN, limit, below it, above it, -0.0, 0.0 against limit = 0.25, darkness 1


def threshold_cases():
    I = np.eye(4)
    out = []
    # z at the ends of the depth range and the doubles either side, background values; the map lies below all of them, so a pixel that
    # is tested at all is darkened (Z_RANGE_LIT: which are not)
    zs = np.array([[1.0, up(1.0), down(1.0), -1.0, down(-1.0), up(-1.0), 0.0, INF, -INF, NAN, -0.0, 0.5]])
    zmap = np.full((1, 12), -2.0)
    for r in (0, 1):
        out.append((f"z_range_r{r}", zs, I, zmap, 1e-3, 0.6, r))
    # q.w at the guard and just above it: k * I keeps s = p where the guard lets the pixel through
    depth = np.full((3, 5), 0.25); depth[1, 2] = -0.75
    zmap = _map(5, 3, 1, holes=False)
    for name, k in (("w_at_guard", 1e-12), ("w_above_guard", up(1e-12)), ("w_zero", 0.0), ("w_negative", -1.0), ("w_two", 2.0)):
        out.append((name, depth, I * k, zmap, 0.0, 1.0, 0))
    # s.x forced to a value c by the row (0, 0, 0, c): 0.0, a sum that ends at +0.0, a quotient that underflows to -0.0, map_w and below
    map_w = 6
    zmap = _map(map_w, 4, 2, holes=False)
    depth = np.full((3, 2), 0.9)
    for name, c, k in (("sx_zero", 0.0, 1.0), ("sx_minus_zero_term", -0.0, 1.0), ("sx_underflows_to_minus_zero", -5e-324, 4.0),
                       ("sx_below_zero", -1e-300, 1.0), ("sx_map_w", float(map_w), 1.0), ("sx_below_map_w", down(float(map_w)), 1.0),
                       ("sy_map_h", None, 1.0)):
        M = np.eye(4) * k
        if c is None:
            M[1] = (0, 0, 0, 4.0)
        else:
            M[0] = (0, 0, 0, c)
        out.append((name, depth, M, zmap, 1e-3, 0.35, 1))
    # products that overflow in step 2: q.x = inf (s.x not finite), q.w = inf (s = 0 or NaN)
    depth = np.array([[1e300, 0.5, -1e300]])
    for name, (r, c) in (("overflow_qx", (0, 2)), ("overflow_qw", (3, 2)), ("overflow_qz", (2, 2))):
        M = np.eye(4); M[r, c] = 1e300
        out.append((name, depth, M, _map(4, 2, 3, holes=False) - 2.0, 0.0, 1.0, 1))
    M = np.eye(4); M[0, 0] = 1.7e308; M[3, 0] = 1.7e308           # from the second column on both products overflow: inf / inf
    out.append(("overflow_both", np.full((2, 3), 0.5), M, _map(4, 2, 3, holes=False) - 2.0, 0.0, 1.0, 0))
    # NaN in M
    depth = np.full((2, 4), 0.3)
    for r, c in ((0, 0), (3, 3), (2, 1), (1, 3)):
        M = np.eye(4); M[r, c] = NAN
        out.append((f"nan_in_M_{r}{c}", depth, M, _map(4, 2, 4, holes=False) - 2.0, 0.0, 1.0, 0))
    # map entries against limit = 0.5 - 0.25 = 0.25 exactly: equality does not occlude, +inf and NaN never do, -inf does
    zmap = np.array([[INF, -INF, NAN, 0.25, down(0.25), up(0.25), -0.0, 0.0]])
    depth = np.full((1, 8), 0.5)
    for r in (0, 1, 4):
        out.append((f"map_entries_r{r}", depth, I, zmap, 0.25, 1.0, r))
    return out


def corner_tap_cases():
    """Four pixels that land in the four corners of the map, for every PCF radius: most taps of each lie outside the map."""
    out = []
    for (map_w, map_h) in ((1, 1), (2, 3), (33, 20)):
        zmap = _map(map_w, map_h, 5, holes=False) - 0.5
        M = np.eye(4)
        M[0] = (map_w - 1, 0, 0, 0.25 - 0.5 * (map_w - 1))       # s.x = x * (map_w - 1) + 0.25
        M[1] = (0, map_h - 1, 0, 0.25 - 0.5 * (map_h - 1))
        for r in (0, 1, 4):
            for dk in (0.0, 0.35, 1.0):
                out.append((f"corners_{map_w}x{map_h}_r{r}_d{dk}", np.full((2, 2), 0.9), M, zmap, 1e-3, dk, r))
    return out


def random_case(w, h, map_w, map_h, r, darkness, seed):
    """A frame stretched over the map and a little beyond its edges; depths and map entries around each other, with background holes."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(-1.0, 1.0, (h, w))
    depth[rng.random((h, w)) < 0.2] = INF
    M = np.eye(4)
    M[0] = (1.1 * map_w / w, 0.05, 0, -0.05 * map_w)
    M[1] = (-0.03, 1.1 * map_h / h, 0, -0.04 * map_h)
    M[2] = (0, 0, 0.9, 0.05)
    M[3] = (0.001, 0.002, 0.1, 1.0)
    return (f"random_{w}x{h}_{map_w}x{map_h}_r{r}", depth, M, _map(map_w, map_h, seed + 1), 0.01, darkness, r)


def synthetic_image(w, h, bpp):
    i = np.arange(w * h * bpp, dtype=np.int64)
    return ((i * 7 + i // 251) & 255).astype(np.uint8).reshape(h, w, bpp)


def write_cases(path, cases):
    """The file tests/host/shadow_host.cpp reads: 'TRSHDW01', the count, then per case w, h, map_w, map_h, radius, 0 (int32), bias,
    darkness, M (float64), the depths and the map."""
    with open(path, "wb") as f:
        f.write(b"TRSHDW01" + struct.pack("<i", len(cases)))
        for _, depth, M, zmap, bias, darkness, r in cases:
            h, w = depth.shape
            mh, mw = zmap.shape
            f.write(struct.pack("<6i2d", w, h, mw, mh, r, 0, bias, darkness))
            f.write(np.ascontiguousarray(M, np.float64).tobytes())
            f.write(np.ascontiguousarray(depth, np.float64).tobytes())
            f.write(np.ascontiguousarray(zmap, np.float64).tobytes())


def demo_scene(W, H):
    """The floor and the occluder of examples/demo_shadow.cpp with its light and camera: the clip-space triangles of both passes
    (FLAT draws), the six matrices, and which triangles are the occluder's."""
    import math
    from tinyrenderder_amd import scenes
    quads = [([(-1.5, 0.0, 1.5), (1.5, 0.0, 1.5), (1.5, 0.0, -1.5), (-1.5, 0.0, -1.5)], (200, 190, 170)),
             ([(-0.8, 1.0, 0.8), (0.8, 1.0, 0.8), (0.8, 1.0, -0.8), (-0.8, 1.0, -0.8)], (60, 110, 220))]
    projs = dict(light=scenes.perspective(math.tan(50.0 * math.pi / 180.0 / 2.0), W / H, 1.0, 12.0),
                 cam=scenes.perspective(math.tan(60.0 * math.pi / 180.0 / 2.0), W / H, 1.0, 12.0))
    vp = scenes.init_viewport(0, 0, W, H)
    views = dict(light=scenes.lookat((2.7, 3.78, 2.7), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                 cam=scenes.lookat((0.0, 3.0, 3.6), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0)))
    out = dict(vp=vp, occluder=np.array([False, False, True, True]))
    colors = np.array([scenes.pack_bgra(b, g, r) for _, (r, g, b) in quads for _ in range(2)], np.uint32)
    for name, mv in views.items():
        clip = []
        for pts, _ in quads:
            for tri in ((0, 1, 2), (0, 2, 3)):
                row = []
                for v in tri:
                    eye = scenes._matvec(mv, *pts[v], 1.0)
                    row += scenes._matvec(projs[name], *eye)
                clip.append(row)
        out[name] = dict(mv=mv, proj=projs[name], clip=np.array(clip, np.float64), colors=colors)
    return out
