"""Inputs shared by test_mip.py (host paths) and test_mip_gpu.py (device paths) of the mipmapped textures: sizes, textures, the uv and lod
lists of the filtered samplers, the triangles of the LOD stage.  Everything is seeded; the expected values come from mip_model.py."""
import numpy as np

BPPS = (1, 3, 4)
# 1x1 (one level), sides of 1, odd sides at several levels, one side far longer than the other, around a power of two
SIZES = [(1, 1), (2, 1), (1, 2), (3, 5), (1, 130), (130, 1), (257, 3), (63, 65), (64, 64), (65, 63)]


def texture(w, h, bpp, seed=0):
    return np.random.default_rng(1000 * w + 10 * h + bpp + seed).integers(0, 256, (h, w, bpp), dtype=np.uint8)


SAMPLE_TEXTURES = [(13, 7, 3), (8, 8, 4), (5, 1, 1), (1, 1, 4)]      # the last has L = 1


def sample_uv(w, h, levels):
    """uv [n, 2]: texel centres and texel boundaries of every level (each axis' list walked against the other's, so every position of
    either axis occurs), points a hair either side of them, and the values that must clamp: below 0, above 1, +-inf, NaN, +-1e300."""
    xs, ys = [], []
    for l in range(levels):
        wl, hl = max(1, w >> l), max(1, h >> l)
        xs += [i / wl for i in range(wl + 1)] + [(i + 0.5) / wl for i in range(wl)]
        ys += [i / hl for i in range(hl + 1)] + [(i + 0.5) / hl for i in range(hl)]
    n = max(len(xs), len(ys))
    pts = [(xs[i % len(xs)], ys[(3 * i + 1) % len(ys)]) for i in range(n)]
    pts += [(np.nextafter(x, -1.0), np.nextafter(y, 2.0)) for x, y in pts[:n // 2]]
    rng = np.random.default_rng(w * 100 + h)
    pts += [tuple(p) for p in rng.random((40, 2))]
    odd = [-0.25, -1e-9, 1.0, 1.0 + 1e-9, 1.75, np.inf, -np.inf, np.nan, 1e300, -1e300, -0.0, 0.0]
    pts += [(a, 0.37) for a in odd] + [(0.61, a) for a in odd] + [(a, a) for a in odd]
    return np.array(pts, np.float64)


def trilinear_lods(levels):
    """NaN, negative, fractional, exactly integral, the last level and above it, and fractions that make t = 0, 1 and 255."""
    top = levels - 1
    out = [np.nan, -np.inf, -3.0, -0.0, 0.0, 1.0 / 512, 1.0 / 256, 0.5, 255.0 / 256, 0.999999]
    out += [float(l) for l in range(levels)] + [l + 0.25 for l in range(levels)] + [top + 0.5, top + 4.0, 1e300, np.inf]
    return out


def level_lods(levels):
    """lod values for modes 0 and 1 (converted to int): every level, below 0, above L - 1, fractions that truncate, NaN, out of int range."""
    return [float(l) for l in range(-2, levels + 3)] + [0.99, 1.5, -0.5, np.nan, 1e300, -1e300, np.inf]


def viewport(w, h):
    """The Viewport of init_viewport(0, 0, w, h) (our_gl.cpp:59-69), row-major [4, 4]."""
    m = np.eye(4)
    m[0, 0], m[1, 1], m[0, 3], m[1, 3] = w / 2.0, h / 2.0, w / 2.0, h / 2.0
    return m


def lod_triangles(n, seed, perspective):
    """clip [n, 12] and uv [n, 6]: random triangles inside the clip volume, W = 1 or W in [0.5, 5]."""
    rng = np.random.default_rng(seed)
    clip = np.zeros((n, 3, 4))
    W = rng.uniform(0.5, 5.0, (n, 3)) if perspective else np.ones((n, 3))
    clip[..., :3] = rng.uniform(-1.0, 1.0, (n, 3, 3)) * W[..., None]
    clip[..., 3] = W
    return clip.reshape(n, 12), rng.uniform(-0.5, 2.0, (n, 6))


def lod_zeroing_cases():
    """clip [m, 12], uv [m, 6] and names: one triangle per case in which the stage must write four +0.0."""
    base, uv = lod_triangles(1, 77, True)
    rows, names = [], []

    def add(name, edit):
        r = base[0].copy().reshape(3, 4)
        edit(r)
        rows.append(r.reshape(12)); names.append(name)
    for v in range(3):
        add(f"W{v} = 1e-12", lambda r, v=v: r.__setitem__((v, 3), 1e-12))
    add("W = 0", lambda r: r.__setitem__((1, 3), 0.0))
    add("W < 0", lambda r: r.__setitem__((2, 3), -1.0))
    add("W = NaN", lambda r: r.__setitem__((0, 3), np.nan))
    add("W = inf (W / W is NaN)", lambda r: r.__setitem__((1, 3), np.inf))
    add("A = 0 (two equal vertices)", lambda r: r.__setitem__(1, r[0].copy()))
    add("A = 0 (collinear on a row)", lambda r: (r.__setitem__(0, [-0.5, 0.25, 0.0, 1.0]), r.__setitem__(1, [0.0, 0.25, 0.0, 1.0]), r.__setitem__(2, [0.5, 0.25, 0.0, 1.0])))
    add("X = inf", lambda r: r.__setitem__((2, 0), np.inf))
    add("X / W overflows", lambda r: (r.__setitem__((0, 0), 1e308), r.__setitem__((0, 3), 1e-10)))
    add("Z = NaN", lambda r: r.__setitem__((1, 2), np.nan))
    return np.array(rows), np.repeat(uv, len(rows), axis=0), names


def lod_rows(K, uv_offset, out_offset, clip, uv, seed):
    """vary [n, K] with uv at uv_offset and every other double a random bit pattern (NaNs and infinities among them)."""
    rng = np.random.default_rng(seed)
    vary = rng.integers(0, 2 ** 64, (clip.shape[0], K), dtype=np.uint64).view(np.float64).copy()
    vary[:, uv_offset:uv_offset + 6] = uv
    return vary


# (K, uv_offset, out_offset): the PHONG-like layout with the constants behind uv, and both ends of the largest row
LOD_LAYOUTS = [(10, 0, 6), (10, 4, 0), (64, 58, 0), (64, 0, 60), (24, 0, 20)]


def all_lod_cases():
    """(clip, uv) of every triangle the LOD tests use: affine, perspective, and the zeroing cases."""
    a = lod_triangles(40, 1, False)
    p = lod_triangles(60, 2, True)
    z = lod_zeroing_cases()
    return np.concatenate([a[0], p[0], z[0]]), np.concatenate([a[1], p[1], z[1]])
