"""Mipmapped textures of include/trgl.h ("Mipmapped textures") in plain Python and numpy, written from the header's definitions: the
yardstick of test_mip.py and test_mip_gpu.py.  Integer arithmetic is exact and every fp64 operation is one IEEE operation in the
written order (numpy float64 scalars: no contraction, no libm but floor), so every comparison against it is bit for bit.  Nothing here
is shared with the library's code.
"""
import struct

import numpy as np

MAX_LEVELS = 16
F = np.float64


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def num_levels(w, h):
    return 1 + int(max(w, h)).bit_length() - 1


def layout(w, h, bpp):
    """(widths, heights, offsets, total): offsets[l] of level l >= 1 in the packed buffer (offsets[0] = 0 names nothing)."""
    ws, hs = [w], [h]
    while max(ws[-1], hs[-1]) > 1:
        ws.append(max(1, ws[-1] // 2))
        hs.append(max(1, hs[-1] // 2))
    assert len(ws) == num_levels(w, h) <= MAX_LEVELS
    offs, o = [0], 0
    for l in range(1, len(ws)):
        offs.append(o)
        o += (ws[l] * hs[l] * bpp + 15) // 16 * 16
    return ws, hs, offs, o


def next_level(img):
    h, w, bpp = img.shape
    fx, fy = (2 if w >= 2 else 1), (2 if h >= 2 else 1)
    w2, h2 = max(1, w // 2), max(1, h // 2)
    blocks = img[:h2 * fy, :w2 * fx].astype(np.uint32).reshape(h2, fy, w2, fx, bpp)
    return ((blocks.sum(axis=(1, 3)) + (fx * fy) // 2) // (fx * fy)).astype(np.uint8)


def chain(img):
    """[level 0, level 1, ..., level L-1] of img [h, w, bpp] uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    levels = [img]
    while max(levels[-1].shape[:2]) > 1:
        levels.append(next_level(levels[-1]))
    return levels


def pack(levels, fill=0):
    """The packed buffer of levels 1 .. L-1, the padding between them holding `fill`."""
    h, w, bpp = levels[0].shape
    _, _, offs, total = layout(w, h, bpp)
    buf = np.full(total, fill, np.uint8)
    for l in range(1, len(levels)):
        buf[offs[l]:offs[l] + levels[l].size] = levels[l].reshape(-1)
    return buf


def level_mask(w, h, bpp):
    """True at the bytes of the packed buffer that belong to a level."""
    ws, hs, offs, total = layout(w, h, bpp)
    m = np.zeros(total, bool)
    for l in range(1, len(ws)):
        m[offs[l]:offs[l] + ws[l] * hs[l] * bpp] = True
    return m


# ---- samplers ----------------------------------------------------------------------------------------------------------------------
def cvttsd2si(d):
    d = float(d)
    if not (-2147483649.0 < d < 2147483648.0):
        return -2 ** 31
    return int(d)


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _texel(lv, x, y):
    out = [0, 0, 0, 0]
    out[:lv.shape[2]] = [int(v) for v in lv[y, x]]
    return out


def sample_level(levels, uv, level):
    lv = levels[clamp(int(level), 0, len(levels) - 1)]
    h, w, bpp = lv.shape
    with np.errstate(all="ignore"):
        x = clamp(cvttsd2si(F(uv[0]) * F(w)), 0, w - 1)
        y = clamp(cvttsd2si(F(uv[1]) * F(h)), 0, h - 1)
    return _texel(lv, x, y) + [bpp]


def _axis(t, size):
    with np.errstate(all="ignore"):
        u = F(t) * F(size) - F(0.5)
        if not (u >= -1.0):
            u = F(-1.0)
        if u > F(size):
            u = F(size)
        fl = np.floor(u)
        x0 = int(fl)
        f = int((u - fl) * F(256.0))
    return clamp(x0, 0, size - 1), clamp(x0 + 1, 0, size - 1), f


def sample_linear(levels, uv, level):
    lv = levels[clamp(int(level), 0, len(levels) - 1)]
    h, w, bpp = lv.shape
    xa, xb, fx = _axis(uv[0], w)
    ya, yb, fy = _axis(uv[1], h)
    caa, cba, cab, cbb = _texel(lv, xa, ya), _texel(lv, xb, ya), _texel(lv, xa, yb), _texel(lv, xb, yb)
    out = []
    for c in range(4):
        top = caa[c] * (256 - fx) + cba[c] * fx
        bot = cab[c] * (256 - fx) + cbb[c] * fx
        out.append((top * (256 - fy) + bot * fy + 32768) >> 16)
    return out + [bpp]


def sample_trilinear(levels, uv, lod):
    L = len(levels)
    lam = F(lod)
    if not (lam > 0.0):
        lam = F(0.0)
    if lam > F(L - 1):
        lam = F(L - 1)
    l0 = int(lam)
    t = int((lam - F(l0)) * F(256.0))
    l1 = min(l0 + 1, L - 1)
    a = sample_linear(levels, uv, l0)
    if t == 0:
        return a
    b = sample_linear(levels, uv, l1)
    return [(a[c] * (256 - t) + b[c] * t + 128) >> 8 for c in range(4)] + [a[4]]


def sample(levels, uv, lod, mode):
    """[n, 5] uint8 over uv [n, 2] and lod [n]; mode 0 level, 1 linear, 2 trilinear (0 and 1: lod converted to int as cvttsd2si does)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    lod = np.broadcast_to(np.asarray(lod, np.float64), (uv.shape[0],))
    out = np.zeros((uv.shape[0], 5), np.uint8)
    for i in range(uv.shape[0]):
        if mode == 2:
            out[i] = sample_trilinear(levels, uv[i], lod[i])
        elif mode == 1:
            out[i] = sample_linear(levels, uv[i], cvttsd2si(lod[i]))
        else:
            out[i] = sample_level(levels, uv[i], cvttsd2si(lod[i]))
    return out


# ---- level of detail ---------------------------------------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def mip_lod(bar, k, tex_w, tex_h):
    bar = [F(v) for v in bar]
    k = [F(v) for v in k]
    with np.errstate(all="ignore"):
        wp = (bar[0] * k[1] + bar[1] * k[2]) + bar[2] * k[3]
        r = (((k[0] * wp) * wp) * wp) * (F(tex_w) * F(tex_h))
    if not (r > 1.0):
        return 0.0
    if np.isinf(r):
        return 64.0
    b = bits(r)
    e = ((b >> 52) & 0x7ff) - 1023
    m = F(b & ((1 << 52) - 1)) * F(2.0 ** -52)
    return float(F(0.5) * (F(e) + m))


def lod_constants(viewport, clip, uv):
    """(c, W0, W1, W2) of one triangle: viewport 16 doubles, clip 12 doubles, uv = u0 v0 u1 v1 u2 v2."""
    vp = [F(v) for v in np.asarray(viewport, np.float64).reshape(16)]
    c = [F(v) for v in np.asarray(clip, np.float64).reshape(12)]
    uv = [F(v) for v in np.asarray(uv, np.float64).reshape(6)]
    zero = (0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        W = [c[3], c[7], c[11]]
        ok = all(w > 1e-12 for w in W)
        s, q, U, V = [], [], [], []
        for i in range(3):
            ndc = [c[4 * i + k] / W[i] for k in range(4)]
            sx, sy = F(0.0), F(0.0)
            for k in range(4):
                sx = sx + vp[k] * ndc[k]
                sy = sy + vp[4 + k] * ndc[k]
            ok = ok and all(np.isfinite(v) for v in ndc) and bool(np.isfinite(sx)) and bool(np.isfinite(sy))
            s.append((sx, sy))
            q.append(F(1.0) / W[i])
            U.append(uv[2 * i] * q[i])
            V.append(uv[2 * i + 1] * q[i])
        if not ok:
            return zero
        e1x, e1y = s[1][0] - s[0][0], s[1][1] - s[0][1]
        e2x, e2y = s[2][0] - s[0][0], s[2][1] - s[0][1]
        A = e1x * e2y - e1y * e2x
        if A == 0:
            return zero

        def grad(f):
            d1, d2 = f[1] - f[0], f[2] - f[0]
            return d1 * e2y - d2 * e1y, d2 * e1x - d1 * e2x
        gxU, gyU = grad(U)
        gxV, gyV = grad(V)
        gxq, gyq = grad(q)
        N = (U[0] * (gxV * gyq - gyV * gxq) - V[0] * (gxU * gyq - gyU * gxq)) + q[0] * (gxU * gyV - gyU * gxV)
        cc = np.abs(N) / (A * A)
        if not np.isfinite(cc):
            return zero
    return (float(cc), float(W[0]), float(W[1]), float(W[2]))


def lod_stage(viewport, clip, vary, uv_offset, out_offset):
    """A copy of vary [n, K] with the four doubles of every row rewritten."""
    clip = np.asarray(clip, np.float64).reshape(-1, 12)
    out = np.array(vary, np.float64)
    for t in range(clip.shape[0]):
        out[t, out_offset:out_offset + 4] = lod_constants(viewport, clip[t], out[t, uv_offset:uv_offset + 6])
    return out
