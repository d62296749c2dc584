"""Host model of the occlusion test (include/trgl.h, trgl_occlusion_boxes_image) in plain numpy fp64, written from the header's seven
steps: one product and one sum per operation in the order given (no `@` / `dot`, which may fuse or reorder), a brute-force scan of
every pixel of the rectangle for step 7.  Also the proxy of a box - its 12 faces in both windings, built from the very clip corners of
step 1 - which the tests push through the rasterizer to check what a code promises."""
import numpy as np

HIDDEN, VISIBLE, OUTSIDE, UNDECIDED = 0, 1, 2, 3
INT_MIN = -2147483648


def _dot4(m, p):
    s = 0.0 + m[0] * p[0]
    s = s + m[1] * p[1]
    s = s + m[2] * p[2]
    s = s + m[3] * p[3]
    return s


def _cast(a):
    """(int)double as the reference's x86-64 build executes it: NaN and out of range give INT_MIN"""
    ok = (a > -2147483649.0) & (a < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, a, 0.0)), float(INT_MIN)).astype(np.int64)


def clip_corners(view_proj, boxes):
    """Step 1: [n, 8, 4], corner k takes max.x for bit 0, max.y for bit 1, max.z for bit 2."""
    M = np.asarray(view_proj, np.float64).reshape(4, 4)
    b = np.asarray(boxes, np.float64).reshape(-1, 6)
    out = np.empty((len(b), 8, 4))
    for k in range(8):
        p = (b[:, 3] if k & 1 else b[:, 0], b[:, 4] if k & 2 else b[:, 1], b[:, 5] if k & 4 else b[:, 2], np.ones(len(b)))
        for r in range(4):
            out[:, k, r] = _dot4(M[r], p)
    return out


class Result:
    """codes [n] uint8; clip [n, 8, 4]; rect [n, 4] = x0, x1, y0, y1 and zq [n], meaningful where step 7 was reached (scanned)."""


def classify(depth, viewport, view_proj, boxes):
    depth = np.asarray(depth, np.float64)
    h, w = depth.shape
    V = np.asarray(viewport, np.float64).reshape(4, 4)
    res = Result()
    clip = res.clip = clip_corners(view_proj, boxes)
    n = len(clip)
    with np.errstate(all="ignore"):
        undecided = ~(clip[:, :, 3] > 1e-12).all(1)                                                 # step 2
        ndc = clip / clip[:, :, 3:4]                                                                # step 3
        undecided |= ~np.isfinite(ndc).all((1, 2))
        zmin, zmax = ndc[:, :, 2].min(1), ndc[:, :, 2].max(1)                                       # step 4
        outside = (zmin > 1.0) | (zmax < -1.0)
        comp = tuple(ndc[:, :, c] for c in range(4))
        sx, sy = _dot4(V[0], comp), _dot4(V[1], comp)                                               # step 5
        undecided |= np.isnan(sx).any(1) | np.isnan(sy).any(1)
        fx1, fy1 = np.ceil(sx.max(1)), np.ceil(sy.max(1))
        far = (fx1 >= 2147483648.0) | (fy1 >= 2147483648.0)
        x0, x1 = np.maximum(0, _cast(np.floor(sx.min(1)))), np.minimum(w - 1, _cast(fx1))
        y0, y1 = np.maximum(0, _cast(np.floor(sy.min(1)))), np.minimum(h - 1, _cast(fy1))
        empty = (x0 > x1) | (y0 > y1)
        Z = np.maximum(np.abs(zmin), np.abs(zmax))                                                  # step 6
        zq = zmin - np.ldexp(Z, -40)
    codes = np.full(n, UNDECIDED, np.uint8)
    decided = ~undecided
    codes[decided & outside] = OUTSIDE
    decided &= ~outside & ~far                                                                       # (far stays UNDECIDED)
    codes[decided & empty] = OUTSIDE
    res.scanned = decided & ~empty
    for i in np.nonzero(res.scanned)[0]:                                                             # step 7, every pixel
        window = depth[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
        codes[i] = VISIBLE if (zq[i] < window).any() else HIDDEN                                     # a NaN depth compares false
    res.codes, res.rect, res.zq = codes, np.stack([x0, x1, y0, y1], 1), zq
    return res


def codes(depth, viewport, view_proj, boxes):
    return classify(depth, viewport, view_proj, boxes).codes


# the faces of a box as cycles of corner numbers: per axis and side, the four corners that share that bit
_FACES = []
for _axis in range(3):
    _u, _v = [a for a in range(3) if a != _axis]
    for _side in (0, 1):
        _FACES.append([(_side << _axis) | (i << _u) | (j << _v) for i, j in ((0, 0), (1, 0), (1, 1), (0, 1))])


def proxy_triangles(clip8):
    """[24, 12]: the 12 triangles of the box with clip corners clip8 [8, 4], each in both windings."""
    tris = []
    for c in _FACES:
        for a, b, d in ((c[0], c[1], c[2]), (c[0], c[2], c[3])):
            tris.append(np.concatenate([clip8[a], clip8[b], clip8[d]]))
            tris.append(np.concatenate([clip8[a], clip8[d], clip8[b]]))
    return np.array(tris, np.float64)
