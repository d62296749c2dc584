"""A numpy restatement of trgl_sprite_stage and trgl_line_stage (include/trgl.h, "point sprites and wide lines"): plain float64 scalar
expressions in the written order (numpy's + - * / and sqrt are IEEE), a stored NaN as 0x7FF8000000000000, attribute doubles as copies.
The yardstick of tests/test_sprites.py and tests/test_sprites_gpu.py; it shares no code with the library."""
import numpy as np

VIEW, SCREEN = 0, 1
F = np.float64
ZERO, HALF, ONE = F(0.0), F(0.5), F(1.0)
CANON_NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
TRIANGLES = ((0, 1, 2), (0, 2, 3))                     # corners of output triangle 2 i and 2 i + 1
SIGN_X, SIGN_Y = (-1, 1, 1, -1), (-1, -1, 1, 1)        # corner signs of k0 .. k3


def canon(x):
    return CANON_NAN if x != x else x


def matvec(m, v):
    """mat * vec of geometry.h:123-127: each row summed from 0.0 in component order."""
    return [(((ZERO + m[r][0] * v[0]) + m[r][1] * v[1]) + m[r][2] * v[2]) + m[r][3] * v[3] for r in range(4)]


def pm(sign, a, b):
    return a + b if sign > 0 else a - b


def _rows(corners, pairs, attr):
    """The two clip rows and the two varyings rows of a quad: corners 4 x 4, pairs 4 x 2."""
    clip = [[c for k in tri for c in corners[k]] for tri in TRIANGLES]
    vary = [[c for k in tri for c in pairs[k]] + list(attr) for tri in TRIANGLES]
    return clip, vary


def sprite_quad(P, row):
    mv, pr = np.asarray(P["model_view"], F).reshape(4, 4), np.asarray(P["projection"], F).reshape(4, 4)
    s = row[P["size_offset"]] if P["size_offset"] >= 0 else F(P["size"])
    e = matvec(mv, [row[0], row[1], row[2], ONE])
    h = HALF * s
    corners = []
    if P["mode"] == VIEW:
        for k in range(4):
            c = matvec(pr, [pm(SIGN_X[k], e[0], h), pm(SIGN_Y[k], e[1], h), e[2], e[3]])
            corners.append([canon(x) for x in c])
    else:
        c = matvec(pr, e)
        hx, hy = (h * F(P["scale"][0])) * c[3], (h * F(P["scale"][1])) * c[3]
        for k in range(4):
            corners.append([canon(pm(SIGN_X[k], c[0], hx)), canon(pm(SIGN_Y[k], c[1], hy)), canon(c[2]), canon(c[3])])
    pairs = [(ZERO, ZERO), (ONE, ZERO), (ONE, ONE), (ZERO, ONE)]
    a0 = P["attr_offset"]
    return _rows(corners, pairs, row[a0:a0 + P["n_attr"]] if P["n_attr"] else [])


def sprites(P, points, colors=None):
    """(clip [2 n, 12], varyings [2 n, 6 + n_attr], colours [2 n] or None)"""
    points = np.ascontiguousarray(points, F)
    n, K = points.shape[0], 6 + P["n_attr"]
    clip, vary = np.empty((2 * n, 12), F), np.empty((2 * n, K), F)
    with np.errstate(all="ignore"):
        for i in range(n):
            c, v = sprite_quad(P, points[i])
            clip[2 * i:2 * i + 2] = c
            # (the attribute doubles travel as integers: an assignment through float64 may quiet a signalling NaN)
            vary.view(np.uint64)[2 * i:2 * i + 2] = np.array(v, F).view(np.uint64)
    return clip, vary, None if colors is None else np.repeat(np.asarray(colors, np.uint32), 2)


ZERO_QUAD = ([[ZERO] * 12] * 2, [[ZERO] * 6] * 2)


def line_quad(P, pa, pb):
    """(clip rows, varyings rows), or None for the all-zero quad."""
    mv, pr = np.asarray(P["model_view"], F).reshape(4, 4), np.asarray(P["projection"], F).reshape(4, 4)
    w_min, he = F(P["w_min"]), (F(P["half_extent"][0]), F(P["half_extent"][1]))
    ca = matvec(pr, matvec(mv, [pa[0], pa[1], pa[2], ONE]))
    cb = matvec(pr, matvec(mv, [pb[0], pb[1], pb[2], ONE]))
    ta, tb = ZERO, ONE
    a_in, b_in = bool(ca[3] >= w_min), bool(cb[3] >= w_min)
    if not a_in and not b_in:
        return None
    if a_in != b_in:
        (cin, tin), (cout, tout) = ((ca, ta), (cb, tb)) if a_in else ((cb, tb), (ca, ta))
        d_in, d_out = cin[3] - w_min, cout[3] - w_min
        t = d_in / (d_in - d_out)
        cut = [cin[r] + t * (cout[r] - cin[r]) for r in range(4)]
        tcut = tin + t * (tout - tin)
        if a_in:
            cb, tb = cut, tcut
        else:
            ca, ta = cut, tcut
    ax, ay, bx, by = ca[0] / ca[3], ca[1] / ca[3], cb[0] / cb[3], cb[1] / cb[3]
    dx, dy = (bx - ax) * he[0], (by - ay) * he[1]
    length = np.sqrt(dx * dx + dy * dy)
    if not (length > ZERO and np.isfinite(length)):
        return None
    hw = HALF * F(P["width"])
    ox, oy = ((-dy / length) * hw) / he[0], ((dx / length) * hw) / he[1]
    corners, pairs = [], []
    for c, t, sign in ((ca, ta, -1), (cb, tb, -1), (cb, tb, 1), (ca, ta, 1)):          # A-, B-, B+, A+
        corners.append([canon(pm(sign, c[0], ox * c[3])), canon(pm(sign, c[1], oy * c[3])), canon(c[2]), canon(c[3])])
        pairs.append((canon(t), ONE if sign > 0 else ZERO))
    return _rows(corners, pairs, [])


def lines(P, points, indices=None, colors=None, n_segments=None):
    """(clip [2 n, 12], varyings [2 n, 6], colours [2 n] or None); an index that names no point gives the all-zero quad."""
    points = np.ascontiguousarray(points, F)
    if n_segments is None:
        n_segments = points.shape[0] // 2 if indices is None else len(indices) // 2
    n = n_segments
    clip, vary = np.zeros((2 * n, 12), F), np.zeros((2 * n, 6), F)
    col = None if colors is None else np.zeros(2 * n, np.uint32)
    with np.errstate(all="ignore"):
        for j in range(n):
            ia, ib = (2 * j, 2 * j + 1) if indices is None else (int(indices[2 * j]), int(indices[2 * j + 1]))
            q = line_quad(P, points[ia], points[ib]) if ia < points.shape[0] and ib < points.shape[0] else None
            if q is None:
                continue
            clip[2 * j:2 * j + 2], vary[2 * j:2 * j + 2] = q
            if col is not None:
                col[2 * j:2 * j + 2] = colors[j]
    return clip, vary, col


def cross_products(clip, viewport):
    """cross_product of our_gl.cpp:117-127 for every row of clip [n, 12] (NaN where rasterize() has returned before that line)."""
    vp = np.asarray(viewport, F).reshape(4, 4)
    out = np.full(clip.shape[0], np.nan)
    with np.errstate(all="ignore"):
        for i, row in enumerate(np.asarray(clip, F)):
            v = row.reshape(3, 4)
            if (v[:, 3] <= 1e-12).any() or not (v[:, 3] <= 1e-12).size:
                continue
            ndc = [[x / q[3] for x in q] for q in v]
            if not np.isfinite(np.array(ndc)).all():
                continue
            scr = [matvec(vp, q)[:2] for q in ndc]
            e1 = (scr[1][0] - scr[0][0], scr[1][1] - scr[0][1])
            e2 = (scr[2][0] - scr[0][0], scr[2][1] - scr[0][1])
            out[i] = e1[0] * e2[1] - e1[1] * e2[0]
    return out
