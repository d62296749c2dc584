"""Inputs shared by the triangle-order tests (test_triangle_order.py, test_triangle_order_gpu.py): clip rows whose w carry the values
where the depth expressions can go wrong, seeded rows for the gather, and the kinds of order lists."""
import numpy as np

from tinyrenderder_amd import scenes

DEPTH_GROUPS = (0, 1, 63, 64, 65, 257, 1000)          # G: below, at and above a wavefront and a block of 256, several blocks
DEPTH_GROUP_SIZES = (1, 2, 5)


def _from_bits(b):
    return np.array([b], np.uint64).view(np.float64)[0]


# +-0, +-inf, quiet and signalling NaNs of both signs with payloads, denormals of both signs, the largest doubles
SPECIAL_W = [0.0, -0.0, np.inf, -np.inf, _from_bits(0x7FF8000000000000), _from_bits(0xFFF8000000000000), _from_bits(0x7FF0000000000123),
             _from_bits(0xFFF4000000000456), 5e-324, -5e-324, 1.1125369292536007e-308, -1.1125369292536007e-308, 1.7976931348623157e308,
             -1.7976931348623157e308, _from_bits(0x7FFABCDEF0123456), _from_bits(0xFFF00000000000FF)]


def planted_clip(G, g, seed=1):
    """clip [G * g, 12] with random coordinates and w in (-2, 2), and planted among the w: every value of SPECIAL_W in slot 0 and in later
    slots, two specials in one group (+inf with -inf and a NaN behind another NaN among them), groups that hold only zeros of
    alternating sign (the earlier one stays), and equal values in different slots that are the group's smallest or largest."""
    n, per = G * g, 3 * g
    clip = scenes.SplitMix64(seed).uniform(max(n, 1) * 12, -2.0, 2.0).reshape(-1, 12)[:n].copy()
    w = clip.reshape(-1, 4)[:, 3].reshape(G, per) if G else np.zeros((0, per))
    ns = len(SPECIAL_W)
    for q in range(G):
        kind = q % (ns + 4)
        slot = (q // (ns + 4)) % per                                  # slot 0 first, then the later ones
        if kind < ns:
            w[q, slot] = SPECIAL_W[kind]
            if q % 3 == 1:                                            # a second special behind or in front of it
                w[q, (slot + 1) % per] = SPECIAL_W[(kind + 1 + q // 3) % ns]
        if q % 11 == 5:
            w[q] = [0.0 if (v + q) % 2 else -0.0 for v in range(per)]
        if q % 13 == 7:                                               # equal extremes in different slots
            w[q, 0] = w[q, per - 1] = 2.5 if q % 2 else -2.5
    if G:
        clip.reshape(-1, 4)[:, 3] = w.reshape(-1)
    return np.ascontiguousarray(clip)


GATHER_K = (0, 3, 5, 24, 64)
GATHER_GROUPS = (1, 2, 3)
GATHER_ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)    # n_order * g: around a wavefront, a block and the units a block moves
LISTS = ("identity", "reversed", "permutation", "repeats", "subset", "longer")


def gather_rows(n, K, colors, seed=3):
    """(clip [n, 12], vary [n, K] or None, colors [n] or None): random bit patterns - NaNs and infinities among the doubles."""
    r = scenes.SplitMix64(seed + 7 * K + n)
    clip = r.u64(max(n, 1) * 12).view(np.float64).reshape(-1, 12)[:n].copy()
    vary = r.u64(max(n, 1) * K).view(np.float64).reshape(-1, K)[:n].copy() if K else None
    col = (r.u64(max(n, 1)) >> np.uint64(32)).astype(np.uint32)[:n].copy() if colors else None
    return clip, vary, col


def order_list(kind, G, n_order, seed=5, out_of_range=False):
    """n_order uint32 entries over G groups; out_of_range: every fifth entry names no group (G, G + 1, 2^31, 2^32 - 1 among them)."""
    r = scenes.SplitMix64(seed + n_order)
    perm = np.argsort(r.u64(max(G, 1)), kind="stable")[:G]
    base = {"identity": np.arange(G), "reversed": np.arange(G)[::-1], "permutation": perm, "repeats": np.sort(perm)[::-1] // 2,
            "subset": perm[::2] if G > 1 else perm, "longer": np.concatenate([perm, perm[::-1], perm])}[kind]
    o = np.resize(base, n_order).astype(np.uint32)
    if out_of_range:
        bad = np.array([G, G + 1, 1 << 31, 0xFFFFFFFF, G + 12345], np.uint64).astype(np.uint32)
        o[::5] = np.resize(bad, o[::5].shape)
    return o


def list_plan():
    """(rows, group, list kind, n_order, G) for every row count: n_order * group = rows where group divides it, else the nearest below."""
    plan = []
    for i, rows in enumerate(GATHER_ROWS):
        for g in GATHER_GROUPS:
            n_order = max(rows // g, 1)
            kind = LISTS[(i + g) % len(LISTS)]
            G = {"identity": n_order, "reversed": n_order, "permutation": n_order, "repeats": max(n_order // 2, 1),
                 "subset": 2 * n_order, "longer": max(n_order // 3, 1)}[kind]
            plan.append((rows, g, kind, n_order, G))
    return plan
