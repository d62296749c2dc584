"""GPU tests of the stages in front of k_raster, on their own outputs: the setup records, the per-triangle tile counts and boxes,
the sorted (tile, triangle, mask) pair lists and the tile bounds of one flush, read back with Context.debug_snapshot() and held
against tests/binning_model.py (plain numpy from our_gl.cpp:89-141 and DESIGN.md section 3).

A frame cannot see most errors of these stages: a duplicated or foreign pair, a block mask or tile range that is too wide, a
depth bound that says nothing, a literal bit that is always set only cost time, and a depth bound that is too tight shows only
when a scene happens to land inside it.  Every comparison here is exact (bits, integers) or a one-sided inequality against the
CPU oracle's own depths; failure messages name the triangle or the tile and list entry.
"""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import binning_model as bm
import cases
from test_gpu_parity import extreme_depths_scene, large_triangles_scene
from test_raster_paths import LH, LW, _tile_lists_scene, literal_scene, setup_literal
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import DBG_INFO, DBG_INFO_FIELDS, DL_LITERAL, FLAT, GOURAUD, Context, TrglError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FIELDS = ("ax", "ay", "s0x", "s0y", "s1x", "s1y", "uz", "z0", "z1", "z2")       # defined by the reference, bit for bit
EXPAND_STAGE, SETUP_BLOCK, SMALL_TILES, RADIX_BIG_CAP = 3072, 256, 8, 4 << 20      # kernels_bin.hip


def _flat(W, H, clip, col=None, **kw):
    if col is None:
        col = np.arange(len(clip), dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0xFF000000)
    return cases.make_case(W, H, [(FLAT, None, clip, None, col)], **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _zq_of_tilebox(tb):
    return ((tb[:, 0] >> 13) & 7) | (((tb[:, 1] >> 13) & 7) << 3) | ((tb[:, 1] >> 29) << 6)


def submit(ctx, case, strip=None, interleave=None, draws=None):
    """queue one flush of the case's draws on ctx (nothing is flushed)"""
    ctx.set_viewport(case["viewport"])
    if strip is not None:
        ctx.set_strip(*strip)
    if interleave is not None:
        ctx.set_interleave(*interleave)
    for slot, t in case["textures"].items():
        ctx.upload_texture(slot, t)
    for kind, u, clip, vary, col in (case["draws"] if draws is None else draws):
        ctx.draw(kind, clip, vary, col, u)


def snapshots(ctx):
    """flush_begin -> snapshot of the pending flush -> flush_end -> snapshot of the complete flush; both must agree.  Where the
    pending flush has more pairs than the pair buffers hold (flush_end will grow them and bin again) it has no lists yet: reading
    them is refused, and only the complete flush is returned."""
    ctx.flush_begin()
    head = dict(zip(DBG_INFO_FIELDS, (int(v) for v in ctx._debug_read(DBG_INFO, np.int64))))
    assert head["pending"] == 1
    pend = None
    if head["P"] <= head["capacity"]:
        pend = ctx.debug_snapshot()
    else:
        with pytest.raises(TrglError):
            ctx.debug_snapshot()
    ctx.flush_end()
    done = ctx.debug_snapshot()
    assert done["info"]["pending"] == 0
    N = done["info"]["N"]
    assert done["info"]["P"] == ctx.last_flush_info()["pairs"] and N == ctx.last_flush_info()["triangles"]
    assert done["info"]["capacity"] >= done["info"]["P"]
    for k, v in head.items():
        assert k in ("pending", "capacity", "side") or done["info"][k] == v, f"info[{k}]: {v} while pending, {done['info'][k]} after the flush"
    if pend is not None:
        assert pend["info"] == head and done["info"]["capacity"] == head["capacity"] and done["info"]["side"] == head["side"]
        live = done["cnt"] > 0
        for k in ("cnt", "tilebox", "vals", "bmask", "tile_start", "tile_end"):
            assert np.array_equal(pend[k], done[k]), f"{k} changed between the pending and the complete flush"
        assert pend["recs"][:N][live].tobytes() == done["recs"][:N][live].tobytes(), "records changed between the pending and the complete flush"
    return done


def check_setup(s, m, what=""):
    """RECS, CNT, TILEBOX, INFO against the model"""
    info, recs, cnt, tb = s["info"], s["recs"], s["cnt"], s["tilebox"]
    N = info["N"]
    assert N == m.N and len(cnt) == N and (N == 0 or len(recs) == N + 1), (what, N, m.N, len(cnt), len(recs))
    bad = np.flatnonzero(cnt != m.cnt)
    assert not len(bad), f"{what}: cnt of triangle {bad[0]} is {cnt[bad[0]]}, model {m.cnt[bad[0]]} ({len(bad)} differ)"
    assert int(cnt.sum()) == info["P"], (what, int(cnt.sum()), info["P"])
    live = np.flatnonzero(cnt > 0)
    r = recs[:N][live]
    for f in REF_FIELDS:
        bad = np.flatnonzero(_bits(r[f]) != _bits(getattr(m, f)[live]))
        assert not len(bad), f"{what}: {f} of triangle {live[bad[0]]} is {r[f][bad[0]]!r}, model {getattr(m, f)[live][bad[0]]!r} ({len(bad)} differ)"
    for f in ("bx0", "by0", "bx1", "by1"):
        bad = np.flatnonzero(r[f] != getattr(m, f)[live])
        assert not len(bad), f"{what}: {f} of triangle {live[bad[0]]} is {r[f][bad[0]]}, model {getattr(m, f)[live][bad[0]]}"
    bad = np.flatnonzero(r["color"] != m.color[live])
    assert not len(bad), f"{what}: colour of triangle {live[bad[0]]}"
    lit = (r["dl"] & DL_LITERAL) != 0
    bad = np.flatnonzero(lit != m.literal[live])
    assert not len(bad), f"{what}: TRGL_DL_LITERAL of triangle {live[bad[0]]} is {lit[bad[0]]}, model {m.literal[live][bad[0]]} ({len(bad)} differ)"
    want_dl = (m.draw[live] << 24) | m.local[live]
    bad = np.flatnonzero((r["dl"] & 0x7fffffff) != want_dl)
    assert not len(bad), f"{what}: dl of triangle {live[bad[0]]} is {r['dl'][bad[0]]:#x}, want draw {m.draw[live][bad[0]]} local {m.local[live][bad[0]]}"
    with np.errstate(all="ignore"):
        want_ruz = np.where(m.literal[live], 0.0, 1.0 / m.uz[live])
    bad = np.flatnonzero(_bits(r["ruz"]) != _bits(want_ruz))
    assert not len(bad), f"{what}: ruz of triangle {live[bad[0]]} is {r['ruz'][bad[0]]!r}, want {want_ruz[bad[0]]!r} ({len(bad)} differ)"
    # a plane that is switched off is switched off entirely; a literal triangle has none
    off = np.isneginf(r["c0"])
    assert ((r["g1"][off] == 0) & (r["g2"][off] == 0)).all() and off[lit].all(), f"{what}: plane of a literal triangle / half a plane"
    assert not np.isnan(r["c0"]).any() and not np.isposinf(r["c0"]).any()
    # the box in block units that k_expand walks = (bbox n strip) of the model
    box = np.stack([tb[live, 0] & 0x1fff, (tb[live, 0] >> 16) & 0x1fff, tb[live, 1] & 0x1fff, (tb[live, 1] >> 16) & 0x1fff], 1)
    want = np.stack([m.bx0[live] >> 3, m.ylo[live] >> 3, m.bx1[live] >> 3, m.yhi[live] >> 3], 1)
    bad = np.flatnonzero((box != want).any(1))
    assert not len(bad), f"{what}: block box of triangle {live[bad[0]]} is {box[bad[0]]}, model {want[bad[0]]}"
    assert (_zq_of_tilebox(tb[live])[np.isneginf(r["c0"])] == 0).all(), f"{what}: a depth bound without a plane"
    assert info["literal_tris"] == int(m.literal.sum()), (what, info["literal_tris"], int(m.literal.sum()))
    assert info["large_tris"] == int(m.large.sum()), (what, info["large_tris"], int(m.large.sum()))
    assert info["zq_cull"] == int(m.large.any()) and info["wide"] == int(m.tiles_x * m.tiles_y > 65536)
    assert (info["W"], info["H"], info["tiles_x"], info["tiles_y"]) == (m.W, m.H, m.tiles_x, m.tiles_y)
    if N and not info["pending"] and m.owned_rows.any():     # (k_make_items writes it; a context without tile rows launches no raster)
        p = recs[N]
        assert p["c0"] == np.inf and p["uz"] == 1.0 and p["bx0"] > p["bx1"] and p["by0"] > p["by1"], f"{what}: partner record {p}"


def check_pairs(s, m, what=""):
    """VALS, BMASK, TILE_START, TILE_END against the model's pair set"""
    info, vals, bmask, ts, te = s["info"], s["vals"], s["bmask"], s["tile_start"].astype(np.int64), s["tile_end"].astype(np.int64)
    P, T = info["P"], m.tiles_x * m.tiles_y
    assert len(ts) == T and len(te) == T and len(vals) == P and len(bmask) == P, (what, len(ts), T, len(vals), P)
    full = np.flatnonzero(te > ts)
    bad = full[(ts[full] < 0) | (te[full] > P)]
    assert not len(bad), f"{what}: slice [{ts[bad[0]]}, {te[bad[0]]}) of tile {bad[0]} is not inside [0, {P})"
    order = full[np.argsort(ts[full], kind="stable")]
    gap = np.flatnonzero(ts[order][1:] < te[order][:-1])
    assert not len(gap), f"{what}: slices of tiles {order[gap[0]]} and {order[gap[0] + 1]} overlap"
    assert int((te[full] - ts[full]).sum()) == P, f"{what}: slice lengths sum to {int((te[full] - ts[full]).sum())}, P = {P}"
    foreign = full[~m.owned_rows[full // m.tiles_x]]
    assert not len(foreign), f"{what}: tile {foreign[0]} of a row this context does not own has a list"
    # (inside [0, P), disjoint and P long in sum: the slices tile [0, P) in the order of their starts)
    tile_of = np.repeat(order, te[order] - ts[order])
    tri, zq = (vals & 0x1ffffff).astype(np.int64), vals >> 25
    bad = np.flatnonzero(tri >= m.N)
    assert not len(bad), f"{what}: entry {bad[0]} (tile {tile_of[bad[0]]}) names triangle {tri[bad[0]]} of {m.N}"
    bad = np.flatnonzero((tile_of[1:] == tile_of[:-1]) & (tri[1:] <= tri[:-1]))
    assert not len(bad), (f"{what}: tile {tile_of[bad[0]]}: entries {bad[0] - ts[tile_of[bad[0]]]} and the next hold triangles "
                          f"{tri[bad[0]]}, {tri[bad[0] + 1]} - not strictly increasing")
    got = {(int(t), int(i), int(k)) for t, i, k in zip(tile_of, tri, bmask)}
    want = bm.pairs(m)
    miss, extra = sorted(want - got)[:3], sorted(got - want)[:3]
    assert got == want, f"{what}: (tile, triangle, mask) missing {[(t, i, hex(k)) for t, i, k in miss]}, not expected {[(t, i, hex(k)) for t, i, k in extra]}"
    assert len(got) == P
    bad = np.flatnonzero(zq != _zq_of_tilebox(s["tilebox"])[tri])
    assert not len(bad), f"{what}: entry {bad[0]} of triangle {tri[bad[0]]} carries zq {zq[bad[0]]}, its tilebox {_zq_of_tilebox(s['tilebox'])[tri[bad[0]]]}"


def flush_and_check(case, strip=None, interleave=None, frame=True, ctx=None, what=""):
    """one flush of the case in halves with a snapshot in between; records, lists and (frame=True) the frame are checked"""
    m = bm.model(case, strip=strip, interleave=interleave)
    own = ctx is None
    ctx = ctx or Context(case["width"], case["height"], case["bpp"])
    try:
        if own:
            ctx.clear(case["clear"], case["zclear"])
        submit(ctx, case, strip, interleave)
        s = snapshots(ctx)
        check_setup(s, m, what)
        check_pairs(s, m, what)
        if frame:
            got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats())
            rows = strip if interleave is None else [(32 * int(ty), min(32 * int(ty) + 32, m.H)) for ty in np.flatnonzero(m.owned_rows)]
            cases.assert_same_frame(got, cases.run_oracle(case, strip=strip if interleave is None else None), rows=rows,
                                    eye=cases.has_eye(case), stats=own and interleave is None, what=what + " frame after the snapshot")
    finally:
        if own:
            ctx.close()
    return s, m


# ---- setup records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_setup_records_of_every_case(name):
    """Every case of cases.CASES in one flush: counts, records, boxes and INFO equal the model; no triangle goes literal."""
    case = cases.CASES[name]()
    with Context(case["width"], case["height"], case["bpp"]) as ctx:
        ctx.clear(case["clear"], case["zclear"])
        submit(ctx, case)
        s = snapshots(ctx)
    check_setup(s, bm.model(case), name)
    assert s["info"]["literal_tris"] == 0


@pytest.mark.parametrize("seed", [3100, 3101, 3102])
def test_literal_decision_is_the_models_and_covers_setup_literal(seed):
    """What k_setup decided, read back: the literal bit equals the model's predicate on every row, and every row that
    setup_literal (the prediction with margins of test_raster_paths.py) marks and that has pairs carries it."""
    clip, col, rows, cls = literal_scene(seed)
    case = _flat(LW, LH, clip, col, viewport=cases.UNIT_VIEWPORT)
    s, m = flush_and_check(case, what=f"literal scene {seed}")
    lit = setup_literal(clip, cases.UNIT_VIEWPORT, LW, LH)[0]
    bit = (s["recs"][:m.N]["dl"] & DL_LITERAL) != 0
    marked = np.flatnonzero(lit & (s["cnt"] > 0))
    assert len(marked) >= 150, len(marked)
    assert bit[marked].all(), f"row {marked[~bit[marked]][0]} is literal by a margin but carries no TRGL_DL_LITERAL"
    assert not lit[(s["cnt"] > 0) & ~bit].any()
    assert s["info"]["literal_tris"] == int(bit[s["cnt"] > 0].sum()) >= len(marked)


# ---- depth bounds ----------------------------------------------------------------------------------------------------
def _plane_exact(ax, ay, g1, g2, c0, xc, yc):
    """fma(ax - xc, g1, fma(ay - yc, g2, c0)) with each FMA rounded once (Fraction is exact, float() rounds correctly)"""
    inner = float(Fraction(ay - yc) * Fraction(g2) + Fraction(c0))
    return float(Fraction(ax - xc) * Fraction(g1) + Fraction(inner))


def check_depth_bounds(case, what, min_checked=None, min_zq=None):
    """The depth plane (c0, g1, g2) and the 7-bit bound zq of every triangle against the depths the CPU oracle computes for that
    triangle alone on a frame cleared to +inf: plane value as k_raster evaluates it <= depth at every covered pixel, and
    -1 + zq / 64 <= the smallest depth.  min_checked / min_zq: shares of the accepted triangles that must have a finite plane and
    a covered pixel / a bound zq >= 1 (None: some triangle, and the share is printed)."""
    m = bm.model(case)
    with Context(case["width"], case["height"], case["bpp"]) as ctx:
        submit(ctx, case)
        s = snapshots(ctx)
    check_setup(s, m, what)
    recs, zq = s["recs"], _zq_of_tilebox(s["tilebox"])
    vzq = s["vals"] >> 25
    tri = s["vals"] & 0x1ffffff
    assert np.array_equal(vzq, zq[tri]), f"{what}: a pair's zq differs from its triangle's"
    planes = bounds = exact = 0
    for i, ys, xs, z in bm.single_triangle_depths(case, m):
        if not len(ys):
            continue
        assert s["cnt"][i] > 0, f"{what}: triangle {i} covers {len(ys)} pixels and has no pairs"
        r = recs[i]
        if zq[i] >= 1:
            bounds += 1
            assert -1.0 + float(zq[i]) / 64.0 <= z.min(), f"{what}: triangle {i}: bound -1 + {zq[i]}/64 above its smallest depth {z.min()!r}"
        if not np.isfinite(r["c0"]):
            continue
        planes += 1
        ax, ay, g1, g2, c0 = (float(r[k]) for k in ("ax", "ay", "g1", "g2", "c0"))
        xc, yc = xs + 0.5, ys + 0.5
        # Sure cases first, in extended precision: the two FMAs round twice, each by at most half an ulp of a value bounded by the
        # sum of the |terms|; where the long-double value is further below the depth than 2^-40 of that sum, the exact one is too.
        a, b = np.longdouble(ax) - xc, np.longdouble(ay) - yc
        with np.errstate(all="ignore"):
            pl = a * np.longdouble(g1) + (b * np.longdouble(g2) + np.longdouble(c0))
            slack = (np.abs(a * g1) + np.abs(b * g2) + abs(np.longdouble(c0))) * np.longdouble(2.0 ** -40) + np.longdouble(1e-300)
            sure = pl + slack <= z
        for k in np.flatnonzero(~sure):
            exact += 1
            v = _plane_exact(ax, ay, g1, g2, c0, float(xc[k]), float(yc[k]))
            assert v <= z[k], f"{what}: triangle {i} pixel ({xs[k]}, {ys[k]}): plane value {v!r} above the depth {z[k]!r}"
    acc = int(m.accepted.sum())
    print(f"{what}: {acc} accepted, plane checked on {planes} ({planes / max(acc, 1):.1%}), zq >= 1 on {bounds} ({bounds / max(acc, 1):.1%}), "
          f"{exact} pixels through exact FMAs")
    if min_checked is None:
        assert planes > 0 and bounds > 0, (what, planes, bounds)
    else:
        assert planes >= min_checked * acc and bounds >= min_zq * acc, (what, acc, planes, bounds)
    return s, m


@pytest.mark.parametrize("persp", [False, True])
def test_depth_bounds_are_conservative_and_not_vacuous(persp):
    clip, col = scenes.random_triangles(2000, 128, 96, seed=5, rmin=1, rmax=40, perspective_w=persp)
    check_depth_bounds(_flat(128, 96, clip, col), f"random scene, perspective_w={persp}", min_checked=0.9, min_zq=0.5)


@pytest.mark.parametrize("seed", [0, 1])
def test_depth_bounds_on_extreme_depths(seed):
    """the scene of test_depth_plane_early_test_on_extreme_depths: part of its planes are switched off on purpose (k_setup's okp)"""
    W, H, clip, col, _ = extreme_depths_scene(seed)
    check_depth_bounds(_flat(W, H, clip[:5000], col[:5000]), f"extreme depths {seed}")


def test_depth_bounds_on_large_triangles():
    """the scene of test_depth_bound_in_the_pair_on_large_triangles (its second half: small triangles, then large ones)"""
    W, H, clip, col = large_triangles_scene(0)
    s, m = check_depth_bounds(_flat(W, H, clip[4000:6500], col[4000:6500]), "large triangles")
    assert s["info"]["large_tris"] > 0 and s["info"]["zq_cull"] == 1


def test_depth_bounds_on_huge_depths():
    check_depth_bounds(cases.CASES["huge_depths_128"](), "huge_depths_128")


# ---- pair lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat_small_64", "gouraud_256_rgba", "multi_draw_320x200", "odd_dims_101x67", "viewport_offset_256x160"])
def test_pair_lists_of_small_cases(name):
    case = cases.CASES[name]()
    s, m = flush_and_check(case, what=name)
    assert s["info"]["P"] > 0 and s["info"]["wide"] == 0
    if name == "multi_draw_320x200":
        assert len(case["draws"]) == 4 and len({d[0] for d in case["draws"]}) == 3 and m.draw.max() == 3


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 256 + 3])
def test_pair_lists_at_setup_block_edges(n):
    clip, col = scenes.random_triangles(n, 128, 96, seed=700 + n, rmin=2, rmax=40)
    s, m = flush_and_check(_flat(128, 96, clip, col), what=f"{n} triangles")
    assert s["info"]["N"] == n and s["info"]["P"] > 0


def test_pair_lists_of_several_draws_in_one_flush():
    """setup blocks are numbered across the draws of a flush: draws of 1, 255, 256, 257 and 515 triangles, two kinds"""
    W, H = 160, 128
    draws = []
    for k, n in enumerate((1, 255, 256, 257, 2 * 256 + 3)):
        clip, col = scenes.random_triangles(n, W, H, seed=720 + k, rmin=2, rmax=50, perspective_w=bool(k & 1))
        if k & 1:
            draws.append((GOURAUD, None, clip, scenes.SplitMix64(k).uniform(n * 3, 0.0, 1.0).reshape(n, 3), col))
        else:
            draws.append((FLAT, None, clip, None, col))
    s, m = flush_and_check(cases.make_case(W, H, draws), what="five draws")
    assert s["info"]["N"] == 1284 and m.draw.max() == 4 and (s["cnt"][m.draw == 4] > 0).any()


def test_pair_lists_small_and_wave_wide_triangles_staged_and_straight_out():
    """k_expand: triangles of <= 8 tiles (one thread each) and of more (the whole wave) in one block of 256, and a block whose
    pairs exceed EXPAND_STAGE (written straight out) between blocks that stay below it (staged in LDS)."""
    W = H = 256
    small, _ = scenes.random_triangles(640, W, H, seed=731, rmin=1, rmax=12)
    big, _ = scenes.random_triangles(128, W, H, seed=732, rmin=80, rmax=300)
    mid = np.empty((256, 12)); mid[0::2] = big; mid[1::2] = small[512:]
    clip = np.concatenate([small[:256], mid, small[256:512]])
    s, m = flush_and_check(_flat(W, H, clip), what="three setup blocks")
    per_block = s["cnt"].reshape(3, SETUP_BLOCK).sum(1)
    assert 0 < per_block[0] <= EXPAND_STAGE < per_block[1] and 0 < per_block[2] <= EXPAND_STAGE, per_block
    c = s["cnt"][SETUP_BLOCK:2 * SETUP_BLOCK]
    assert ((c > 0) & (c <= SMALL_TILES)).any() and (c > SMALL_TILES).any()


def _strip_scene():
    clip, col = scenes.random_triangles(3000, 192, 320, seed=741, rmin=2, rmax=60)
    return _flat(192, 320, clip, col)


@pytest.mark.parametrize("strip", [(37, 150), (3, 317), (100, 101)])
def test_pair_lists_of_a_strip_off_the_block_grid(strip):
    assert all(y % 8 and y % 32 for y in strip)
    s, m = flush_and_check(_strip_scene(), strip=strip, what=f"strip {strip}")
    assert (s["info"]["strip_y0"], s["info"]["strip_y1"], s["info"]["il_tiles"]) == (*strip, 0) and s["info"]["P"] > 0
    assert 0 < (s["cnt"] > 0).sum() < m.accepted.sum()


@pytest.mark.parametrize("il_tiles,world,rank", [(t, w, r) for t in (1, 2) for w in (2, 4) for r in range(w)])
def test_pair_lists_of_interleaved_bands(il_tiles, world, rank):
    s, m = flush_and_check(_strip_scene(), interleave=(32 * il_tiles, rank, world), what=f"bands of {il_tiles} tile rows, rank {rank} of {world}")
    assert (s["info"]["il_tiles"], s["info"]["il_world"], s["info"]["il_rank"]) == (il_tiles, world, rank) and s["info"]["P"] > 0
    assert m.owned_rows.any() and not m.owned_rows.all()


def test_pair_lists_with_wide_tile_keys():
    """more than 65536 tiles (8224 x 8224 = 257 x 257): 32-bit sort words and the masks in a stream of their own; few triangles,
    half of them in the last tile rows and columns (tile ids above 65535)"""
    W = H = 8224
    n = 600
    clip, col = scenes.random_triangles(n, W, H, seed=751, rmin=8, rmax=300)
    clip = clip.copy()
    clip[: n // 2, [0, 4, 8]] = clip[: n // 2, [0, 4, 8]] * 0.03 + 0.965 * clip[: n // 2, [3, 7, 11]]
    clip[: n // 2, [1, 5, 9]] = clip[: n // 2, [1, 5, 9]] * 0.03 + 0.965 * clip[: n // 2, [3, 7, 11]]
    s, m = flush_and_check(_flat(W, H, clip, col, bpp=1), frame=False, what="wide")
    assert s["info"]["wide"] == 1 and s["info"]["tiles_x"] * s["info"]["tiles_y"] > 65536
    assert max(t for t, _, _ in bm.pairs(m)) > 65535


def test_pair_lists_in_eight_wave_radix_blocks():
    """pair buffers of at least 4 M entries sort in radix blocks of 8 waves: a first flush of 2.1 M triangles (all rejected: w = 0)
    sizes the buffers at 2 pairs per triangle, the small flush behind it is read back.  That flush is NOT sorted from the segments:
    after a flush without pairs the automatic choice offers it segments of 192 slots, its blocks hold more, and it falls back - the
    8-wave kernels of the direct path do nothing here (tests/test_direct_pairs_big_gpu.py runs them)."""
    W, H = 256, 192
    clip, col = scenes.random_triangles(9000, W, H, seed=761, rmin=2, rmax=50)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, np.zeros((2_100_000, 12)))
        ctx.flush()
        assert ctx.debug_snapshot()["info"]["P"] == 0
        s, m = flush_and_check(_flat(W, H, clip, col), ctx=ctx, what="8-wave blocks")
    assert s["info"]["capacity"] >= RADIX_BIG_CAP and s["info"]["P"] > 8192, s["info"]
    assert (s["info"]["seg_S"], s["info"]["seg_G"], s["info"]["direct"], s["info"]["fell_back"]) == (192, 16, 1, 1), s["info"]
    assert np.add.reduceat(s["cnt"], np.arange(0, len(s["cnt"]), SETUP_BLOCK)).max() > 192


def test_pair_lists_after_the_buffers_grew():
    """a flush whose pairs exceed the capacity a small first flush left: the binning queued by flush_begin does nothing (the
    pending flush has no lists to read), flush_end grows the buffers and bins again"""
    W = H = 256
    small, cs = scenes.random_triangles(300, W, H, seed=771, rmin=1, rmax=6)
    big, cb = scenes.random_triangles(700, W, H, seed=772, rmin=40, rmax=300)
    case = _flat(W, H, big, cb)
    m = bm.model(case)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, small, colors=cs)
        ctx.flush()
        cap0 = ctx.debug_snapshot()["info"]["capacity"]
        submit(ctx, case)
        ctx.flush_begin()
        info = dict(zip(DBG_INFO_FIELDS, (int(v) for v in ctx._debug_read(DBG_INFO, np.int64))))
        assert info["capacity"] == cap0 < info["P"] == m.cnt.sum(), (info, cap0)
        with pytest.raises(TrglError):
            ctx.debug_snapshot()
        ctx.flush_end()
        s = ctx.debug_snapshot()
        assert s["info"]["capacity"] >= s["info"]["P"] > cap0
        check_setup(s, m, "grown")
        check_pairs(s, m, "grown")
        got = (ctx.read_framebuffer(), ctx.read_zbuffer())
    both = cases.make_case(W, H, [(FLAT, None, small, None, cs), (FLAT, None, big, None, cb)])
    cases.assert_same_frame(got, cases.run_oracle(both), stats=False, what="grown")


def test_short_lists_after_a_long_flush_and_a_clear_only_flush():
    """one context: a long flush, then short lists (stale words behind P in the pair buffers, stale bounds of the long flush), a
    flush that only clears, short lists again"""
    W = H = 256
    big, cb = scenes.random_triangles(400, W, H, seed=3800, rmin=80, rmax=300)
    with Context(W, H, 3) as ctx:
        s, _ = flush_and_check(_flat(W, H, big, cb), ctx=ctx, frame=False, what="long")
        long_P = s["info"]["P"]
        assert long_P > 10_000
        clip, col = _tile_lists_scene(W, H, 3801)
        ctx.clear()
        s, _ = flush_and_check(_flat(W, H, clip, col), ctx=ctx, what="short lists")
        assert 0 < s["info"]["P"] < long_P and s["info"]["capacity"] > long_P
        ctx.clear()
        ctx.flush()                             # a flush without triangles
        e = ctx.debug_snapshot()
        assert e["info"]["N"] == 0 and e["info"]["P"] == 0 and len(e["vals"]) == 0 and (e["tile_end"] <= e["tile_start"]).all()
        few, cf = scenes.random_triangles(7, W, H, seed=342, rmin=2, rmax=20)
        s, _ = flush_and_check(_flat(W, H, few, cf), ctx=ctx, what="few after the clear")
        assert 0 < s["info"]["P"] < 100
        with pytest.raises(TrglError):          # a draw ends the validity of the last flush's snapshot
            ctx.draw(FLAT, few, colors=cf)
            ctx.debug_snapshot()


# ---- the diagnostic build ----------------------------------------------------------------------------------------------
def test_no_list_entry_is_a_foreign_word_in_the_diagnostic_build():
    """test_short_tile_lists_after_a_large_frame's scenario against libtrgl_dbg.so, in one fresh child process: k_raster's count of
    list entries that are no triangle of the flush (DevStats::dbg[9], and dbg[10]: the first such candidate) stays 0 and the frames
    equal the oracle.  The guard against stale pair-buffer words reaching the visit loop."""
    lib = os.path.join(ROOT, "tinyrenderder_amd", "libtrgl_dbg.so")
    assert os.path.exists(lib), f"{lib} is missing: build() makes it"
    env = dict(os.environ, TRGL_LIB=lib)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-s", os.path.join(ROOT, "tests", "dbg_child_short_lists.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.strip().endswith("ok"), r.stdout
