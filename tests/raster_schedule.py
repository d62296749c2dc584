"""A model of the schedule of k_raster's list loop (csrc/kernels_raster.hip, DESIGN.md "k_raster"), and scenes built to reach its
edges.  Plain Python, no GPU: tests/test_raster_schedule.py holds the model to hand-made lists and proves on binning_model's
lists that every scene reaches the edges it is meant for; tests/test_raster_schedule_gpu.py runs the same proof over the lists
the device itself built (Context.debug_snapshot()) and compares the frames with the CPU oracle.

What one wave (one 8x8 block, bit `kblk` of the pair masks) does with its tile's slice [beg, end) of the sorted pair list, as the
kernel's comments state it:

  steps    256 entries per step, 4 per lane, from beg & ~3 on; the lane's load address is clamped to the last group of four of the
           list, and entries outside [beg, end) are masked.  The entries with the block's bit are appended to a ring of 512 words in
           list order: position (head + cnt + rank) & 511.
  rounds   when 64 candidates wait, or on the last step any, a round of min(cnt, 64) is STARTED (its gather requested); a started
           round is TESTED in the next loop iteration that can start another round, or on the last step.  If neither holds the
           loop leaves with the request in flight, over as many steps as it takes.

replay() follows that bookkeeping and nothing else: it covers flushes with zq_cull == 0, where candidacy depends on the masks alone,
and it does not model what the cull decides or what a visit covers.
"""
import numpy as np

import binning_model as BM
import cases
from tinyrenderder_amd import scenes

STEP, PER_LANE, LANES, ROUND, RING = 256, 4, 64, 64, 512
EMPTY_START = 0xFFFFFFFF          # tile_start of a tile without pairs (its tile_end is 0)


# =====================================================================================================================
# the model
# =====================================================================================================================
class Wave:
    """The events of one wave.  steps: one dict per list step - p0, last, before / after (slots of the step outside [beg, end) on
    either side), before_bit / after_bit (how many of the words loaded for those slots carry the block's bit), tail_bit (the
    distinct list words behind `end` in its group of four that carry it), added, cnt_before, cnt_after, ring_positions (written:
    (head + cnt + rank) & 511), positions (the same before the mask), straddle (a lane whose own entries lie on both sides of a multiple of 512), in_flight_in
    (size of the round in flight when the step began), left_in_flight (the loop left with a request in flight).
    iters: one dict per loop iteration that did something - step, last, waiting, tested (size of the round tested, 0 = none),
    started (size of the round started, 0 = none).
    rounds: one dict per round - n, members (list positions of its candidates, in lane order), started_in_step, waiting (cnt when
    it was started), on_last, tested_in_step, idle_steps (steps that added nothing and left it in flight)."""

    def __init__(self, beg, end, kblk):
        self.beg, self.end, self.kblk = beg, end, kblk
        self.steps, self.iters, self.rounds = [], [], []
        self.total = 0                    # candidates appended
        self.max_occupancy = 0            # largest cnt
        self.max_position = -1            # largest unmasked ring position written: >= 512 k means the ring wrapped k times


def replay(beg, end, bmask, kblk, beyond=0xFFFF):
    """bmask: the pair buffer's mask words, indexed by list position (words behind its end read as `beyond`: by default every bit,
    what a stale word of an earlier flush may hold)."""
    bm = np.asarray(bmask)
    size = len(bm)
    bits = ((bm.astype(np.int64) >> kblk) & 1).tolist()
    far = (beyond >> kblk) & 1
    w = Wave(beg, end, kblk)
    if not beg < end:
        return w
    ring = [None] * RING
    head = cnt = 0
    flying = None                                       # the round whose gather is in flight
    last_group = (end - 1) - (end - 1) % PER_LANE
    w.tail_bit = sum(bits[q] if q < size else far for q in range(end, last_group + PER_LANE))
    p0 = beg - beg % PER_LANE
    while p0 < end:
        st = dict(p0=p0, last=p0 + STEP >= end, before=0, after=0, before_bit=0, after_bit=0, cnt_before=cnt, positions=[], ring_positions=[],
                  straddle=False, in_flight_in=flying["n"] if flying else 0, left_in_flight=False)
        for lane in range(LANES):
            at = p0 + PER_LANE * lane
            src = min(at, last_group)
            first = None
            for j in range(PER_LANE):
                q = at + j
                bit = bits[src + j] if src + j < size else far
                if q < beg:
                    st["before"] += 1; st["before_bit"] += bit
                elif q >= end:
                    st["after"] += 1; st["after_bit"] += bit
                elif bit:
                    pos = head + cnt
                    ring[pos % RING] = q
                    st["positions"].append(pos)
                    st["ring_positions"].append(pos % RING)
                    first = pos if first is None else first
                    if pos // RING != first // RING:
                        st["straddle"] = True
                    cnt += 1
                    assert cnt <= RING, "the ring overflowed"
        st["added"] = cnt - st["cnt_before"]
        st["cnt_after"] = cnt
        st["tail_bit"] = w.tail_bit if st["last"] else 0
        w.total += st["added"]
        w.max_occupancy = max(w.max_occupancy, cnt)
        if st["positions"]:
            w.max_position = st["positions"][-1]
        last = st["last"]
        while True:
            can = cnt >= ROUND or (last and cnt > 0)
            tested = None
            if flying is not None:
                if not can and not last:
                    st["left_in_flight"] = True
                    if st["added"] == 0:
                        flying["idle_steps"] += 1
                    break
                tested = flying
                tested["tested_in_step"] = len(w.steps)
            elif not can:
                break
            it = dict(step=len(w.steps), last=last, waiting=cnt, tested=tested["n"] if tested else 0, started=0)
            flying = None
            if can:
                n = min(cnt, ROUND)
                flying = dict(n=n, members=[ring[(head + l) % RING] for l in range(n)], started_in_step=len(w.steps), waiting=cnt,
                              on_last=last, tested_in_step=None, idle_steps=0)
                w.rounds.append(flying)
                it["started"] = n
                head += n; cnt -= n
            w.iters.append(it)
        w.steps.append(st)
        p0 += STEP
    assert flying is None and cnt == 0, "the list ended with candidates waiting or a round untested"
    return w


def round_schedule(added):
    """The rounds that follow from the candidates appended per step, by queue arithmetic alone (no loop over the kernel's
    iterations; tests hold replay() to it): [(n, started_in_step, tested_in_step, idle_steps)].  Round k takes candidates
    64 k .. 64 k + 63 and starts in the first step by whose end that many have been appended; what is left below 64 goes on the
    last step.  A round is tested where the next one starts, the last one on the last step; the steps in between that append
    nothing are the ones it idles over."""
    total = np.cumsum(added)
    T, last = int(total[-1]) if len(added) else 0, len(added) - 1
    start = [int(np.searchsorted(total, ROUND * (k + 1))) for k in range(T // ROUND)] + ([last] if T % ROUND else [])
    size = [ROUND] * (T // ROUND) + ([T % ROUND] if T % ROUND else [])
    tested = start[1:] + [last]
    return [(n, s, e, sum(1 for q in range(s + 1, e) if added[q] == 0)) for n, s, e in zip(size, start, tested)]


BLOCK_TOTALS = (1, 63, 64, 65, 127, 128, 129)


def edges(w):
    """The names of the loop edges one wave reaches (the scenes below say what each is for)."""
    e = set()
    if not w.steps:
        return e
    first, last = w.steps[0], w.steps[-1]
    span = w.end - first["p0"]
    if first["before_bit"]:
        e.add("bit_before_beg")
    if last["tail_bit"]:
        e.add("bit_after_end")
    for r in (0, 1, 255):
        if span % STEP == r:
            e.add(f"span_mod256_{r}")
    if w.total == 0 and len(w.steps) >= 3:
        e.add("no_candidate_3_steps")
    if w.total >= 1100 and w.max_position >= 2 * RING:
        e.add("ring_wraps_twice")
    if any(s["straddle"] for s in w.steps):
        e.add("lane_straddles_wrap")
    if any(s["cnt_before"] == ROUND - 1 and s["added"] == STEP and s["cnt_after"] == 319 for s in w.steps):
        e.add("occupancy_319")
    if w.total in BLOCK_TOTALS:
        e.add(f"total_{w.total}")
    if any(r["on_last"] and r["waiting"] == ROUND for r in w.rounds):
        e.add("start_64_on_last_step")
    if w.rounds and w.rounds[-1]["n"] in (1, 63):
        e.add(f"final_round_{w.rounds[-1]['n']}")
    if len(w.steps) > 1 and last["added"] == 0 and last["in_flight_in"]:
        e.add("last_step_adds_nothing_in_flight")
    if any(s["left_in_flight"] for s in w.steps):
        e.add("left_in_flight")
    if any(r["idle_steps"] == 1 for r in w.rounds):
        e.add("in_flight_over_1_idle_step")
    if any(r["idle_steps"] >= 2 for r in w.rounds):
        e.add("in_flight_over_2_idle_steps")
    return e


# =====================================================================================================================
# lists: from binning_model (CPU) or from Context.debug_snapshot() (device), and the waves that walk them
# =====================================================================================================================
class Lists:
    """tri [P] (triangle index of each pair), bmask [P], tile_start / tile_end [tiles], tiles_x, H, strip = (y0, y1)"""


def lists_from_model(m):
    """The sorted pair list of binning_model's model m: by tile, triangles in submission order."""
    per = [[] for _ in range(m.tiles_x * m.tiles_y)]
    for i in np.flatnonzero(m.has_pairs):
        for t, mk in BM.triangle_tiles(m, int(i)):
            per[t].append((int(i), mk))
    L = Lists()
    L.tri = np.array([i for p in per for i, _ in p], np.int64)
    L.bmask = np.array([mk for p in per for _, mk in p], np.uint16)
    n = np.array([len(p) for p in per], np.int64)
    L.tile_end = np.where(n > 0, np.cumsum(n), 0)
    L.tile_start = np.where(n > 0, np.cumsum(n) - n, EMPTY_START)
    L.tiles_x, L.H, L.strip = m.tiles_x, m.H, m.strip
    return L


def lists_from_snapshot(snap):
    info = snap["info"]
    L = Lists()
    L.tri = (snap["vals"] & np.uint32(0x1FFFFFF)).astype(np.int64)
    L.bmask = snap["bmask"]
    L.tile_start, L.tile_end = snap["tile_start"].astype(np.int64), snap["tile_end"].astype(np.int64)
    L.tiles_x, L.H, L.strip = info["tiles_x"], info["H"], (info["strip_y0"], info["strip_y1"])
    return L


def waves(L, tiles=None):
    """{(tile, kblk): Wave} for every wave the raster kernel runs over the lists: sixteen per tile with pairs, less the block rows
    outside the frame or the strip."""
    out = {}
    for t in (range(len(L.tile_start)) if tiles is None else tiles):
        beg, end = int(L.tile_start[t]), int(L.tile_end[t])
        if end <= beg:
            continue
        ty = t // L.tiles_x
        for brow in range(4):
            y0 = ty * BM.TILE + BM.BLOCK * brow
            if y0 < L.H and y0 + BM.BLOCK - 1 >= L.strip[0] and y0 < L.strip[1]:
                for c in range(4):
                    out[(t, 4 * brow + c)] = replay(beg, end, L.bmask, 4 * brow + c)
    return out


def reach(ws):
    """edge name -> number of waves that reach it"""
    out = {}
    for w in ws.values():
        for e in edges(w):
            out[e] = out.get(e, 0) + 1
    return out


# =====================================================================================================================
# scenes.  UNIT_VIEWPORT (screen = NDC), one constant depth per triangle, so that "in front of" is a plain comparison.
# A scene is a Scene: clip [n, 12], col [n], W, H and per triangle: tile, role (a string), block (the block it is meant for).
# Triangles are submitted tile by tile, so a tile's list is its triangles in the order given here.
# =====================================================================================================================
MAIN = 5                           # block (1, 1) of a tile: a full-block triangle from there stays inside the tile (blocks 1..3)


class Scene:
    def __init__(self, name, W, H, seed):
        self.name, self.W, self.H = name, W, H
        self.tiles_x = W // BM.TILE
        self.rows = {}                                   # tile -> [(clip row, role, block)]
        self.rng = scenes.SplitMix64(seed)
        self.u = self.rng.uniform(3 * 40000).reshape(-1, 3)
        self.k = 0

    def _origin(self, tile, block):
        ty, tx = divmod(tile, self.tiles_x)
        return tx * BM.TILE + BM.BLOCK * (block % 4), ty * BM.TILE + BM.BLOCK * (block // 4)

    def _add(self, tile, row, role, block):
        self.rows.setdefault(tile, []).append((row, role, block))

    def small(self, tile, block, z, role="small", r=None):
        """a triangle of radius 0.6..1.3 px (or r) well inside the block, in its rows 3..6 (so that a strip from row 3 on keeps it)"""
        X0, Y0 = self._origin(tile, block)
        u = self.u[self.k]; self.k += 1
        r = 0.6 + 0.7 * u[2] if r is None else r
        cx, cy = X0 + 2.2 + 3.2 * u[0], Y0 + 4.3 + 1.5 * u[1]
        self._add(tile, cases.screen_triangle((cx + r, cy), (cx - 0.5 * r, cy + 0.866 * r), (cx - 0.5 * r, cy - 0.866 * r), (z, z, z)), role, block)

    def wide(self, tile, block, z, role="overlap"):
        """a triangle of radius 2.5 px around a random centre of the block's middle: it overlaps its likes in part"""
        X0, Y0 = self._origin(tile, block)
        u = self.u[self.k]; self.k += 1
        cx, cy, r = X0 + 2.8 + 2.4 * u[0], Y0 + 2.8 + 2.4 * u[1], 2.5
        self._add(tile, cases.screen_triangle((cx + r, cy), (cx - 0.5 * r, cy + 0.866 * r), (cx - 0.5 * r, cy - 0.866 * r), (z, z, z)), role, block)

    def pixel(self, tile, block, i, z, role="disjoint"):
        """a triangle around the centre of pixel i (0..63) of the block that covers this pixel centre and no other"""
        X0, Y0 = self._origin(tile, block)
        cx, cy, r = X0 + (i % 8) + 0.5, Y0 + (i // 8) + 0.5, 0.45
        self._add(tile, cases.screen_triangle((cx + r, cy), (cx - 0.5 * r, cy + 0.866 * r), (cx - 0.5 * r, cy - 0.866 * r), (z, z, z)), role, block)

    def full(self, tile, block, z, role="full", shape=0):
        """a triangle that covers all 64 pixel centres of the block (and parts of the blocks right of and above it, inside the tile);
        shape 1 has other barycentrics at the same pixels (CHECKER discards other fragments of it)"""
        assert block % 4 <= 1 and block // 4 <= 1
        X0, Y0 = self._origin(tile, block)
        bx, cy = ((16.3, 16.3), (17.3, 15.9))[shape]
        self._add(tile, cases.screen_triangle((X0 + 0.1, Y0 + 0.1), (X0 + bx, Y0 + 0.1), (X0 + 0.1, Y0 + cy), (z, z, z)), role, block)

    def sliver(self, tile):
        """one triangle that k_setup sends down the literal path (test_raster_paths.literal_scene, reason 2), in a tile of its own"""
        X0, Y0 = self._origin(tile, 0)
        x0, y0, L, wd = X0 + 3.5, Y0 + 9.5, 20.0, 1e-11
        self._add(tile, cases.screen_triangle((x0, y0), (x0 + L, y0), (x0 + L / 2, y0 + wd), (0.1, 0.2, 0.3)), "sliver", 4)

    def depth(self, lo=-0.8, hi=0.8):
        self.k += 1
        return lo + (hi - lo) * float(self.u[self.k - 1][0])

    def build(self):
        order = [(t, row, role, block) for t in sorted(self.rows) for row, role, block in self.rows[t]]
        self.clip = np.array([o[1] for o in order]).reshape(-1, 12)
        self.tile = np.array([o[0] for o in order], np.int64)
        self.role = np.array([o[2] for o in order])
        self.block = np.array([o[3] for o in order], np.int64)
        self.col = (np.arange(len(order), dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0xFF000000)
        self.z = self.clip[:, 2].copy()
        return self

    def in_list(self, tile):
        """list-relative index of the next triangle of the tile"""
        return len(self.rows.get(tile, []))


STEP_LENGTHS = (255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025)


def steps_scene(a):
    """256 x 64.  Tile 0 holds `a` triangles (a = 0..3), tiles 1..12 lists of STEP_LENGTHS, tile 13 five: over a = 0..3 every length
    starts at every beg & 3.  Every triangle lies in block MAIN of its tile, so the entries before a list's beg and behind its end
    carry the bit of the wave that has candidates there, and the other fifteen blocks of a tile have no candidate in lists of up
    to five steps."""
    s = Scene(f"steps_{a}", 256, 64, seed=9100 + a)
    for _ in range(a):
        s.small(0, MAIN, s.depth())
    for t, n in enumerate(STEP_LENGTHS, start=1):
        for _ in range(n):
            s.small(t, MAIN, s.depth())
    for _ in range(5):
        s.small(13, MAIN, s.depth())
    return s.build()


def stale_words_draw(W, H, n=500):
    """A FLAT draw of n triangles that each cover the whole frame: flushed BEFORE a steps scene on the same context, it leaves
    16 n pairs with every block bit set in the pair buffers, the stale words behind the last tile's end.  Depths 0.9 and 0.95:
    behind everything else."""
    clip = np.array([cases.screen_triangle((-8.0, -8.0), (3.0 * W, -8.0), (-8.0, 5.0 * H), (z, z, z)) for z in [0.9] + [0.95] * (n - 1)])
    return clip, np.full(n, 0xFF203040, np.uint32)


def ring_scene():
    """128 x 32.  Tile 0: one triangle (so tile 1 begins at beg & 3 = 1).  Tile 1, front to back: two full-block triangles (the
    second makes the wave resolve the first, after which the block's largest depth is 0.5) and 1102 small ones behind them with
    rising depth - most are culled.  Tile 2, back to front: 1101 small ones, each nearer than all before - most are visited.
    Both lists give block MAIN 1100 candidates and more from beg & 3 = 1: 255 + 256 + 256 + ... entries per step."""
    s = Scene("ring", 128, 32, seed=9200)
    s.small(0, MAIN, 0.0)
    s.full(1, MAIN, 0.5, "front"); s.full(1, MAIN, 0.4, "front")
    for i in range(1102):
        s.small(1, MAIN, 0.55 + 0.0003 * i)
    for i in range(1101):
        s.small(2, MAIN, 0.95 - 0.0017 * i)
    return s.build()


RING_STRIP = (11, 29)              # rows owned in the strip run: block rows 1 and 3 of the tiles are owned in part


def _fill_to(s, tile, block, r):
    while s.in_list(tile) < r:
        s.small(tile, block, s.depth())


def rounds_scene():
    """160 x 32.  Tile 0: blocks 0, 1, 2, 3, 4, 6, 7 receive 1, 63, 64, 65, 127, 128 and 129 candidates.  Tile 1: one step, 64 of
    block 0 (a round started with exactly 64 waiting on the last step).  Tile 2, four steps: block 0 has 70 at the start, nothing
    in steps 1 and 2, five in step 3; block 2 has 70 in step 1, nothing in step 2, five in step 3 (requests in flight over two and
    over one step that add nothing).  Tile 3, two steps: block 0 has 70 in step 0 and nothing in the last."""
    s = Scene("rounds", 160, 32, seed=9300)
    for block, n in zip((0, 1, 2, 3, 4, 6, 7), BLOCK_TOTALS):
        for _ in range(n):
            s.small(0, block, s.depth())
    for _ in range(64):
        s.small(1, 0, s.depth())
    for _ in range(10):
        s.small(1, 1, s.depth())
    _fill_to(s, 2, 0, 70); _fill_to(s, 2, 1, 300); _fill_to(s, 2, 2, 370); _fill_to(s, 2, 1, 800); _fill_to(s, 2, 2, 805)
    _fill_to(s, 2, 1, 990); _fill_to(s, 2, 0, 995); _fill_to(s, 2, 1, 1000)
    _fill_to(s, 3, 0, 70); _fill_to(s, 3, 1, 400)
    return s.build()


SURVIVOR_TILES = {0: 1, 1: 2, 2: 63, 3: 64, 4: 1}        # tile -> fronts in the second round of its block MAIN
NAN_TILE = 4


def survivors_scene():
    """192 x 32.  Per tile of SURVIVOR_TILES, block MAIN gets 128 candidates in one step, two rounds of 64.  Round one: two full-block
    triangles (0.5, then 0.4: the wave resolves the first, the block's largest depth is 0.5 from then on) and 62 small ones at 0.8.
    Round two: k full-block triangles, each strictly in front of everything before it (role "front"), among 64 - k small ones at
    0.7, which the cull drops.  k = 1 and 63 leave an odd survivor (the partner record), k = 64 makes the lane index wrap."""
    s = Scene("survivors", 192, 32, seed=9400)
    for t, k in SURVIVOR_TILES.items():
        s.full(t, MAIN, 0.5, "cover"); s.full(t, MAIN, 0.4, "cover")
        for _ in range(62):
            s.small(t, MAIN, 0.8)
        behind = {1: set(range(64)) - {37}, 2: set(range(64)) - {0, 63}, 63: {10}, 64: set()}[k]
        f = 0
        for i in range(64):
            if i in behind:
                s.small(t, MAIN, 0.7)
            else:
                s.full(t, MAIN, 0.3 - 0.004 * f, "front"); f += 1
    return s.build()


def survivors_nan_zbuffer(s):
    """A z-buffer for survivors_scene: +inf, and NaN on eleven pixels of block MAIN of NAN_TILE (they let every depth plane pass
    the first test of a visit, the partner record's too, and can never be written)."""
    z = np.full((s.H, s.W), np.inf)
    X0, Y0 = s._origin(NAN_TILE, MAIN)
    z[Y0 + 2, X0:X0 + 8] = np.nan
    z[Y0 + 5, X0 + 1:X0 + 4] = np.nan
    return z


STACK = 200


def notes_scene():
    """160 x 32.  Tile 0: (a) 64 pairwise-disjoint one-pixel triangles in block MAIN, consecutive in the list (notes pile up
    without a resolve), and (e) 40 triangles of radius 2.5 in block 7 that overlap in part, nearer and nearer.  Tiles 1, 2, 3: 100
    triangles of block 0, then a stack of 200 full-block triangles on block MAIN at (b) falling, (c) equal, (d) rising depth.  Block
    MAIN gets 156 - (beg & 3) of them in step 0 - one round is visited there, a second is in flight - and the rest in step 1, where
    three more rounds follow: its notes cross a list step and round boundaries.  Stacks (b) and (d) alternate between two shapes,
    so that under CHECKER the nearest triangle of (d) discards fragments where the next, farther one passes."""
    s = Scene("notes", 160, 32, seed=9500)
    for i in range(64):
        s.pixel(0, MAIN, (i * 27) % 64, s.depth())
    for i in range(40):
        s.wide(0, 7, 0.9 - 0.04 * i)
    for t, zf in ((1, lambda i: 0.9 - 0.009 * i), (2, lambda i: 0.25), (3, lambda i: -0.9 + 0.009 * i)):
        _fill_to(s, t, 0, 100)
        for i in range(STACK):
            s.full(t, MAIN, zf(i), "stack", shape=i % 2 if t != 2 else 0)      # (c): one shape, so that the depths tie bit for bit
    return s.build()


SCENES = {"ring": ring_scene, "rounds": rounds_scene, "survivors": survivors_scene, "notes": notes_scene}
EXTRA_TILE = {"ring": 3, "rounds": 4, "survivors": 5, "notes": 4}       # a tile no scene uses: the literal sliver goes there

_built = {}


def scene(name):
    """a built scene, once ("steps_0".."steps_3" or a key of SCENES); never written to"""
    if name not in _built:
        _built[name] = steps_scene(int(name[-1])) if name.startswith("steps_") else SCENES[name]()
    return _built[name]


def with_sliver(s):
    """(clip, col) of the scene with one literal triangle appended, in the scene's spare tile"""
    t = Scene("sliver", s.W, s.H, seed=1)
    t.sliver(EXTRA_TILE[s.name])
    t.build()
    return np.concatenate([s.clip, t.clip]), np.concatenate([s.col, np.array([0xFF00C0F0], np.uint32)])


def with_large_triangle(s):
    """(clip, col) with one triangle of 64 pixels and more submitted first, behind everything (depth 0.99): the flush then compares
    the depth bounds of its pair words (zq_cull)."""
    big = cases.screen_triangle((-4.0, -4.0), (s.W + 40.0, -4.0), (-4.0, 3.0 * s.H), (0.99, 0.99, 0.99))
    return np.concatenate([big[None], s.clip]), np.concatenate([np.array([0xFF112233], np.uint32), s.col])


# ---- what each scene has to reach: the assertions shared by the CPU and the GPU tests -------------------------------------------
def wave_rounds_by_role(w, L, s, role):
    """per round of the wave: how many of its candidates are triangles of the scene with that role (a literal sliver appended to
    the scene has an index behind its roles)"""
    return [sum(1 for q in r["members"] if L.tri[q] < len(s.role) and s.role[L.tri[q]] == role) for r in w.rounds]


REQUIRED = {
    "steps": {"bit_before_beg", "bit_after_end", "no_candidate_3_steps"},
    "ring": {"ring_wraps_twice", "lane_straddles_wrap", "occupancy_319"},
    "rounds": {f"total_{n}" for n in BLOCK_TOTALS} | {"start_64_on_last_step", "final_round_1", "final_round_63",
                                                       "last_step_adds_nothing_in_flight", "in_flight_over_1_idle_step",
                                                       "in_flight_over_2_idle_steps"},
    "survivors": set(), "notes": set(),
}


# which of the spans end - (beg & ~3) = 0, 1, 255 mod 256 the lists of steps_scene(a) have.  Every triple 256 k - 1, 256 k, 256 k + 1 of
# STEP_LENGTHS sums to 0 mod 4, so with b = (a + 3) & 3 its lists begin at beg & 3 = a, b, b and span 256 k + a - 1, 256 k + b and
# 256 k + 1 + b.  Over a = 0..3 all three residues occur.
STEP_SPANS = {0: {"span_mod256_255"}, 1: {"span_mod256_0", "span_mod256_1"}, 2: {"span_mod256_1"}, 3: set()}


def step_alignments(L):
    """list length -> beg & 3, of the twelve lists of a steps scene"""
    return {int(L.tile_end[t] - L.tile_start[t]): int(L.tile_start[t]) & 3 for t in range(1, 1 + len(STEP_LENGTHS))}


def assert_reach(s, L):
    """Every edge the scene `s` is built for occurs in some wave of the lists L (of a flush that holds the scene's triangles first, in
    the scene's order).  Returns reach(waves)."""
    ws = waves(L)
    got = reach(ws)
    kind = s.name.split("_")[0]
    missing = REQUIRED[kind] - set(got)
    assert not missing, f"{s.name}: no wave reaches {sorted(missing)} (reached: {got})"
    if kind == "steps":
        # tile 0 holds exactly `a` pairs, so every list begins where the arithmetic says: over a = 0..3 that is every length at
        # every beg & 3, and the spans 0, 1 and 255 mod 256 that follow from it
        a = int(s.name[-1])
        assert (int(L.tile_end[0]) - int(L.tile_start[0]) if a else int(L.tile_end[0])) == a, (L.tile_start[0], L.tile_end[0])
        begs = a + np.concatenate([[0], np.cumsum(STEP_LENGTHS[:-1])])
        assert step_alignments(L) == {n: int(b) & 3 for n, b in zip(STEP_LENGTHS, begs)}, step_alignments(L)
        spans = {f"span_mod256_{(n + (int(b) & 3)) % STEP}" for n, b in zip(STEP_LENGTHS, begs)} & {f"span_mod256_{r}" for r in (0, 1, 255)}
        assert spans == STEP_SPANS[a] and spans <= set(got), (spans, got)
        for t in range(1, 1 + len(STEP_LENGTHS)):
            beg, end = int(L.tile_start[t]), int(L.tile_end[t])
            assert beg == begs[t - 1], (t, beg)
            w = ws[(t, MAIN)]
            assert w.total == end - beg and len(w.steps) == -(-(end - (beg & ~3)) // STEP)
            if beg & 3:
                assert w.steps[0]["before_bit"] == (beg & 3), (t, w.steps[0])       # the previous tile's last entries carry the bit
            assert w.tail_bit == (-end) % 4, (t, w.tail_bit)                        # and so do the next tile's first
        assert sorted(step_alignments(L)) == sorted(STEP_LENGTHS)
    if kind == "ring":
        for t in (1, 2):
            w = ws[(t, MAIN)]
            e = edges(w)
            assert {"ring_wraps_twice", "lane_straddles_wrap", "occupancy_319"} <= e, (t, e)
            assert w.total >= 1100 and w.max_occupancy == 319
    if kind == "survivors":
        for t, k in SURVIVOR_TILES.items():
            w = ws[(t, MAIN)]
            fronts = wave_rounds_by_role(w, L, s, "front")
            assert [r["n"] for r in w.rounds] == [64, 64] and fronts == [0, k], (t, fronts)
    if kind == "notes":
        w = ws[(0, MAIN)]
        assert max(wave_rounds_by_role(w, L, s, "disjoint")) >= 16 and w.total == 64
        assert ws[(0, 7)].total == 40
        for t in (1, 2, 3):
            w = ws[(t, MAIN)]
            per = wave_rounds_by_role(w, L, s, "stack")
            assert sum(per) == STACK and sum(1 for n in per if n) >= 3, per
            visited_in = {r["tested_in_step"] for r, n in zip(w.rounds, per) if n}
            assert visited_in == {0, 1}, visited_in        # a stack round is visited before the list step, the others behind it
    return got
