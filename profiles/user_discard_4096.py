"""A 4096x4096 frame of 1 M random triangles (scenes.random_triangles, bench.py's generator) with the built-in CHECKER kind and with
a user kind that may discard and restates it (tests/discard_shader_sources.py: TRGL_SHADER_MAY_DISCARD, its own raster kernel).

    rocprofv3 --kernel-trace --stats -d DIR -o discard -- python profiles/user_discard_4096.py
    python profiles/user_discard_4096.py --summarize DIR/discard_results.db > profiles/user_discard_4096_summary.txt

The first form draws the frame 6 times with each kind, alternating, one flush per frame, checks that the two frames (pixels, z bits,
counters) are bit-identical and prints the registration times (host clock).  The second reads the kernel trace: per-kernel durations,
and per frame the GPU time of its kernels (a flush starts at k_setup).  The committed summary also carries the lines the first form
printed in the same run."""
import os
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 6
N, W, H, CELLS = 1 << 20, 4096, 4096, 8


def render():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import discard_shader_sources as D
    from tinyrenderder_amd import scenes
    from tinyrenderder_amd.api import Context, CHECKER, make_uniforms
    clip, col = scenes.random_triangles(N, W, H)
    u = make_uniforms(cells=CELLS)
    with Context(W, H, 3) as ctx:
        t0 = time.perf_counter(); kind = ctx.register_shader(D.CHECKER, 0, may_discard=True); t1 = time.perf_counter()
        with Context(64, 64, 3) as c2:
            t2 = time.perf_counter(); c2.register_shader(D.CHECKER, 0, may_discard=True); t3 = time.perf_counter()
        print(f"registration: first in the process (compile + load) {1e3 * (t1 - t0):.1f} ms, "
              f"cached on a second context (load only) {1e3 * (t3 - t2):.2f} ms")
        out = {}
        for k in (CHECKER, kind) * FRAMES:
            ctx.clear(); ctx.reset_stats(); ctx.draw(k, clip, colors=col, uniforms=u); ctx.flush()
            out[k] = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats_line())
        same = (np.array_equal(out[CHECKER][0], out[kind][0]) and np.array_equal(out[CHECKER][1].view(np.uint64), out[kind][1].view(np.uint64))
                and out[CHECKER][2] == out[kind][2])
        print("frames bit-identical:", same, "-", out[kind][2].strip())
        return 0 if same else 1


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    return name.split("(")[0]


def summarize(db):
    c = sqlite3.connect(db)
    ks = c.execute("select name, start, end from kernels order by start").fetchall()
    frames, cur = [], None
    for name, start, end in ks:
        n = short(name)
        if n == "k_setup":
            cur = []; frames.append(cur)
        if cur is not None:
            cur.append((n, start, end))
    per = {"built-in CHECKER": [], "user kind": []}
    for f in frames:
        key = "user kind" if any(n == "trgl_raster_user" for n, _, _ in f) else "built-in CHECKER"
        per[key].append((sum(e - s for _, s, e in f) / 1e3, (max(e for _, _, e in f) - min(s for _, s, _ in f)) / 1e3))
    rows = c.execute("select name, count(*), avg(duration), min(duration), max(duration) from kernels group by name "
                     "order by sum(duration) desc").fetchall()
    avg = {short(r[0]): r[2] / 1e3 for r in rows}
    builtin = next(k for k in avg if k.startswith("k_raster<4"))
    for para in __doc__.split("\n\n"):
        print("\n".join("# " + ln for ln in para.splitlines()))
    print("# MI355X, one GPU.  Microseconds.")
    print(f"# raster kernel: trgl_raster_user / {builtin} = {avg['trgl_raster_user'] / avg[builtin]:.3f} (estimate <= 3)")
    med = {k: (statistics.median(a for a, _ in v), statistics.median(b for _, b in v)) for k, v in per.items()}
    for k, (gpu, span) in med.items():
        print(f"# frame, {k}: median over {len(per[k])} frames: kernels {gpu:.1f}, first start to last end {span:.1f}")
    print(f"# frame ratio user / built-in: kernels {med['user kind'][0] / med['built-in CHECKER'][0]:.3f}, "
          f"span {med['user kind'][1] / med['built-in CHECKER'][1]:.3f}")
    print()
    print("%-48s %6s %10s %10s %10s" % ("kernel", "calls", "avg_us", "min_us", "max_us"))
    for r in rows:
        print("%-48s %6d %10.1f %10.1f %10.1f" % (short(r[0])[:48], r[1], r[2] / 1e3, r[3] / 1e3, r[4] / 1e3))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        sys.exit(summarize(sys.argv[2]))
    sys.exit(render())
