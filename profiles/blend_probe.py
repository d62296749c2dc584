"""A 4096x4096 frame of 1 M random triangles (scenes.random_triangles, bench.py's generator, with random alphas in the colours) drawn
by user kinds of the run-time raster kernel (raster_user.h): the CHECKER restatement with TRGL_SHADER_MAY_DISCARD alone (flags 1), a
kind that returns its colour (flags 1), and trgl_blend_over with TRGL_SHADER_READS_DEST (flags 5) and with TRGL_SHADER_NO_DEPTH_WRITE
as well (flags 13) - each from a clear and onto a resident frame (the clear flushed on its own first, so the kernel loads the depths
and, under READS_DEST, the pixels).

    rocprofv3 --kernel-trace --stats -d DIR -o blend -- python profiles/blend_probe.py > DIR/render.log
    python profiles/blend_probe.py --summarize DIR/blend_results.db DIR/render.log > profiles/blend_probe_summary.txt

The first form draws the 8 frames 5 times over, one flush per frame, and prints each kind's stats line.  The second reads the kernel
trace: the i-th trgl_raster_user launch belongs to frame i of that fixed order.  fragments_drawn is the number of trgl_fragment
calls that drew: without depth writes every covered fragment in front of the clear depth draws, so flags 13 shades about twice the
fragments of flags 5 on this overdrawn scene.  The CHECKER restatement discards half of its z-passes and converts two doubles per
call; "source" is the never-discarding kind the blending kinds are to be compared with."""
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5
N, W, H, CELLS = 1 << 20, 4096, 4096, 8
KINDS = ["checker flags 1", "source flags 1", "over flags 5", "over flags 13"]
STATES = ["from a clear", "resident frame"]
ORDER = [(k, s) for s in STATES for k in KINDS]

SOURCE = "__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, in.color }; }\n"
OVER = "__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }\n"


def render():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import discard_shader_sources as D
    from tinyrenderder_amd import scenes
    from tinyrenderder_amd.api import Context, make_uniforms
    clip, _ = scenes.random_triangles(N, W, H)
    col = (scenes.SplitMix64(77).u64(N) >> np.uint64(32)).astype(np.uint32)
    u = make_uniforms(cells=CELLS)
    with Context(W, H, 3) as ctx:
        kinds = {"checker flags 1": ctx.register_shader(D.CHECKER, 0, True), "source flags 1": ctx.register_shader(SOURCE, 0, True),
                 "over flags 5": ctx.register_shader(OVER, 0, True, reads_dest=True),
                 "over flags 13": ctx.register_shader(OVER, 0, True, reads_dest=True, depth_write=False)}
        lines = {}
        for _ in range(REPEATS):
            for k, s in ORDER:
                ctx.clear(); ctx.reset_stats()
                if s == "resident frame":
                    ctx.flush()                        # the clear values go to memory: the draw's flush starts from them there
                ctx.draw(kinds[k], clip, colors=col, uniforms=u); ctx.flush()
                lines[(k, s)] = ctx.stats_line().strip()
        for k in KINDS:
            same = lines[(k, STATES[0])] == lines[(k, STATES[1])]
            print(f"{k}: {lines[(k, STATES[0])]}" + ("" if same else f"  BUT onto the resident frame {lines[(k, STATES[1])]}"))
        return 0 if all(lines[(k, STATES[0])] == lines[(k, STATES[1])] for k in KINDS) else 1


def summarize(db, log):
    c = sqlite3.connect(db)
    durs = [r[0] / 1e3 for r in c.execute("select end - start from kernels where name like '%trgl_raster_user%' order by start")]
    assert len(durs) == REPEATS * len(ORDER), (len(durs), REPEATS * len(ORDER))
    per = {o: durs[i::len(ORDER)] for i, o in enumerate(ORDER)}
    for para in __doc__.split("\n\n"):
        print("\n".join("# " + ln for ln in para.splitlines()))
    print("# MI355X, one GPU.  trgl_raster_user, microseconds; /checker and /source: to those flags-1 kinds in the same state.")
    for ln in open(log).read().splitlines():
        print("# " + ln)
    print()
    print("%-18s %-16s %6s %10s %10s %10s %9s %9s" % ("kind", "state", "calls", "avg_us", "min_us", "max_us", "/checker", "/source"))
    for s in STATES:
        checker, source = sum(per[(KINDS[0], s)]) / REPEATS, sum(per[(KINDS[1], s)]) / REPEATS
        for k in KINDS:
            d = per[(k, s)]
            a = sum(d) / len(d)
            print("%-18s %-16s %6d %10.1f %10.1f %10.1f %9.3f %9.3f" % (k, s, len(d), a, min(d), max(d), a / checker, a / source))
    print()
    for k in KINDS:
        a, b = sum(per[(k, STATES[0])]) / REPEATS, sum(per[(k, STATES[1])]) / REPEATS
        print(f"# {k}: resident frame / from a clear = {b / a:.3f}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summarize":
        sys.exit(summarize(sys.argv[2], sys.argv[3]))
    sys.exit(render())
