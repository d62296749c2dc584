"""Times of depth-ordered triangle draws on one MI355X (DESIGN.md §6 "Depth-ordered triangle draws" records the results).

  python profiles/triangle_order_probe.py [--size 4096] [--triangles 1000000] [--head-level 7] [--reps 20] [--limit 900]
                                          [--out profiles/triangle_order_probe_summary.txt]

Two sets of rows on a --size x --size frame: --triangles random translucent triangles (K = 0, colours; a kind that blends), and the PHONG
rows of the head stand-in at --head-level (20 * 4^level faces: 327 680 at level 7; K = 24, no colours).  Medians after a warm-up, with
min and max.
  (a) depths    k_triangle_depths (CENTROID, group 1) against a device-to-device copy of the clip array, which reads as many bytes
                (n * 96) and writes as many again; HIP events on the context's stream.  The ratio is recorded.
  (b) gather    trgl_order_stage under a random permutation against a copy that moves as many bytes, and against torch's route on the
                same arrays (index_select of clip, varyings and colours into preallocated outputs).  Required: the gather is not slower
                than the torch route, within that yardstick's own spread over its reps.  The ratio to the copy is recorded.
  (c) chain     trgl_triangle_depths + trgl_depth_order + trgl_draw_ordered + flush + sync against trgl_draw + flush + sync of arrays
                sorted beforehand; the host clock.  The difference is what depths, sort and gather cost a frame.
(a) and (b) alternate their sides inside one loop, two untimed snapshot copies queued in front so that the events bracket device work.
The measurement runs in one child process under a time limit of --limit seconds; the parent never touches the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3
OVER = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
"""


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import scenes
    from tinyrenderder_amd.api import PHONG, Context, make_uniforms
    if not torch.cuda.is_available():
        raise SystemExit("triangle_order_probe: no GPU; there is nothing to measure without one")
    size = a.size
    res = dict(size=size)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    with Context(size, size, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        over = ctx.register_shader(OVER, 0, True, reads_dest=True, depth_write=False)
        ctx.zbuffer_snapshot(1)

        def event_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream); out = fn(); e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        def alternate(sides):
            ts = {k: [] for k in sides}
            for rep in range(WARM + a.reps):
                for k, fn in sides.items():
                    ms, _ = event_ms(fn)
                    if rep >= WARM:
                        ts[k].append(ms)
                ctx.sync()
                ctx._keep.clear()
            return {k: stat(v) for k, v in ts.items()}

        def host_ms(fn):
            v = []
            for rep in range(WARM + a.reps):
                ctx.clear((0, 0, 0, 255), np.inf); ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync()
                if rep >= WARM:
                    v.append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return stat(v)

        for name in ("soup", "head"):
            if name == "soup":
                n = a.triangles
                clip, _ = scenes.random_triangles(n, size, size, perspective_w=True)
                col = (scenes.SplitMix64(77).u64(n) >> np.uint64(32)).astype(np.uint32)
                vary, kind, u = None, over, None
            else:
                hd = scenes.head_standin(a.head_level, size, size)
                clip, vary, col = hd["clip"], hd["varyings"], None
                n, kind = clip.shape[0], PHONG
                u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"])
            K = 0 if vary is None else vary.shape[1]
            d_clip = torch.from_numpy(clip).cuda()
            d_vary = None if vary is None else torch.from_numpy(np.ascontiguousarray(vary)).cuda()
            d_col = None if col is None else torch.from_numpy(col.view(np.int32)).cuda()
            perm = torch.from_numpy(np.argsort(scenes.SplitMix64(78).u64(n), kind="stable").astype(np.int32)).cuda()
            arrays = [t for t in (d_clip, d_vary, d_col) if t is not None]
            outs = [torch.empty_like(t) for t in arrays]
            outs2 = [torch.empty_like(t) for t in arrays]
            out3 = (outs[0], outs[1] if K else None, outs[-1] if col is not None else None)
            torch.cuda.synchronize()
            r = dict(n=n, K=K, colors=col is not None, row_bytes=96 + 8 * K + (4 if col is not None else 0))

            # ---- (a) ----
            def depths():
                return ctx.triangle_depths(d_clip, 1, 0, device=True)

            def copy_clip():
                with torch.cuda.stream(stream):
                    outs2[0].copy_(d_clip)

            r["a"] = alternate(dict(depths=depths, copy=copy_clip))
            ctx.sync()

            # ---- (b) ----
            def gather():
                return ctx.order_stage(d_clip, d_vary, d_col, perm, 1, device=True, out=out3)

            def copy_all():
                with torch.cuda.stream(stream):
                    for o, t in zip(outs2, arrays):
                        o.copy_(t)

            def torch_route():
                with torch.cuda.stream(stream):
                    for o, t in zip(outs2, arrays):
                        torch.index_select(t, 0, perm, out=o)

            r["b"] = alternate(dict(gather=gather, copy=copy_all, torch=torch_route))
            ctx.sync()
            for o, o2 in zip(outs, outs2):                         # what was timed computes the same bytes as torch's route
                assert torch.equal(o.view(torch.uint8), o2.view(torch.uint8)), "the gather and index_select differ"

            # ---- (c) ----
            def chain():
                d = ctx.triangle_depths(d_clip, 1, 0, device=True)
                o = ctx.depth_order(d, device=True)
                ctx.draw(kind, d_clip, d_vary, d_col, u, device=True, order=o, order_device=True)
                ctx.flush()
                return o

            o = chain(); ctx.sync()
            fb0, st0 = ctx.read_framebuffer(), ctx.stats()
            with torch.cuda.stream(stream):
                idx = o.long()
                sorted_arrays = [None if t is None else t[idx].contiguous() for t in (d_clip, d_vary, d_col)]
            ctx.sync()

            def presorted():
                ctx.draw(kind, sorted_arrays[0], sorted_arrays[1], sorted_arrays[2], u, device=True)
                ctx.flush()

            ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); chain(); fb0, st0 = ctx.read_framebuffer(), ctx.stats()
            ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); presorted(); fb1, st1 = ctx.read_framebuffer(), ctx.stats()
            assert np.array_equal(fb0, fb1) and st0 == st1, "the ordered draw and the draw of sorted arrays differ"
            for rep in range(2):                                   # the two alternate: two rounds each, the second is reported
                r["c"] = dict(chain=host_ms(chain), presorted=host_ms(presorted))
            res[name] = r
            print(name, json.dumps(r), flush=True)
            del d_clip, d_vary, d_col, perm, arrays, outs, outs2, out3, sorted_arrays
            ctx._keep.clear()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--head-level", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--triangles", str(a.triangles), "--head-level", str(a.head_level),
                        "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("triangle_order_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    tbs = lambda nbytes, v: nbytes / (v["median_ms"] * 1e-3) / 1e12
    lines = ["depth-ordered triangle draws, one MI355X, one run on %s, %d x %d frame" % (time.strftime("%Y-%m-%d"), res["size"], res["size"]),
             "medians (min .. max) after a warm-up; (a), (b) HIP events on the context's stream, (c) the host clock around calls + flush + sync"]
    gate_ok = True
    for name, what in (("soup", "random translucent triangles, K = 0, colours"), ("head", "PHONG rows of the head stand-in, K = 24")):
        r = res[name]
        n, rb = r["n"], r["row_bytes"]
        lines.append("%s: %d %s (%d bytes per row)" % (name, n, what, rb))
        d, c = r["a"]["depths"], r["a"]["copy"]
        lines.append("(a) k_triangle_depths   %s  reads n * 96 bytes at %.2f TB/s" % (fmt(d), tbs(n * 96, d)))
        lines.append("    copy of the clip    %s  reads n * 96 and writes n * 96; ratio %.3f" % (fmt(c), d["median_ms"] / c["median_ms"]))
        g, c, t = r["b"]["gather"], r["b"]["copy"], r["b"]["torch"]
        spread = t["max_ms"] - t["min_ms"]
        ok = g["median_ms"] <= t["median_ms"] + spread
        gate_ok = gate_ok and ok
        lines.append("(b) k_gather_rows       %s  one launch per array, %.2f TB/s read + written" % (fmt(g), tbs(2 * n * rb, g)))
        lines.append("    copy of as many     %s  ratio %.3f" % (fmt(c), g["median_ms"] / c["median_ms"]))
        lines.append("    torch index_select  %s  ratio %.3f, the yardstick's own spread %.3f ms: %s" % (
            fmt(t), g["median_ms"] / t["median_ms"], spread, "not slower" if ok else "SLOWER than the yardstick - the requirement is missed"))
        ch, ps = r["c"]["chain"], r["c"]["presorted"]
        lines.append("(c) depths, order, ordered draw, flush  %s" % fmt(ch))
        lines.append("    trgl_draw of sorted arrays, flush   %s  ratio %.3f, difference %.3f ms" % (fmt(ps), ch["median_ms"] / ps["median_ms"],
                                                                                                 ch["median_ms"] - ps["median_ms"]))
    lines += ["notes: the arrays of a set are read again by every repetition and fit the 256 MiB Infinity Cache, as they do in a frame whose",
              "vertex stage has just written them: the rates above are not HBM rates, and the 5.5 TB/s MI355X_MICROARCH.md reports for whole-row gathers",
              "(1,152-byte rows, a table far larger than that cache) is not their yardstick.  What keeps the gather above the copy was not",
              "profiled; rows here are 96 to 288 bytes (4 for colours), each behind a read of the list, one launch per array."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if not gate_ok:
        raise SystemExit("triangle_order_probe: the gather is slower than the torch route")


if __name__ == "__main__":
    main()
