"""Times of the sprite and line stages on one MI355X (DESIGN.md §6 "Point sprites and wide lines" records the results).

  python profiles/sprite_probe.py [--size 4096] [--points 1000000] [--reps 20] [--limit 900] [--out profiles/sprite_probe_summary.txt]

Three sets: --points sprites with n_attr = 0 (rows x, y, z, size) and with n_attr = 2 (two more doubles), both with colours, and --points
indexed segments over half as many points (rows x, y, z), with colours.  Medians after a warm-up, with min and max.
  (a) the stage kernel (k_sprite_stage / k_line_stage), HIP events on the context's stream
  (b) a device-to-device copy that reads and writes as many bytes together as the kernel reads plus writes, timed the same way and
      alternating with (a) inside one loop; the ratio (a) / (b) is recorded
  (c) the route the stage replaces: the host twin, then an upload of its rows; the host clock around both and a synchronise
  (d) a whole blended frame on a --size x --size target: sprite stage + triangle depths (group 2) + depth order + ordered draw + flush +
      sync, against trgl_draw + flush + sync of rows expanded and sorted beforehand; the host clock.  Both frames are compared first.
Two untimed snapshot copies are queued in front of (a) and (b) so that the events bracket device work.  The measurement runs in one
child process under a time limit of --limit seconds; the parent never touches the GPU."""
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
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import Context
    if not torch.cuda.is_available():
        raise SystemExit("sprite_probe: no GPU; there is nothing to measure without one")
    size, n = a.size, a.points
    res = dict(size=size, n=n)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    mv = scenes.lookat((0.3, 0.2, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    pr = scenes.perspective(0.5, 1.0, 0.25, 20.0)
    with Context(size, size, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        over = ctx.register_shader(OVER, 0, True, reads_dest=True, depth_write=False)
        ctx.zbuffer_snapshot(1)

        def event_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream); fn(); e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def alternate(sides):
            ts = {k: [] for k in sides}
            for rep in range(WARM + a.reps):
                for k, fn in sides.items():
                    ms = event_ms(fn)
                    if rep >= WARM:
                        ts[k].append(ms)
                ctx.sync()
                ctx._keep.clear()
            return {k: stat(v) for k, v in ts.items()}

        def host_ms(fn, reps, clear=False):
            v = []
            for rep in range(1 + reps):
                if clear:
                    ctx.clear((0, 0, 0, 255), np.inf)
                ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync(); torch.cuda.synchronize()
                if rep >= 1:
                    v.append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return stat(v)

        r = scenes.SplitMix64(91)
        col = (r.u64(n) >> np.uint64(32)).astype(np.uint32)
        d_col = torch.from_numpy(col.view(np.int32)).cuda()
        sets = {}
        for name, n_attr in (("sprites_attr0", 0), ("sprites_attr2", 2)):
            stride = 4 + n_attr
            pts = r.uniform(n * stride, -1.0, 1.0).reshape(n, stride)
            pts[:, 3] = r.uniform(n, 2.0, 6.0)                       # pixels
            P = api.make_sprite_params(mv, pr, 1.0, (2.0 / size, 2.0 / size), api.SPRITE_SCREEN, 3, 4, n_attr)
            sets[name] = dict(kind="sprites", P=P, pts=pts, idx=None, K=6 + n_attr, read=n * (stride * 8 + 4))
        m = n // 2
        lpts = r.uniform(m * 3, -1.0, 1.0).reshape(m, 3)
        lidx = (r.u64(2 * n) % np.uint64(m)).astype(np.uint32)
        LP = api.make_line_params(mv, pr, 2.0, (size / 2.0, size / 2.0), 0.25)
        sets["lines_indexed"] = dict(kind="lines", P=LP, pts=lpts, idx=lidx, K=6, read=m * 24 + n * 8 + n * 4)

        for name, s in sets.items():
            K = s["K"]
            d_pts = torch.from_numpy(s["pts"]).cuda()
            d_idx = None if s["idx"] is None else torch.from_numpy(s["idx"].view(np.int32)).cuda()
            out = (torch.empty((2 * n, 12), dtype=torch.float64, device="cuda"), torch.empty((2 * n, K), dtype=torch.float64, device="cuda"),
                   torch.empty(2 * n, dtype=torch.int32, device="cuda"))
            write = n * (192 + 16 * K + 8)
            half = (s["read"] + write) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if s["kind"] == "sprites":
                stage = lambda: ctx.sprite_stage(s["P"], d_pts, d_col, device=True, out=out)
                twin = lambda: api.sprite_stage(s["P"], s["pts"], col)
            else:
                stage = lambda: ctx.line_stage(s["P"], d_pts, d_idx, d_col, device=True, out=out)
                twin = lambda: api.line_stage(s["P"], s["pts"], s["idx"], col)

            def copy():
                with torch.cuda.stream(stream):
                    dst.copy_(src)

            rr = dict(K=K, read_bytes=s["read"], write_bytes=write)
            rr["ab"] = alternate(dict(stage=stage, copy=copy))
            ctx.sync()
            want = twin()                                            # what was timed computes the host twin's bytes
            for o, w_ in zip(out, want):
                assert np.array_equal(o.cpu().numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(w_).view(np.uint8).reshape(-1)), name

            def route():
                rows = twin()
                return [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in rows]

            rr["c"] = host_ms(route, 3)
            res[name] = rr
            print(name, json.dumps(rr), flush=True)

            if name == "sprites_attr0":                              # ---- (d) ----
                def chain():
                    q = ctx.sprite_stage(s["P"], d_pts, d_col, device=True, out=out)
                    d = ctx.triangle_depths(q[0], 2, 0, device=True)
                    o = ctx.depth_order(d, device=True)
                    ctx.draw(over, q[0], colors=q[2], device=True, order=o, order_device=True, group=2)
                    ctx.flush()
                    return o

                ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); o = chain(); fb0, st0 = ctx.read_framebuffer(), ctx.stats()
                with torch.cuda.stream(stream):
                    rows = (o.long()[:, None] * 2 + torch.arange(2, device="cuda")[None, :]).reshape(-1)
                    s_clip, s_col = out[0][rows].contiguous(), out[2][rows].contiguous()
                ctx.sync()

                def presorted():
                    ctx.draw(over, s_clip, colors=s_col, device=True)
                    ctx.flush()

                ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); presorted(); fb1, st1 = ctx.read_framebuffer(), ctx.stats()
                assert np.array_equal(fb0, fb1) and st0 == st1, "the chain and the draw of sorted rows differ"
                for rep in range(2):                                 # the two alternate: two rounds each, the second is reported
                    res["d"] = dict(chain=host_ms(chain, a.reps, True), presorted=host_ms(presorted, a.reps, True), fragments=st0[1])
                print("d", json.dumps(res["d"]), flush=True)
                del s_clip, s_col, rows
            del d_pts, d_idx, out, src, dst
            ctx._keep.clear()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--points", str(a.points), "--reps", str(a.reps)],
                       capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("sprite_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    tbs = lambda nbytes, v: nbytes / (v["median_ms"] * 1e-3) / 1e12
    n = res["n"]
    lines = ["point sprites and wide lines, one MI355X, one run on %s, %d primitives, %d x %d frame" % (time.strftime("%Y-%m-%d"), n, res["size"], res["size"]),
             "medians (min .. max) after a warm-up; (a), (b) HIP events on the context's stream, (c), (d) the host clock around calls + sync"]
    for name, what in (("sprites_attr0", "sprites, rows of 4 doubles, K = 6, colours"), ("sprites_attr2", "sprites, rows of 6 doubles, K = 8, colours"),
                       ("lines_indexed", "indexed segments over n / 2 points, K = 6, colours")):
        rr = res[name]
        tot = rr["read_bytes"] + rr["write_bytes"]
        st, cp = rr["ab"]["stage"], rr["ab"]["copy"]
        lines.append("%s: %s; reads %d and writes %d bytes per primitive" % (name, what, rr["read_bytes"] // n, rr["write_bytes"] // n))
        lines.append("(a) the stage kernel      %s  %.2f TB/s read + written" % (fmt(st), tbs(tot, st)))
        lines.append("(b) copy of as many bytes %s  ratio (a) / (b) %.3f" % (fmt(cp), st["median_ms"] / cp["median_ms"]))
        lines.append("(c) host twin + upload    %s  %.0f x (a)" % (fmt(rr["c"]), rr["c"]["median_ms"] / st["median_ms"]))
    ch, ps = res["d"]["chain"], res["d"]["presorted"]
    lines.append("(d) blended frame of the sprites_attr0 set, %d fragments drawn" % res["d"]["fragments"])
    lines.append("    sprite stage, depths, order, ordered draw, flush  %s" % fmt(ch))
    lines.append("    trgl_draw of expanded and sorted rows, flush      %s  ratio %.3f, difference %.3f ms" % (
        fmt(ps), ch["median_ms"] / ps["median_ms"], ch["median_ms"] - ps["median_ms"]))
    lines += ["notes: every repetition reads and writes the same arrays; the outputs of a set (up to 0.33 GB) exceed the 256 MiB Infinity Cache, the",
              "inputs do not.  The project's yardstick for a row-moving kernel is the ordered gather at 1.46 x its copy",
              "(profiles/triangle_order_probe_summary.txt)."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
