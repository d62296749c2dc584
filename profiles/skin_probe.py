"""Times of the skin stage and of the palette composition on one MI355X (DESIGN.md §6 "Skeletal animation" records the results).

  python profiles/skin_probe.py [--vertices 1000000] [--reps 20] [--limit 900] [--out profiles/skin_probe_summary.txt]

Sets: --vertices vertices at stride 14 with 4 influences and all three flags under 64 and under 1024 joints (the palette staged in LDS
and read through the cache), the same at stride 8 with TRGL_SKIN_NORMAL, two variants of the first that show where its time goes (no
flags; one influence), 10 000 poses of a 1 000-vertex mesh (stride 14, 64 joints), and trgl_pose_palette for 10 000 poses of 64 joints
in a chain, with inverse bind matrices.  Medians after a warm-up, with min and max.
  (a) the kernel (k_skin_stage / k_pose_palette), HIP events on the context's stream
  (b) a device-to-device copy that reads and writes as many bytes together as the call reads once plus writes, timed the same way and
      alternating with (a) inside one loop; the ratio (a) / (b) is recorded
  (c) the route the call replaces: the host twin, then an upload of its output; the host clock around both and a synchronise
What was timed is compared with the host twin's bytes first.  Two untimed snapshot copies are queued in front of (a) and (b) so that the
events bracket device work.  The measurement runs in one child process under a time limit of --limit seconds; the parent never touches
the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import Context
    if not torch.cuda.is_available():
        raise SystemExit("skin_probe: no GPU; there is nothing to measure without one")
    res = dict(n=a.vertices)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    with Context(64, 64, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
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

        def host_ms(fn, reps):
            v = []
            for rep in range(1 + reps):
                ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync(); torch.cuda.synchronize()
                if rep >= 1:
                    v.append((time.perf_counter() - t0) * 1e3)
            return stat(v)

        def rigid(r, n):
            ang = r.uniform(n, -1.0, 1.0)
            m = np.zeros((n, 16))
            m[:, 0], m[:, 1], m[:, 4], m[:, 5], m[:, 10], m[:, 15] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0, 1.0
            m[:, [3, 7, 11]] = r.uniform(3 * n, -0.5, 0.5).reshape(n, 3)
            return m

        def measure(name, call, twin, out, read, write, twin_reps=3):
            half = (read + write) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def copy():
                with torch.cuda.stream(stream):
                    dst.copy_(src)

            rr = dict(read_bytes=read, write_bytes=write)
            rr["ab"] = alternate(dict(stage=call, copy=copy))
            ctx.sync()
            want = twin()                                            # what was timed computes the host twin's bytes
            assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(-1), np.ascontiguousarray(want).view(np.uint64).reshape(-1)), name
            rr["c"] = host_ms(lambda: torch.from_numpy(twin()).cuda(), twin_reps)
            res[name] = rr
            print(name, json.dumps(rr), flush=True)

        r = scenes.SplitMix64(77)
        for name, n, stride, flags, nj, poses, k in (("s14_j64", a.vertices, 14, 7, 64, 1, 4), ("s14_j1024", a.vertices, 14, 7, 1024, 1, 4),
                                                     ("s8_j64", a.vertices, 8, 1, 64, 1, 4), ("s8_j1024", a.vertices, 8, 1, 1024, 1, 4),
                                                     ("s14_j64_noflags", a.vertices, 14, 0, 64, 1, 4), ("s14_j64_k1", a.vertices, 14, 7, 64, 1, 1),
                                                     ("poses10000", 1000, 14, 7, 64, 10000, 4)):
            v = r.uniform(n * stride, -1.0, 1.0).reshape(n, stride)
            w = r.uniform(n * k, 0.0, 1.0).reshape(n, k)
            w /= w.sum(axis=1, keepdims=True)
            j = (r.u64(n * k) % np.uint64(nj)).astype(np.uint16).reshape(n, k)
            pal = rigid(r, poses * nj).reshape(poses, nj, 16)
            d_v, d_w, d_pal = torch.from_numpy(v).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(pal).cuda()
            d_j = torch.from_numpy(j.view(np.int16)).cuda()
            out = torch.empty((poses, n, stride), dtype=torch.float64, device="cuda")
            read = n * (stride * 8 + k * 10) + poses * nj * 96      # rows 0 .. 2 of every matrix
            measure(name, lambda: ctx.skin_stage(d_v, d_j, d_w, d_pal, flags, device=True, out=out),
                    lambda: api.skin_stage(v, j, w, pal, flags), out, read, poses * n * stride * 8, twin_reps=2 if poses > 1 else 3)
            del d_v, d_w, d_pal, d_j, out
            ctx._keep.clear()

        poses, nj = 10000, 64
        parents = np.arange(-1, nj - 1).astype(np.int32)
        loc, ib = rigid(r, poses * nj).reshape(poses, nj, 16), rigid(r, nj)
        d_par, d_loc, d_ib = torch.from_numpy(parents).cuda(), torch.from_numpy(loc).cuda(), torch.from_numpy(ib).cuda()
        out = torch.empty((poses, nj, 16), dtype=torch.float64, device="cuda")
        measure("palette10000", lambda: ctx.pose_palette(d_par, d_loc, d_ib, device=True, out=out), lambda: api.pose_palette(parents, loc, ib), out,
                poses * nj * 128 + nj * 132, poses * nj * 128)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--vertices", str(a.vertices), "--reps", str(a.reps)],
                       capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("skin_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    tbs = lambda nbytes, v: nbytes / (v["median_ms"] * 1e-3) / 1e12
    n = res["n"]
    lines = ["skeletal animation, one MI355X, one run on %s, %d vertices with 4 influences unless noted" % (time.strftime("%Y-%m-%d"), n),
             "medians (min .. max) after a warm-up; (a), (b) HIP events on the context's stream, (c) the host clock around calls + sync"]
    for name, what in (("s14_j64", "stride 14, normal + tangent + bitangent, 64 joints (palette in LDS), 1 pose"),
                       ("s14_j1024", "stride 14, normal + tangent + bitangent, 1024 joints (palette through the cache), 1 pose"),
                       ("s8_j64", "stride 8, normal, 64 joints, 1 pose"), ("s8_j1024", "stride 8, normal, 1024 joints, 1 pose"),
                       ("s14_j64_noflags", "where the time goes: s14_j64 without flags (positions only: no square root, no division)"),
                       ("s14_j64_k1", "where the time goes: s14_j64 with 1 influence in place of 4 (a quarter of the joint and weight loads and blends)"),
                       ("poses10000", "10000 poses of a 1000-vertex mesh, stride 14, all flags, 64 joints"),
                       ("palette10000", "trgl_pose_palette: 10000 poses of a chain of 64 joints, with inverse bind matrices")):
        rr = res[name]
        tot = rr["read_bytes"] + rr["write_bytes"]
        st, cp = rr["ab"]["stage"], rr["ab"]["copy"]
        lines.append("%s: %s; reads %d and writes %d bytes" % (name, what, rr["read_bytes"], rr["write_bytes"]))
        lines.append("(a) the kernel            %s  %.2f TB/s read + written" % (fmt(st), tbs(tot, st)))
        lines.append("(b) copy of as many bytes %s  ratio (a) / (b) %.3f" % (fmt(cp), st["median_ms"] / cp["median_ms"]))
        lines.append("(c) host twin + upload    %s  %.0f x (a)" % (fmt(rr["c"]), rr["c"]["median_ms"] / st["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
