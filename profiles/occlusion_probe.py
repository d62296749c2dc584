"""Times of the occlusion queries on one MI355X (DESIGN.md §6 "Occlusion culling of boxes" records the results).

  python profiles/occlusion_probe.py [--size 4096] [--reps 30] [--limit 600] [--out profiles/occlusion_probe_summary.txt]

A --size x --size frame whose depths are a full-screen quad at z = -0.9 with 4000 random triangles in front of and behind it.  Timed
with HIP events recorded on the context's stream around each call (the calls do not wait; the events do; two untimed copies queued in
front keep the stream busy meanwhile, so that the events bracket device work and not the host's launches), medians over --reps
repetitions after a warm-up, the four calls alternating inside one loop:
  snapshot           trgl_zbuffer_snapshot: one device-to-device copy of the W * H depths - the yardstick (reads and writes W * H * 8 bytes)
  build              trgl_occlusion_boxes with ONE box that step 4 rejects: k_occl_build over the frame plus a one-wave query launch.
                     The build reads the bytes the copy reads and writes 1/64 of what it writes: it must not take longer than the copy.
  hidden_full_frame  1024 boxes that cover the whole frame and are hidden, from device memory: no early exit.  A scan would read 1024
                     frames; the walk reads the level-2 values.  The whole call, build included, must stay below 8 snapshot copies:
                     the probe writes its summary and then fails if it does not.
  small_boxes        100000 boxes of about 16 x 16 pixels from device memory, the build included
Before anything is timed the device codes are compared with the host path's (all small boxes; two of the full-frame boxes, the host
scanning every pixel).  Nothing here is a share of any peak.  The measurement runs in one child process under a time limit of --limit
seconds; the parent never touches the GPU."""
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
    from tinyrenderder_amd.api import FLAT, Context
    if not torch.cuda.is_available():
        raise SystemExit("occlusion_probe: no GPU; there is nothing to measure without one")
    n = a.size
    rng = np.random.default_rng(7)
    quad = np.array([[-1, -1, -0.9, 1, 1, -1, -0.9, 1, 1, 1, -0.9, 1], [-1, -1, -0.9, 1, 1, 1, -0.9, 1, -1, 1, -0.9, 1]], np.float64)
    tris, tcol = scenes.random_triangles(4000, n, n, seed=3, rmin=8, rmax=256)
    V, I4 = scenes.init_viewport(0, 0, n, n), np.eye(4)
    full = np.tile(np.array([[-1.0, -1.0, 0.0, 1.0, 1.0, 0.5]]), (1024, 1))
    c = rng.uniform(-1.0, 1.0, (100000, 3))
    half = np.concatenate([np.full((100000, 2), 16.0 / n), rng.uniform(0.0, 0.05, (100000, 1))], 1)
    small = np.concatenate([c - half, c + half], 1)
    reject = np.array([[0.0, 0.0, 2.0, 0.1, 0.1, 3.0]])
    res = dict(size=n)
    with Context(n, n, 3) as ctx:
        ctx.draw(FLAT, quad, colors=np.full(2, 0xff808080, np.uint32))
        ctx.draw(FLAT, tris, colors=tcol)
        z = ctx.read_zbuffer()
        z[~(z <= -0.9)] = -0.9                               # (a pixel the quad's edge rule left out would make every full-frame box visible)
        ctx.write_zbuffer(z)
        stream = torch.cuda.ExternalStream(ctx.stream)
        d_full, d_small, d_reject = (torch.from_numpy(b).cuda() for b in (full, small, reject))
        torch.cuda.synchronize()
        outs = [ctx.occlusion_boxes(I4, b, device=True) for b in (d_full, d_small, d_reject)]
        ctx.sync()                                           # torch's stream, which copies them to the host, waits for nobody
        got_full, got_small, got_reject = (o.cpu().numpy() for o in outs)
        assert (got_full == api.OCCL_HIDDEN).all() and np.array_equal(got_full[:2], api.occlusion_boxes_image(z, V, I4, full[:2]))
        assert np.array_equal(got_small, api.occlusion_boxes_image(z, V, I4, small))
        assert got_reject.tolist() == [api.OCCL_OUTSIDE]
        res["small_codes"] = np.bincount(got_small, minlength=4).tolist()

        def event_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream); fn(); e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        calls = dict(snapshot=lambda: ctx.zbuffer_snapshot(0),
                     build=lambda: ctx.occlusion_boxes(I4, d_reject, device=True),
                     hidden_full_frame=lambda: ctx.occlusion_boxes(I4, d_full, device=True),
                     small_boxes=lambda: ctx.occlusion_boxes(I4, d_small, device=True))
        ts = {k: [] for k in calls}
        for rep in range(WARM + a.reps):
            for k, fn in calls.items():                  # alternating: every call sees the same machine
                ms = event_ms(fn)
                if rep >= WARM:
                    ts[k].append(ms)
            ctx.sync()
        for k, v in ts.items():
            res[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
            print(k, json.dumps(res[k]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("occlusion_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    n = res["size"]
    lines = ["occlusion queries, one MI355X, one run on %s: %d x %d frame (%d bytes of depths)" % (time.strftime("%Y-%m-%d"), n, n, n * n * 8),
             "HIP events on the context's stream around each call, median (min .. max) over the repetitions, the four calls alternating"]
    notes = dict(snapshot="one copy of the depths", build="k_occl_build + a one-box query", hidden_full_frame="1024 boxes, build included",
                 small_boxes="100000 boxes, build included; codes HIDDEN/VISIBLE/OUTSIDE/UNDECIDED = %s" % res["small_codes"])
    for k in ("snapshot", "build", "hidden_full_frame", "small_boxes"):
        v = res[k]
        lines.append("%-18s %8.3f ms (%.3f .. %.3f, %d reps)  %s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], v["reps"], notes[k]))
    copy, build, hidden = (res[k]["median_ms"] for k in ("snapshot", "build", "hidden_full_frame"))
    lines.append("(a) build %.3f ms against copy %.3f ms: %s" % (build, copy, "not longer than the copy" if build <= copy else "LONGER than the copy - the requirement is missed"))
    lines.append("(b) 1024 hidden full-frame boxes %.3f ms against 8 copies %.3f ms: %s" %
                 (hidden, 8 * copy, "below 8 copies" if hidden < 8 * copy else "NOT below 8 copies - the requirement is missed"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if hidden >= 8 * copy:
        raise SystemExit("occlusion_probe: 1024 hidden full-frame boxes are not below 8 snapshot copies - the query scans where it should walk")


if __name__ == "__main__":
    main()
