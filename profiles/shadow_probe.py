"""Times of the shadow post-pass on one MI355X (DESIGN.md §6 "Shadow post-pass" records the results).

  python profiles/shadow_probe.py [--size 4096] [--reps 30] [--limit 600] [--kernel-trace] [--out profiles/shadow_probe_summary.txt]

The head stand-in (scenes.head_standin, level 6) over a floor, drawn at --size x --size from a light along the key direction
(main.cpp:615) - its depths become the snapshot, a --size x --size light map - and then from the stand-in's own camera.  Timed, each as
the call followed by a sync, by the host clock, medians over --reps repetitions after a warm-up:
  shadow_mask r0 / r2    trgl_shadow_mask into a device mask at pcf_radius 0 and 2
  framebuffer_modulate   trgl_framebuffer_modulate by that mask
  postprocess_ao         trgl_postprocess with only the AO map asked for, for scale: k_ssao plus the 3 * W * H bytes to the host
Each device mask is compared with the host path before anything is timed.  algorithmic bytes: W * H * (8 + 1) + 8 per live pixel and tap
for the mask (live: the pixels that reach step 7, counted on the host), W * H * (1 + 2 * bpp) for modulate; bytes / median is printed as
GB/s and is NOT a share of any peak.
The measurement runs in one child process under a time limit of --limit seconds; the parent never touches the GPU.  With
--kernel-trace the parent then runs the same child once more under `rocprofv3 --kernel-trace --stats` (its own process, its own
time limit), reads the trace's CSV and adds the durations of k_shadow_mask (per radius), k_modulate and k_ssao - medians over the
launches behind each call's check and warm-up launches - to the summary: kernel times come from that run, call times from the run
without the profiler."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3      # warm-up calls of timed(); the child makes one checked call in front of them


def timed(fn, reps, warm=WARM):
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if k >= warm:
            ts.append(dt)
    return dict(median_ms=statistics.median(ts) * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, reps=reps)


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import FLAT, Context
    if not torch.cuda.is_available():
        raise SystemExit("shadow_probe: no GPU; there is nothing to measure without one")
    n = a.size
    hd = scenes.head_standin(6, n, n)
    floor = np.array([[[-3.0, -1.1, 3.0], [3.0, -1.1, 3.0], [3.0, -1.1, -3.0]], [[-3.0, -1.1, 3.0], [3.0, -1.1, -3.0], [-3.0, -1.1, -3.0]]])
    pos = np.concatenate([hd["positions"], floor], 0)
    colors = np.full(pos.shape[0], 0xffc0c0c0, np.uint32)
    key = hd["world_lights"]["key"]
    views = dict(light=(scenes.lookat(tuple(key * 4.0), (0, 0, 0), (0, 1, 0)), scenes.perspective(0.5, 1.0, 0.5, 50.0)),
                 cam=(hd["model_view"], hd["projection"]))
    vp = scenes.init_viewport(0, 0, n, n)

    def clip_of(mv, proj):
        e = scenes._matvec(mv, pos[..., 0], pos[..., 1], pos[..., 2], 1.0)
        return np.ascontiguousarray(np.stack(scenes._matvec(proj, *e), -1).reshape(pos.shape[0], 12))

    M = api.shadow_matrix(views["light"][0], views["light"][1], vp, views["cam"][0], views["cam"][1], vp)
    res = dict(size=n, triangles=int(pos.shape[0]))
    with Context(n, n, 3) as ctx:
        ctx.draw(FLAT, clip_of(*views["light"]), colors=colors)
        zl = ctx.read_zbuffer()
        ctx.zbuffer_snapshot(1)
        ctx.clear()
        ctx.draw(FLAT, clip_of(*views["cam"]), colors=colors)
        zc, fb = ctx.read_zbuffer(), ctx.read_framebuffer()
        # the pixels that reach step 7: against a map of -inf every one of them is fully occluded
        probe_map = np.full(zl.shape, -np.inf)
        live = int((api.shadow_mask_image(api.make_shadow_params(M, 0.0, 1.0, 0), zc, probe_map) == 0).sum())
        res.update(finite_depths=int(np.isfinite(zc).sum()), live_pixels=live, light_map_finite=int(np.isfinite(zl).sum()))
        mask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        for r in (0, 2):
            p = api.make_shadow_params(M, 2e-3, 0.6, r)
            ctx.shadow_mask(p, slot=1, out=mask, device=True); ctx.sync()
            got = mask.cpu().numpy()
            assert np.array_equal(got, api.shadow_mask_image(p, zc, zl)), r
            t = timed(lambda: (ctx.shadow_mask(p, slot=1, out=mask, device=True), ctx.sync()), a.reps)
            nbytes = n * n * 9 + 8 * live * (2 * r + 1) ** 2
            res["shadow_mask_r%d" % r] = dict(t, algorithmic_bytes=nbytes, gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9, shadowed_pixels=int((got < 255).sum()))
            print("shadow_mask_r%d" % r, json.dumps(res["shadow_mask_r%d" % r]), flush=True)
        ctx.framebuffer_modulate(mask, device=True)
        assert np.array_equal(ctx.read_framebuffer(), api.image_modulate(fb, mask.cpu().numpy()))
        t = timed(lambda: (ctx.framebuffer_modulate(mask, device=True), ctx.sync()), a.reps)
        nbytes = n * n * (1 + 2 * 3)
        res["framebuffer_modulate"] = dict(t, algorithmic_bytes=nbytes, gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9)
        print("framebuffer_modulate", json.dumps(res["framebuffer_modulate"]), flush=True)
        res["postprocess_ao"] = dict(timed(lambda: ctx.postprocess(zbuffer_image=False, ao=True, final=False), max(3, a.reps // 3), warm=2),
                                     note="k_ssao + %d bytes to the host" % (3 * n * n))
        print("postprocess_ao", json.dumps(res["postprocess_ao"]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def kernel_times(a):
    """The child once more under rocprofv3; per kernel the launches in time order, without each call's check and warm-up launches."""
    import csv
    import glob
    import tempfile
    out = tempfile.mkdtemp(prefix="shadow_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
           sys.executable, __file__, "--child", "--size", str(a.size), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("shadow_probe: the run under rocprofv3 failed (%d)" % r.returncode)
    rows = []
    for path in glob.glob(out + "/**/*kernel_trace.csv", recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                k = {name.lower(): v for name, v in row.items()}
                rows.append((int(k["start_timestamp"]), k["kernel_name"], (int(k["end_timestamp"]) - int(k["start_timestamp"])) / 1e3))
    rows.sort()
    of = lambda key: [us for _, name, us in rows if key in name]
    per = 1 + WARM + a.reps
    mask, mod, ssao = of("k_shadow_mask"), of("k_modulate"), of("k_ssao")
    picks = [("k_shadow_mask r0", mask[1 + WARM:per]), ("k_shadow_mask r2", mask[per + 1 + WARM:2 * per]),
             ("k_modulate", mod[1 + WARM:per]), ("k_ssao", ssao[2:])]
    lines = ["kernel durations of the same child under rocprofv3 --kernel-trace --stats (a separate run; check and warm-up launches left out):"]
    for name, us in picks:
        if not us:
            raise SystemExit("shadow_probe: no launches of %s in the trace" % name)
        lines.append("%-22s %8.1f us (%.1f .. %.1f, %d launches)" % (name, statistics.median(us), min(us), max(us), len(us)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernel-trace", action="store_true", help="add kernel durations from a second run under rocprofv3")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("shadow_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    lines = ["shadow post-pass, one MI355X, one run: %d x %d frame and light map, %d triangles, %d finite depths, %d live pixels" %
             (res["size"], res["size"], res["triangles"], res["finite_depths"], res["live_pixels"]),
             "call + sync by the host clock, median (min .. max) over the repetitions; bytes are the algorithm's, no share of peak is claimed"]
    for k in ("shadow_mask_r0", "shadow_mask_r2", "framebuffer_modulate", "postprocess_ao"):
        v = res[k]
        extra = "  %d bytes, %.0f GB/s" % (v["algorithmic_bytes"], v["gb_per_s"]) if "gb_per_s" in v else "  (%s)" % v["note"]
        lines.append("%-22s %8.3f ms (%.3f .. %.3f, %d reps)%s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], v["reps"], extra))
    if a.kernel_trace:
        lines += kernel_times(a)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
