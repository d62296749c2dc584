"""Times of depth-ordered instanced draws on one MI355X (DESIGN.md §6 "Depth-ordered instanced draws" records the results).

  python profiles/instance_order_probe.py [--size 4096] [--instances 100000] [--reps 20] [--limit 600]
                                          [--out profiles/instance_order_probe_summary.txt]

The scene of profiles/instanced_probe.py: a 12-face cube under --instances model matrices on a --size x --size frame.  Medians after a
warm-up, with min and max.
  (a) order     trgl_instance_depths + trgl_depth_order, everything in device memory, against what a caller could do before they
                existed with everything on the device: torch computes the depths (row 2 of model_view times the matrices, then the dot
                with the point), torch.sort(stable=True), then index-gathers of the matrices, the colours and the visibility codes (the
                ordered draw reads through the list, so the new route has no gather).  HIP events on the context's stream around each
                side, two untimed snapshot copies queued in front so that the events bracket device work; the two sides alternate inside
                one loop.  Required: the new route is not slower than the yardstick, within the yardstick's own run-to-run spread.
  (b) draw      one trgl_draw_instanced_ordered + flush + sync against trgl_draw_instanced + flush + sync over arrays the torch route
                has already permuted; the host clock.  Expected: one more 4-byte read per instance, which should not show.
  (c) fragments fragments_drawn and the time of the raster kernel (trgl_raster_user, TRGL_PHASE_RASTER_KERNEL) for an opaque kind that
                may discard, under array order, back to front and front to back.  Reported, not targeted.
Nothing here is a share of any peak.  The measurement runs in one child process under a time limit of --limit seconds; the parent never
touches the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3
CUTOUT = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ (in.color >> 24) < 96u, in.color }; }
"""


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import PHONG, Context, make_uniforms
    if not torch.cuda.is_available():
        raise SystemExit("instance_order_probe: no GPU; there is nothing to measure without one")
    size, n = a.size, a.instances
    rng = np.random.default_rng(11)
    p = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)])
    cube = np.ascontiguousarray(np.concatenate([p, p / np.sqrt(0.75), p[:, :2] + 0.5], 1))
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                     np.uint32)
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, 1.0, 1.0, 30.0)
    u = make_uniforms(mv)
    centres = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-4.0, -2.0, n)], 1)
    side = 0.01
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10]] = side
    inst[:, 15] = 1.0
    inst[:, [3, 7, 11]] = centres
    colors = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    point = np.zeros(3)
    res = dict(size=size, instances=n)
    with Context(size, size, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        d_cube, d_faces = torch.from_numpy(cube).cuda(), torch.from_numpy(faces.view(np.int32)).cuda()
        d_inst, d_col = torch.from_numpy(inst).cuda(), torch.from_numpy(colors.view(np.int32)).cuda()
        d_codes = torch.ones(n, dtype=torch.uint8, device="cuda")
        d_row, d_point = torch.from_numpy(mv[2].copy()).cuda(), torch.from_numpy(point).cuda()
        torch.cuda.synchronize()
        ctx.zbuffer_snapshot(1)

        # ---- (a) ----
        def event_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream); out = fn(); e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        def new_route():
            d = ctx.instance_depths(mv, point, d_inst, device=True)
            return ctx.depth_order(d, device=True)

        def torch_route():
            with torch.cuda.stream(stream):
                r = torch.matmul(d_row, d_inst.view(n, 4, 4))                       # [n, 4]: row 2 of model_view * M
                d = r[:, :3] @ d_point + r[:, 3]
                idx = torch.sort(d, stable=True).indices
                return idx, d_inst[idx], d_col[idx], d_codes[idx]

        sides = dict(new=new_route, torch=torch_route)
        ts = {k: [] for k in sides}
        last = {}
        for rep in range(WARM + a.reps):
            for k, fn in sides.items():
                ms, last[k] = event_ms(fn)
                if rep >= WARM:
                    ts[k].append(ms)
            ctx.sync()
            ctx._keep.clear()                                     # (the tensors of the untimed repetitions)
        order = last["new"]
        sorted_inst, sorted_col = last["torch"][1], last["torch"][2]
        # what was timed computes the right thing: the list sorts the model's depths, ties ascending
        o = order.cpu().numpy().view(np.uint32).astype(np.int64)
        r2 = [(((0.0 + mv[2, 0] * inst[:, c]) + mv[2, 1] * inst[:, 4 + c]) + mv[2, 2] * inst[:, 8 + c]) + mv[2, 3] * inst[:, 12 + c] for c in range(4)]
        d = (((0.0 + r2[0] * point[0]) + r2[1] * point[1]) + r2[2] * point[2]) + r2[3] * 1.0
        assert sorted(o.tolist()) == list(range(n)) and (np.diff(d[o]) >= 0).all() and (np.diff(o)[np.diff(d[o]) == 0] > 0).all(), "the order is not the model's"
        for k, v in ts.items():
            res["order_" + k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
            print("order", k, json.dumps(res["order_" + k]), flush=True)

        # ---- (b) ----
        def host_ms(fn, reps):
            v = []
            for rep in range(WARM + reps):
                ctx.clear((0, 0, 0, 255), np.inf); ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync()
                if rep >= WARM:
                    v.append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))

        def ordered_draw(kind=PHONG, o=order, col=None):
            ctx.draw_instanced(kind, u, proj, d_cube, d_faces, instances=d_inst, instance_colors=col, device=True, instances_device=True,
                               order=o, order_device=True)
            ctx.flush()

        def presorted_draw():
            ctx.draw_instanced(PHONG, u, proj, d_cube, d_faces, instances=sorted_inst, device=True, instances_device=True)
            ctx.flush()

        for rep in range(2):                                      # the two alternate: two rounds each, the second is reported
            res["draw_ordered"] = host_ms(ordered_draw, a.reps)
            res["draw_presorted"] = host_ms(presorted_draw, a.reps)
        # and they draw the same frame
        ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); ordered_draw(); fb0, st0 = ctx.read_framebuffer(), ctx.stats()
        ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); presorted_draw(); fb1, st1 = ctx.read_framebuffer(), ctx.stats()
        assert np.array_equal(fb0, fb1) and st0 == st1, "the ordered draw and the draw of permuted arrays differ"
        print("draw ordered", json.dumps(res["draw_ordered"]), flush=True)
        print("draw presorted", json.dumps(res["draw_presorted"]), flush=True)

        # ---- (c) ----
        cutout = ctx.register_shader(CUTOUT, 24, True)
        front = ctx.depth_order(ctx.instance_depths(mv, point, d_inst, device=True), front_to_back=True, device=True)
        ctx.sync()
        keep = (order, front)
        ctx.set_profiling(True)
        for name, o in (("array", None), ("back_to_front", order), ("front_to_back", front)):
            v = []
            frags = None
            for rep in range(WARM + a.reps):
                ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); ctx.reset_phase_ms()
                if o is None:
                    ctx.draw_instanced(cutout, u, proj, d_cube, d_faces, instances=d_inst, instance_colors=d_col, device=True, instances_device=True)
                    ctx.flush()
                else:
                    ordered_draw(cutout, o, d_col)
                ctx.sync()
                frags = ctx.stats()[1]
                if rep >= WARM:
                    v.append(ctx.phase_ms()[0][api.PHASE_RASTER_KERNEL])
                ctx._keep.clear()
            res["frag_" + name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v), fragments_drawn=frags)
            print("fragments", name, json.dumps(res["frag_" + name]), flush=True)
        ctx.set_profiling(False)
        del keep
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--instances", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--instances", str(a.instances), "--reps", str(a.reps)],
                       capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("instance_order_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    n, size = res["instances"], res["size"]
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["depth-ordered instanced draws, one MI355X, one run on %s: a 12-face cube under %d matrices, %d x %d frame" % (time.strftime("%Y-%m-%d"), n, size, size),
             "medians (min .. max) after a warm-up; (a) HIP events on the context's stream, (b) the host clock around call + flush + sync, (c) the raster kernel's events"]
    on, ot = res["order_new"], res["order_torch"]
    spread = ot["max_ms"] - ot["min_ms"]
    ok = on["median_ms"] <= ot["median_ms"] + spread
    lines.append("(a) depths + order      %s  k_instance_depths, k_order_keys, the radix sort of 64-bit keys" % fmt(on))
    lines.append("    torch route         %s  matmul + dot, torch.sort(stable=True), gathers of matrices, colours, codes" % fmt(ot))
    lines.append("    ratio %.3f, the yardstick's own spread %.3f ms: %s" % (on["median_ms"] / ot["median_ms"], spread,
                 "not slower" if ok else "SLOWER than the yardstick - the requirement is missed"))
    do, dp = res["draw_ordered"], res["draw_presorted"]
    lines.append("(b) ordered draw        %s  trgl_draw_instanced_ordered through the device list" % fmt(do))
    lines.append("    pre-sorted arrays   %s  trgl_draw_instanced over the arrays the torch route permuted; ratio %.3f" % (fmt(dp), do["median_ms"] / dp["median_ms"]))
    for i, name in enumerate(("array", "back_to_front", "front_to_back")):
        v = res["frag_" + name]
        lines.append("%s %-19s %s  fragments_drawn %d" % ("(c)" if i == 0 else "   ", name.replace("_", " "), fmt(v), v["fragments_drawn"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
