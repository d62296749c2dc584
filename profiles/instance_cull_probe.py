"""Times of trgl_instance_boxes and trgl_frustum_boxes on one MI355X (DESIGN.md §6 "World boxes and frustum codes" records the results).

  python profiles/instance_cull_probe.py [--size 4096] [--instances 100000,1000000] [--reps 20] [--limit 900]
                                         [--out profiles/instance_cull_probe_summary.txt]

A 12-face cube of side 0.01 under --instances model matrices (instance_stride 16) scattered over a region wider than the view, so that
the frustum culls a share of them; a --size x --size frame.  Medians after a warm-up, with min and max.  Each size is measured: at
100 000 instances kernels of this size are launch-bound, at 1 000 000 they show what they do to memory.
  (a) kernels   k_instance_boxes and k_frustum_boxes (SET, and MERGE) against a device-to-device copy that moves as many bytes as the
                kernel does - bytes read plus bytes written: n x (128 + 48) for the boxes, n x (48 + 1) for the codes - so the copy's
                source is half that long.  HIP events on the context's stream around BATCH launches of one kind, two untimed snapshot
                copies queued in front so that the events bracket device work; the time is per launch.  The sides alternate in one loop.
                Under MERGE the kernel reads no code byte (it writes only the bytes of culled boxes), so its copy stays the same.
  (b) calls     the two device calls together (events, as above) against the route a caller has without them: the library's own host
                loops over the matrices - the array calls with TRGL_MEM_HOST, which are the single-box calls' arithmetic without their
                per-call overhead, so a lower bound for that route - and the upload of the boxes and the codes (pageable numpy arrays,
                torch's copy, then a synchronise); the host clock.
  (c) chain     the whole chain of examples/demo_instance_cull.cpp - boxes, occlusion codes, frustum codes merged in, depths, order,
                the ordered instanced draw, flush, sync - against the same chain with the boxes and the frustum codes made on the host
                and uploaded (the merge then is one torch.where on the context's stream); the host clock.
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
BATCH = 20


def stat(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))


def measure(a, n):
    import numpy as np
    import torch
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import PHONG, Context, make_uniforms
    size = a.size
    rng = np.random.default_rng(11)
    p = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)])
    cube = np.ascontiguousarray(np.concatenate([p, p / np.sqrt(0.75), p[:, :2] + 0.5], 1))
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                     np.uint32)
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, 1.0, 1.0, 30.0)
    u = make_uniforms(mv)
    view_proj = np.zeros((4, 4))
    for k in range(4):                                            # geometry.h:196-205
        view_proj = view_proj + proj[:, k:k + 1] * mv[k:k + 1, :]
    planes = api.frustum_from_matrix(np.ascontiguousarray(view_proj.T))      # the camera's planes (our_gl.cpp:217-250 reads columns)
    centres = np.stack([rng.uniform(-9.0, 9.0, n), rng.uniform(-9.0, 9.0, n), rng.uniform(-4.0, -2.0, n)], 1)
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10]] = 0.01
    inst[:, 15] = 1.0
    inst[:, [3, 7, 11]] = centres
    local = np.concatenate(api.mesh_bounds(cube))
    point = np.zeros(3)
    res = dict(size=size, instances=n)
    with Context(size, size, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        d_cube, d_faces = torch.from_numpy(cube).cuda(), torch.from_numpy(faces.view(np.int32)).cuda()
        d_inst = torch.from_numpy(inst).cuda()
        d_boxes = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        d_codes = torch.empty(n, dtype=torch.uint8, device="cuda")
        src_b, dst_b = (torch.empty(n * (128 + 48) // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        src_c, dst_c = (torch.empty((n * (48 + 1) + 1) // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        ctx.zbuffer_snapshot(1)

        def event_ms(fn, batch=1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream)
            for _ in range(batch):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / batch

        def copy(dst, src):
            with torch.cuda.stream(stream):
                dst.copy_(src)

        # ---- (a) ----
        ctx.instance_boxes(local, d_inst, out=d_boxes)
        sides = {
            "boxes_kernel": lambda: ctx.instance_boxes(local, d_inst, out=d_boxes),
            "boxes_copy": lambda: copy(dst_b, src_b),
            "codes_set_kernel": lambda: ctx.frustum_boxes(planes, d_boxes, d_codes),
            "codes_merge_kernel": lambda: ctx.frustum_boxes(planes, d_boxes, d_codes, merge=True),
            "codes_copy": lambda: copy(dst_c, src_c),
        }
        ts = {k: [] for k in sides}
        for rep in range(WARM + a.reps):
            for k, fn in sides.items():
                ms = event_ms(fn, BATCH)
                if rep >= WARM:
                    ts[k].append(ms)
            ctx.sync()
            ctx._keep.clear()
        for k, v in ts.items():
            res[k] = stat(v)
            print(n, k, json.dumps(res[k]), flush=True)

        # ---- (b) ----
        def device_calls():
            ctx.instance_boxes(local, d_inst, out=d_boxes)
            ctx.frustum_boxes(planes, d_boxes, d_codes)

        def host_route():
            boxes = api.instance_boxes(local, inst)
            codes = api.frustum_boxes(planes, boxes)
            db, dc = torch.from_numpy(boxes).cuda(), torch.from_numpy(codes).cuda()
            torch.cuda.synchronize()
            return boxes, codes, db, dc

        dev, host = [], []
        for rep in range(WARM + a.reps):
            ms = event_ms(device_calls, BATCH)
            t0 = time.perf_counter(); h_boxes, h_codes, _, _ = host_route(); hms = (time.perf_counter() - t0) * 1e3
            if rep >= WARM:
                dev.append(ms); host.append(hms)
            ctx._keep.clear()
        ctx.sync()
        # what was timed computes the same thing
        assert np.array_equal(d_boxes.cpu().numpy().view(np.uint64), h_boxes.view(np.uint64)), "device boxes differ from the host path"
        assert np.array_equal(d_codes.cpu().numpy(), h_codes), "device codes differ from the host path"
        res["calls_device"], res["calls_host"] = stat(dev), stat(host)
        res["culled"] = int((h_codes == api.OCCL_OUTSIDE).sum())
        print(n, "calls device", json.dumps(res["calls_device"]), flush=True)
        print(n, "calls host", json.dumps(res["calls_host"]), flush=True)

        # ---- (c) ----
        def draw(codes):
            order = ctx.depth_order(ctx.instance_depths(mv, point, d_inst, device=True), front_to_back=True, device=True)
            ctx.draw_instanced(PHONG, u, proj, d_cube, d_faces, instances=d_inst, visible=codes, device=True, instances_device=True,
                               order=order, order_device=True)
            ctx.flush()

        def device_chain():
            boxes = ctx.instance_boxes(local, d_inst, out=d_boxes)
            codes = ctx.occlusion_boxes(view_proj, boxes, device=True)
            ctx.frustum_boxes(planes, boxes, codes, merge=True)
            draw(codes)

        def host_chain():
            boxes = api.instance_boxes(local, inst)
            frustum = api.frustum_boxes(planes, boxes)
            db, df = torch.from_numpy(boxes).cuda(), torch.from_numpy(frustum).cuda()
            torch.cuda.synchronize()                              # torch's stream is not the context's
            codes = ctx.occlusion_boxes(view_proj, db, device=True)
            with torch.cuda.stream(stream):
                codes = torch.where(df == api.OCCL_OUTSIDE, df, codes)
            draw(codes)

        def host_ms(fn):
            v = []
            for rep in range(WARM + a.reps):
                ctx.clear((0, 0, 0, 255), np.inf); ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync()
                if rep >= WARM:
                    v.append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return stat(v)

        res["chain_device"], res["chain_host"] = host_ms(device_chain), host_ms(host_chain)
        ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); device_chain(); fb0, st0 = ctx.read_framebuffer(), ctx.stats()
        ctx.clear((0, 0, 0, 255), np.inf); ctx.reset_stats(); host_chain(); fb1, st1 = ctx.read_framebuffer(), ctx.stats()
        assert np.array_equal(fb0, fb1) and st0 == st1, "the two chains draw different frames"
        res["drawn"] = (st0[0]) // 12
        print(n, "chain device", json.dumps(res["chain_device"]), flush=True)
        print(n, "chain host", json.dumps(res["chain_host"]), flush=True)
    return res


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("instance_cull_probe: no GPU; there is nothing to measure without one")
    out = [measure(a, int(n)) for n in a.instances.split(",")]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--instances", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--instances", a.instances, "--reps", str(a.reps)],
                       capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("instance_cull_probe: the measurement failed (%d)" % r.returncode)
    results = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.4f ms (%.4f .. %.4f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["world boxes and frustum codes of instances, one MI355X, one run on %s: a 12-face cube, instance_stride 16, %d x %d frame"
             % (time.strftime("%Y-%m-%d"), results[0]["size"], results[0]["size"]),
             "medians (min .. max) after a warm-up; (a) HIP events around %d launches, per launch; (b) events against the host clock; (c) the host clock around chain + flush + sync" % BATCH,
             "kept: one thread per instance, no LDS staging (a lane's 128 bytes are cache lines of its own; see the ratios of (a) at 1000000)"]
    for res in results:
        n = res["instances"]
        lines.append("---- %d instances (%d culled by the frustum, %d drawn) ----" % (n, res["culled"], res["drawn"]))
        bk, bc = res["boxes_kernel"], res["boxes_copy"]
        lines.append("(a) k_instance_boxes    %s  %d bytes read + written, %.0f GB/s" % (fmt(bk), n * 176, n * 176 / bk["median_ms"] / 1e6))
        lines.append("    copy of as many     %s  ratio %.2f" % (fmt(bc), bk["median_ms"] / bc["median_ms"]))
        cs, cm, cc = res["codes_set_kernel"], res["codes_merge_kernel"], res["codes_copy"]
        lines.append("    k_frustum_boxes SET %s  %d bytes read + written, %.0f GB/s" % (fmt(cs), n * 49, n * 49 / cs["median_ms"] / 1e6))
        lines.append("    ... MERGE           %s  (reads no code byte, writes the culled ones)" % fmt(cm))
        lines.append("    copy of as many     %s  ratio %.2f (SET), %.2f (MERGE)" % (fmt(cc), cs["median_ms"] / cc["median_ms"], cm["median_ms"] / cc["median_ms"]))
        cd, ch = res["calls_device"], res["calls_host"]
        lines.append("(b) the two device calls %s" % fmt(cd))
        lines.append("    host loops + upload %s  ratio %.0f" % (fmt(ch), ch["median_ms"] / cd["median_ms"]))
        hd, hh = res["chain_device"], res["chain_host"]
        lines.append("(c) chain on the device %s  boxes, occlusion, frustum MERGE, depths, order, ordered draw" % fmt(hd))
        lines.append("    boxes + frustum on the host %s  ratio %.2f" % (fmt(hh), hh["median_ms"] / hd["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
