"""Times of instanced draws on one MI355X (DESIGN.md §6 "Instanced draws" records the results).

  python profiles/instanced_probe.py [--size 4096] [--instances 100000] [--reps 20] [--loop-reps 20] [--limit 900]
                                     [--out profiles/instanced_probe_summary.txt]

A 12-face cube under --instances model matrices on a --size x --size frame, medians after a warm-up.
  (a) stage     the instanced vertex stage (k_inst_mv + k_instance_vertex_stage: trgl_instance_stage, everything in device memory, no
                visibility bytes, so nothing waits) against the yardstick, k_vertex_stage over ONE mesh of instances * 12 faces whose index
                buffer repeats the cube's (the same 8 vertices' worth of locality).  Both write 288 B per face; the instanced one also
                reads 132 B per 12 faces and divides once per thread.  HIP events on the context's stream around each call, two
                untimed snapshot copies queued in front so that the events bracket device work; the two alternate inside one loop.
                Target: within 1.10 x.
  (b) call      one trgl_draw_instanced + flush + sync against the loop it replaces, --instances trgl_draw_indexed calls + flush + sync,
                by the host clock; the flushes each takes.
  (c) occlusion a wall over half the frame, the cubes behind and beside it.  Left: trgl_occlusion_boxes with the codes left in device
                memory, one instanced draw gated by them (its one 8-byte wait), flush, sync.  Right: the same query, the codes copied
                to the host, a host loop of trgl_draw_indexed over the visible instances, flush, sync.  Both start from the wall's
                depths (a snapshot restored in front of each run).
The loop sides take seconds per run; --loop-reps says how many are taken (the summary names the number).  Nothing here is a share of
any peak.  The measurement runs in one child process under a time limit of --limit seconds; the parent never touches the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 2


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api, scenes
    from tinyrenderder_amd.api import FLAT, PHONG, Context, make_uniforms
    if not torch.cuda.is_available():
        raise SystemExit("instanced_probe: no GPU; there is nothing to measure without one")
    size, n = a.size, a.instances
    rng = np.random.default_rng(11)
    p = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)])
    cube = np.ascontiguousarray(np.concatenate([p, p / np.sqrt(0.75), p[:, :2] + 0.5], 1))
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                     np.uint32)
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, 1.0, 1.0, 30.0)
    view_proj = proj @ mv
    u = make_uniforms(mv)
    centres = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-4.0, -2.0, n)], 1)
    side = 0.01
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10]] = side
    inst[:, 15] = 1.0
    inst[:, [3, 7, 11]] = centres
    boxes = np.concatenate([centres - 0.75 * side, centres + 0.75 * side], 1)
    wall_v = np.array([[-8.0, -8.0, 0.0], [0.0, -8.0, 0.0], [0.0, 8.0, 0.0], [-8.0, 8.0, 0.0]])
    eye = wall_v @ mv[:3, :3].T + mv[:3, 3]
    wall = np.concatenate([eye, np.ones((4, 1))], 1) @ proj.T
    wall_clip = np.ascontiguousarray(wall[[0, 1, 2, 0, 2, 3]].reshape(2, 12))
    big_idx = np.ascontiguousarray(np.tile(faces, (n, 1)))
    res = dict(size=size, instances=n)
    with Context(size, size, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        d_cube, d_faces, d_big = torch.from_numpy(cube).cuda(), torch.from_numpy(faces.view(np.int32)).cuda(), torch.from_numpy(big_idx.view(np.int32)).cuda()
        d_inst, d_boxes = torch.from_numpy(inst).cuda(), torch.from_numpy(boxes).cuda()
        out = (torch.empty((n * 12, 12), dtype=torch.float64, device="cuda"), torch.empty((n * 12, 24), dtype=torch.float64, device="cuda"), None)
        ref = (torch.empty((n * 12, 12), dtype=torch.float64, device="cuda"), torch.empty((n * 12, 24), dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        ctx.draw(FLAT, wall_clip, colors=np.full(2, 0xff808080, np.uint32))
        ctx.flush()
        ctx.zbuffer_snapshot(0)
        ctx.zbuffer_snapshot(1)

        # ---- (a) ----
        def event_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.zbuffer_snapshot(1); ctx.zbuffer_snapshot(1)      # keeps the stream busy while the host queues what is timed
            e0.record(stream); fn(); e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        stage = dict(instanced=lambda: ctx.instance_stage(-1, u, proj, d_cube, d_faces, instances=d_inst, device=True, instances_device=True, out=out),
                     yardstick=lambda: ctx.vertex_stage(-1, u, proj, d_cube, d_big, device=True, out=ref))
        ts = {k: [] for k in stage}
        for rep in range(WARM + a.reps):
            for k, fn in stage.items():
                ms = event_ms(fn)
                if rep >= WARM:
                    ts[k].append(ms)
            ctx.sync()
        # what was timed computes the right thing: the rows of one instance are the plain stage's under MV * M
        ctx.sync()
        one = ctx.vertex_stage(-1, make_uniforms(_mat_product(mv, inst[7].reshape(4, 4))), proj, cube, faces)
        assert np.array_equal(out[0][84:96].cpu().numpy().view(np.uint64), one[0].view(np.uint64)), "instance 7: rows differ from the plain stage under MV * M"
        for k, v in ts.items():
            res["stage_" + k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
            print("stage", k, json.dumps(res["stage_" + k]), flush=True)
        if a.only == "stage":
            print("RESULT " + json.dumps(res), flush=True)
            return

        # ---- (b), (c) ----
        def flushes_of(fn):
            ctx.set_profiling(True); ctx.reset_phase_ms()
            fn()
            k = ctx.phase_ms()[1]
            ctx.set_profiling(False)
            return k

        def host_ms(fn, reps):
            v = []
            for rep in range(WARM + reps):
                ctx.zbuffer_restore(0); ctx.sync()
                t0 = time.perf_counter(); fn(); ctx.sync()
                if rep >= WARM:
                    v.append((time.perf_counter() - t0) * 1e3)
            return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))

        uniforms = None

        def loop(which):
            for i in which:
                ctx.draw_indexed(PHONG, uniforms[i], proj, d_cube, d_faces, device=True)
            ctx.flush()

        t0 = time.perf_counter()
        uniforms = [make_uniforms(_mat_product(mv, inst[i].reshape(4, 4))) for i in range(n)]      # (outside the timed part: the loop's ModelView * modelMatrix)
        res["uniforms_host_s"] = time.perf_counter() - t0

        def one_call():
            ctx.draw_instanced(PHONG, u, proj, d_cube, d_faces, instances=d_inst, device=True, instances_device=True)
            ctx.flush()

        res["call_instanced"] = host_ms(one_call, a.reps)
        res["call_instanced"]["flushes"] = flushes_of(one_call)
        print("call instanced", json.dumps(res["call_instanced"]), flush=True)
        res["call_loop"] = host_ms(lambda: loop(range(n)), a.loop_reps)
        res["call_loop"]["flushes"] = flushes_of(lambda: loop(range(n)))
        print("call loop", json.dumps(res["call_loop"]), flush=True)

        def gated_device():
            codes = ctx.occlusion_boxes(view_proj, d_boxes, device=True)
            ctx.draw_instanced(PHONG, u, proj, d_cube, d_faces, instances=d_inst, visible=codes, device=True, instances_device=True)
            ctx.flush()

        def gated_host():
            codes = ctx.occlusion_boxes(view_proj, d_boxes, device=True)
            ctx.sync()
            host = codes.cpu().numpy()
            loop(np.flatnonzero(host & 1))

        ctx.zbuffer_restore(0)
        codes = ctx.occlusion_boxes(view_proj, d_boxes, device=True)
        ctx.sync()
        res["codes"] = np.bincount(codes.cpu().numpy(), minlength=4).tolist()
        res["occl_device"] = host_ms(gated_device, a.reps)
        print("occlusion device", json.dumps(res["occl_device"]), flush=True)
        res["occl_host"] = host_ms(gated_host, a.loop_reps)
        print("occlusion host", json.dumps(res["occl_host"]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def _mat_product(a, b):
    """geometry.h:196-205: sums from 0.0, k ascending."""
    import numpy as np
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s = s + a[i, k] * b[k, j]
            out[i, j] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--instances", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--only", default="", help="stage: (a) alone, for a run under a profiler")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--size", str(a.size), "--instances", str(a.instances), "--reps", str(a.reps),
                        "--loop-reps", str(a.loop_reps), "--only", a.only], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("instanced_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    n, size = res["instances"], res["size"]
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["instanced draws, one MI355X, one run on %s: a 12-face cube under %d matrices, %d x %d frame" % (time.strftime("%Y-%m-%d"), n, size, size),
             "medians (min .. max) after a warm-up; (a) HIP events on the context's stream, (b) and (c) the host clock around call + flush + sync"]
    si, sy = res["stage_instanced"], res["stage_yardstick"]
    ratio = si["median_ms"] / sy["median_ms"]
    lines.append("(a) instanced stage     %s  k_inst_mv + k_instance_vertex_stage, %d output faces" % (fmt(si), 12 * n))
    lines.append("    k_vertex_stage      %s  one mesh of %d faces over the same 8 vertices" % (fmt(sy), 12 * n))
    lines.append("    ratio %.3f: %s" % (ratio, "within 1.10 x" if ratio <= 1.10 else "NOT within 1.10 x - the target is missed"))
    if "call_loop" in res:
        ci, cl = res["call_instanced"], res["call_loop"]
        lines.append("(b) one instanced call  %s  %d flush(es)" % (fmt(ci), ci["flushes"]))
        lines.append("    loop of draw_indexed %s  %d flushes; ratio %.1f" % (fmt(cl), cl["flushes"], cl["median_ms"] / ci["median_ms"]))
        od, oh = res["occl_device"], res["occl_host"]
        lines.append("(c) codes on the device %s  query + gated instanced draw; codes HIDDEN/VISIBLE/OUTSIDE/UNDECIDED = %s" % (fmt(od), res["codes"]))
        lines.append("    codes to the host   %s  query + copy + loop over the visible; ratio %.1f" % (fmt(oh), oh["median_ms"] / od["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
