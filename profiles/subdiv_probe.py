"""Times of the mesh-subdivision calls on one MI355X (DESIGN.md §6 "Mesh subdivision" records the results).

  python profiles/subdiv_probe.py [--reps 20] [--limit 900] [--out profiles/subdiv_probe_summary.txt]

Meshes: the torus of profiles/outline_probe.py - 1000 x 500 quads, 1 000 000 faces, 500 000 vertices, 1 500 000 edges, closed, every
vertex of valence 6 - at stride 3 (smooth 3) and stride 14 (smooth 3), and a cube of 12 faces for the launch-bound end.  Medians
after a warm-up, with min and max.
  (1) trgl_subdiv_vertices, LOOP and LINEAR, against a device-to-device copy of the distinct bytes the LOOP call reads plus those it
      writes - the stencil array, the vertex array once, the output; HIP events on the context's stream, the three alternating
  (2) trgl_subdiv_topology against the radix sort of its entries alone (trgl_debug_subdiv_sort: the floor); events
  (3) the route (1) replaces: the host twin, then an upload of the refined vertices; the host clock
  (4) a frame - clear, draw, flush, sync - with trgl_draw_subdivided, against trgl_draw_indexed of a mesh refined beforehand: the
      difference is the vertex kernel; the host clock (stride 14 only: the built-in vertex stage reads 8 doubles)
What is timed is compared with the host twins' bytes first.  Two untimed snapshot copies are queued in front of every event pair so
that the events bracket device work.  The measurement runs in one child process under a time limit of --limit seconds; the parent
never touches the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "profiles")

WARM = 3


def child(a):
    import numpy as np
    import torch
    from outline_probe import cube, torus
    from tinyrenderder_amd import api
    from tinyrenderder_amd.api import Context, PHONG
    if not torch.cuda.is_available():
        raise SystemExit("subdiv_probe: no GPU; there is nothing to measure without one")
    res = {}
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    W = H = 512
    with Context(W, H, 3) as ctx:
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

        def host_ms(sides, reps):
            ts = {k: [] for k in sides}
            for rep in range(1 + reps):
                for k, fn in sides.items():
                    ctx.sync()
                    t0 = time.perf_counter(); fn(); ctx.sync(); torch.cuda.synchronize()
                    if rep >= 1:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return {k: stat(v) for k, v in ts.items()}

        mv = np.array([1, 0, 0, -0.5, 0, 1, 0, -0.8, 0, 0, 1, -6, 0, 0, 0, 1], np.float64)
        pr = np.array([2.5, 0, 0, 0, 0, 2.5, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64)
        u = api.make_uniforms(mv.reshape(4, 4), (0, 0, 1), (0, 0, 1), (0, 0, 1))
        rng = np.random.default_rng(7)
        for name, (v8, f) in (("torus", torus(1000, 500)), ("cube", cube())):
            nv, F = v8.shape[0], f.shape[0]
            rec, E = api.mesh_edges(f, nv)
            want_ref, want_st = api.subdiv_topology(f, nv, rec[:E], E)
            d_f, d_rec = torch.from_numpy(f.view(np.int32)).cuda(), torch.from_numpy(rec[:E].view(np.int32)).cuda()
            out_t = (torch.empty((4 * F, 3), dtype=torch.int32, device="cuda"), torch.empty(want_st.size, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            rr = dict(faces=F, vertices=nv, edges=E)
            # (2)
            d_ref, d_st = ctx.subdiv_topology(d_f, nv, d_rec, E, device=True, out=out_t)
            ctx.sync()
            assert np.array_equal(d_ref.cpu().numpy().view(np.uint32), want_ref) and np.array_equal(d_st.cpu().numpy().view(np.uint32), want_st), name
            rr["topology"] = alternate(dict(topology=lambda: ctx.subdiv_topology(d_f, nv, d_rec, E, device=True, out=out_t),
                                            sort=lambda: ctx._chk(ctx.L.trgl_debug_subdiv_sort(ctx.h, E, nv))))
            t0 = time.perf_counter(); api.subdiv_topology(f, nv, rec[:E], E); rr["topology_host_ms"] = (time.perf_counter() - t0) * 1e3
            # (1), (3), (4)
            for stride in (3, 14):
                v = np.ascontiguousarray(np.concatenate([v8, rng.uniform(-1, 1, (nv, 6))], 1)[:, :stride])
                v[:, 3:6] = v[:, :3] if stride >= 6 else v[:, 3:6]           # (something normal-like for the frame)
                d_v = torch.from_numpy(v).cuda()
                d_out = torch.empty((nv + E, stride), dtype=torch.float64, device="cuda")
                P = {m: api.make_subdiv_params(stride, mode, 3) for m, mode in (("loop", api.SUBDIV_LOOP), ("linear", api.SUBDIV_LINEAR))}
                torch.cuda.synchronize()
                for m in P:
                    want = api.subdiv_vertices(P[m], v, want_st, E)
                    ctx.subdiv_vertices(P[m], d_v, d_st, E, device=True, out=d_out)
                    ctx.sync()
                    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want.view(np.uint64)), (name, stride, m)
                read, write = 4 * want_st.size + 8 * nv * stride, 8 * (nv + E) * stride
                half = (read + write) // 2
                src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()

                def copy():
                    with torch.cuda.stream(stream):
                        dst.copy_(src)

                s = dict(read_bytes=read, write_bytes=write)
                s["vertices"] = alternate(dict(loop=lambda: ctx.subdiv_vertices(P["loop"], d_v, d_st, E, device=True, out=d_out),
                                               linear=lambda: ctx.subdiv_vertices(P["linear"], d_v, d_st, E, device=True, out=d_out), copy=copy))
                s["route"] = host_ms(dict(route=lambda: torch.from_numpy(api.subdiv_vertices(P["loop"], v, want_st, E)).cuda()), 3)["route"]
                if stride == 14:
                    ctx.subdiv_vertices(P["loop"], d_v, d_st, E, device=True, out=d_out)
                    ctx.sync()

                    def frame(one):
                        ctx.clear((255, 255, 255, 255), np.inf)
                        if one:
                            ctx.draw_subdivided(PHONG, u, pr, P["loop"], d_v, d_st, d_ref, E, device=True)
                        else:
                            ctx.draw_indexed(PHONG, u, pr, d_out, d_ref, device=True)
                        ctx.flush()

                    fb = []
                    for one in (True, False):
                        frame(one)
                        fb.append(ctx.read_framebuffer())
                    assert np.array_equal(fb[0], fb[1]) and (fb[0] != 255).any(), name
                    s["frame"] = host_ms(dict(subdivided=lambda: frame(True), indexed=lambda: frame(False)), a.reps)
                rr["stride%d" % stride] = s
                del d_v, d_out, src, dst
            res[name] = rr
            print(name, json.dumps(rr), flush=True)
            del d_f, d_rec, out_t, d_ref, d_st
            ctx._keep.clear()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("subdiv_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["mesh subdivision, one MI355X, one run on %s" % time.strftime("%Y-%m-%d"),
             "medians (min .. max) after a warm-up; (1), (2) HIP events on the context's stream, (3), (4) the host clock around calls + sync"]
    for name, rr in res.items():
        t = rr["topology"]
        lines.append("%s: %d faces, %d vertices, %d edges; refined: %d faces, %d vertices" % (name, rr["faces"], rr["vertices"], rr["edges"], 4 * rr["faces"],
                                                                                           rr["vertices"] + rr["edges"]))
        lines.append("(2) trgl_subdiv_topology           %s" % fmt(t["topology"]))
        lines.append("    the sort of its entries alone  %s  ratio %.3f" % (fmt(t["sort"]), t["topology"]["median_ms"] / t["sort"]["median_ms"]))
        lines.append("    its host twin                  %9.3f ms (once)" % rr["topology_host_ms"])
        for stride in (3, 14):
            s = rr["stride%d" % stride]
            v = s["vertices"]
            tot = s["read_bytes"] + s["write_bytes"]
            lines.append("  stride %d, smooth 3: reads %d and writes %d distinct bytes" % (stride, s["read_bytes"], s["write_bytes"]))
            lines.append("(1) trgl_subdiv_vertices, LOOP     %s" % fmt(v["loop"]))
            lines.append("    LINEAR                         %s" % fmt(v["linear"]))
            lines.append("    copy of as many bytes          %s  ratios %.3f LOOP, %.3f LINEAR; %.2f TB/s" %
                         (fmt(v["copy"]), v["loop"]["median_ms"] / v["copy"]["median_ms"], v["linear"]["median_ms"] / v["copy"]["median_ms"],
                          tot / (v["copy"]["median_ms"] * 1e-3) / 1e12))
            lines.append("(3) host twin + upload of vertices %s  %.0f x (1) LOOP" % (fmt(s["route"]), s["route"]["median_ms"] / v["loop"]["median_ms"]))
            if "frame" in s:
                d = s["frame"]
                lines.append("(4) frame with trgl_draw_subdivided %s" % fmt(d["subdivided"]))
                lines.append("    frame with trgl_draw_indexed    %s  difference %.3f ms" % (fmt(d["indexed"]), d["subdivided"]["median_ms"] - d["indexed"]["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
