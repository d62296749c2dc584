"""Times of the mesh-edge calls on one MI355X (DESIGN.md §6 "Mesh edges" records the results).

  python profiles/outline_probe.py [--reps 20] [--limit 900] [--out profiles/outline_probe_summary.txt]

Meshes: a torus of 1000 x 500 quads - 1 000 000 faces, 500 000 vertices at stride 8, closed - and a cube of 12 faces for the
launch-bound end.  Medians after a warm-up, with min and max.
  (a) trgl_mesh_edges without its count (no wait), against the radix sort of the same keys alone (trgl_debug_edge_sort: the floor);
      HIP events on the context's stream, the two alternating inside one loop
  (b) trgl_edge_select, plain and compacted (no count), against a device-to-device copy of the distinct bytes it reads plus those
      it writes - records 16, indices 12 per face, positions 24 per vertex; a code byte, a segment and a colour per record
  (c) the route (b) replaces: the host twin with compaction, then an upload of its segments and colours; the host clock
  (d) a frame - clear, draw, flush, sync - with trgl_draw_outline, against trgl_draw_lines over segments selected beforehand: the
      difference is the selection plus the 8-byte wait; the host clock
What was timed is compared with the host twins' bytes first.  Two untimed snapshot copies are queued in front of every event pair so
that the events bracket device work.  The measurement runs in one child process under a time limit of --limit seconds; the parent
never touches the GPU."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3
EYE = (0.5, 0.8, 6.0, 1.0)
COLORS = (0xFF000000, 0xFF000000, 0xFF000000, 0xFF808080)


def torus(m, n, stride=8):
    """m x n quads around a torus of radii 1 and 0.4: 2 m n faces, m n vertices, every edge on two faces"""
    import numpy as np
    j, i = np.mgrid[0:n, 0:m]
    a, b = 2 * np.pi * i / m, 2 * np.pi * j / n
    v = np.zeros((m * n, stride))
    v[:, 0], v[:, 1], v[:, 2] = ((1 + 0.4 * np.cos(b)) * np.cos(a)).ravel(), ((1 + 0.4 * np.cos(b)) * np.sin(a)).ravel(), (0.4 * np.sin(b)).ravel()
    p = lambda ii, jj: ((jj % n) * m + (ii % m)).ravel()
    f = np.stack([np.stack([p(i, j), p(i + 1, j), p(i + 1, j + 1)], 1), np.stack([p(i, j), p(i + 1, j + 1), p(i, j + 1)], 1)], 1)
    return v, f.reshape(-1, 3).astype(np.uint32)


def cube(stride=8):
    import numpy as np
    v = np.zeros((8, stride))
    v[:, :3] = [[2 * (k & 1) - 1, 2 * ((k >> 1) & 1) - 1, 2 * ((k >> 2) & 1) - 1] for k in range(8)]
    f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return v, np.array(f, np.uint32)


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api
    from tinyrenderder_amd.api import Context, FLAT
    if not torch.cuda.is_available():
        raise SystemExit("outline_probe: no GPU; there is nothing to measure without one")
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

        mv = np.array([1, 0, 0, -0.5, 0, 1, 0, -0.8, 0, 0, 1, -6, 0, 0, 0, 1], np.float64)      # the camera at EYE, looking down -z
        pr = np.array([2.5, 0, 0, 0, 0, 2.5, 0, 0, 0, 0, -1.125, -2.25 - 1.0 / 64, 0, 0, -1, 0], np.float64)
        LP = api.make_line_params(mv, pr, 2.0, (W / 2.0, H / 2.0), 1.0)
        for name, (v, f) in (("torus", torus(1000, 500)), ("cube", cube())):
            nv, F = v.shape[0], f.shape[0]
            d_v, d_f = torch.from_numpy(v).cuda(), torch.from_numpy(f.view(np.int32)).cuda()
            d_rec = torch.empty((3 * F, 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rr = dict(faces=F, vertices=nv)
            # (a)
            want_rec, E = api.mesh_edges(f, nv)
            _, got_E = ctx.mesh_edges(d_f, nv, device=True, out=d_rec)
            assert got_E == E and np.array_equal(d_rec.cpu().numpy().view(np.uint32), want_rec), name
            rr["edges"] = E
            rr["a"] = alternate(dict(edges=lambda: ctx.mesh_edges(d_f, nv, device=True, out=d_rec, count=False),
                                     sort=lambda: ctx._chk(ctx.L.trgl_debug_edge_sort(ctx.h, F, nv))))
            rr["a_host"] = host_ms(dict(twin=lambda: api.mesh_edges(f, nv)), 2)["twin"]
            # (b), (c)
            read, write = 16 * E + 12 * F + 24 * nv, 13 * E
            half = (read + write) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            out = (torch.empty(E, dtype=torch.uint8, device="cuda"), torch.empty((E, 2), dtype=torch.int32, device="cuda"),
                   torch.empty(E, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            P = {c: api.make_edge_params(EYE, 0.999, api.EDGE_SILHOUETTE | api.EDGE_CREASE, COLORS, c) for c in (False, True)}
            for c in (False, True):
                want = api.edge_select(P[c], v, f, want_rec, E)
                *_, n_sel = ctx.edge_select(P[c], d_v, d_f, d_rec, n_edges=E, device=True, out=out, count=c)
                ctx.sync()
                assert all(np.array_equal(o.cpu().numpy().view(w.dtype), w) for o, w in zip(out, want[:3])) and (not c or n_sel == want[3]), name
                rr["selected"] = want[3]

            def copy():
                with torch.cuda.stream(stream):
                    dst.copy_(src)

            rr["read_bytes"], rr["write_bytes"] = read, write
            rr["b"] = alternate(dict(plain=lambda: ctx.edge_select(P[False], d_v, d_f, d_rec, n_edges=E, device=True, out=out, count=False),
                                     compact=lambda: ctx.edge_select(P[True], d_v, d_f, d_rec, n_edges=E, device=True, out=out, count=False),
                                     copy=copy))

            def route():
                _, seg, col, n = api.edge_select(P[True], v, f, want_rec, E)
                return torch.from_numpy(seg[:n].view(np.int32)).cuda(), torch.from_numpy(col[:n].view(np.int32)).cuda()

            rr["c"] = host_ms(dict(route=route), 3)["route"]
            # (d)
            *_, n_sel = ctx.edge_select(P[True], d_v, d_f, d_rec, n_edges=E, device=True, out=out)
            d_seg, d_col = out[1].clone(), out[2].clone()
            torch.cuda.synchronize()

            def frame(outline):
                ctx.clear((255, 255, 255, 255), np.inf)
                if outline:
                    ctx.draw_outline(FLAT, LP, P[True], d_v, d_f, d_rec, n_edges=E, device=True)
                else:
                    ctx.draw_lines(FLAT, LP, d_v, d_seg, d_col, n_segments=n_sel, device=True)
                ctx.flush()

            fb = []
            for outline in (True, False):
                frame(outline)
                fb.append(ctx.read_framebuffer())
            assert np.array_equal(fb[0], fb[1]) and (fb[0] != 255).any(), name
            rr["d"] = host_ms(dict(outline=lambda: frame(True), lines=lambda: frame(False)), a.reps)
            res[name] = rr
            print(name, json.dumps(rr), flush=True)
            del d_v, d_f, d_rec, src, dst, out, d_seg, d_col
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
        raise SystemExit("outline_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["mesh edges, one MI355X, one run on %s" % time.strftime("%Y-%m-%d"),
             "medians (min .. max) after a warm-up; (a), (b) HIP events on the context's stream, (c), (d) the host clock around calls + sync"]
    for name, rr in res.items():
        a_, b_, d_ = rr["a"], rr["b"], rr["d"]
        tot = rr["read_bytes"] + rr["write_bytes"]
        lines.append("%s: %d faces, %d vertices at stride 8, %d edges, %d selected (silhouettes and creases)" % (name, rr["faces"], rr["vertices"],
                                                                                                             rr["edges"], rr["selected"]))
        lines.append("(a) trgl_mesh_edges, no count      %s" % fmt(a_["edges"]))
        lines.append("    the sort of its keys alone     %s  ratio %.3f" % (fmt(a_["sort"]), a_["edges"]["median_ms"] / a_["sort"]["median_ms"]))
        lines.append("    its host twin                  %s" % fmt(rr["a_host"]))
        lines.append("(b) trgl_edge_select, plain        %s  reads %d and writes %d distinct bytes" % (fmt(b_["plain"]), rr["read_bytes"], rr["write_bytes"]))
        lines.append("    compacted, no count            %s" % fmt(b_["compact"]))
        lines.append("    copy of as many bytes          %s  ratios %.3f plain, %.3f compacted; %.2f TB/s" %
                     (fmt(b_["copy"]), b_["plain"]["median_ms"] / b_["copy"]["median_ms"], b_["compact"]["median_ms"] / b_["copy"]["median_ms"],
                      tot / (b_["copy"]["median_ms"] * 1e-3) / 1e12))
        lines.append("(c) host twin + upload of segments %s  %.0f x (b) compacted" % (fmt(rr["c"]), rr["c"]["median_ms"] / b_["compact"]["median_ms"]))
        lines.append("(d) frame with trgl_draw_outline   %s" % fmt(d_["outline"]))
        lines.append("    frame with trgl_draw_lines     %s  difference %.3f ms" % (fmt(d_["lines"]), d_["outline"]["median_ms"] - d_["lines"]["median_ms"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
