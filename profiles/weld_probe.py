"""Times of trgl_mesh_weld on one MI355X (DESIGN.md §6 "Mesh welding" records the results).

  python profiles/weld_probe.py [--reps 10] [--limit 900] [--out profiles/weld_probe_summary.txt]

Arrays: about 1 M vertices at stride 14 (position key, doubles 0 .. 2) and at stride 3 (the whole record), once without duplicates
(random positions) and once as the soup of a closed mesh - a torus of 408 x 408 quads, three records per face, six corners per vertex:
83 % duplicates, indices 0 .. n - 1 -; and the cube of an OBJ reader, 24 vertices, for the launch-bound end.  Medians after a warm-up,
with min and max.
  (a) trgl_mesh_weld with all four outputs, no count (no wait); HIP events on the context's stream
  (b) the radix sort of its (hash, vertex) pairs alone (trgl_debug_weld_sort: the floor), alternating with (a) inside one loop
  (c) a device-to-device copy of the distinct bytes the call reads plus those it writes: the records and the indices in, the map, the
      first occurrences, the records and the indices out - alternating with (a) and (b)
  (d) the route it replaces: the host twin, then an upload of its four outputs; the host clock
  (e) torch.unique(dim=0, return_inverse=True) over the same key columns, an outside comparison (it numbers in sorted order, so only
      its time is taken); the host clock around the call and a synchronize
What was timed is compared with the host twin's bytes first.  Every repetition reads and writes the same arrays, so whatever fits the
last-level cache is replayed from it: the copy (c) is measured under the same condition, and neither is a figure for cold HBM.  Two
untimed snapshot copies are queued in front of every event pair so that the events bracket device work.  The measurement runs in one
child process under a time limit of --limit seconds; the parent never touches the GPU and writes the summary as the child reported it."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 3


def torus_soup(m, n, stride, seed=5):
    """the faces of a torus of m x n quads as a soup: [6 m n, stride] records - position first, noise behind -, indices 0 .. 6 m n - 1"""
    import numpy as np
    j, i = np.mgrid[0:n, 0:m]
    a, b = 2 * np.pi * i / m, 2 * np.pi * j / n
    pos = np.stack([((1 + 0.4 * np.cos(b)) * np.cos(a)).ravel(), ((1 + 0.4 * np.cos(b)) * np.sin(a)).ravel(), (0.4 * np.sin(b)).ravel()], 1)
    p = lambda ii, jj: ((jj % n) * m + (ii % m)).ravel()
    f = np.stack([np.stack([p(i, j), p(i + 1, j), p(i + 1, j + 1)], 1), np.stack([p(i, j), p(i + 1, j + 1), p(i, j + 1)], 1)], 1).reshape(-1)
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, (f.size, stride))
    v[:, :3] = pos[f]
    return np.ascontiguousarray(v), np.arange(f.size, dtype=np.uint32).reshape(-1, 3)


def distinct(n, stride, seed=6):
    import numpy as np
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, stride))
    return np.ascontiguousarray(v), np.arange(n - n % 3, dtype=np.uint32).reshape(-1, 3)


def split_cube(stride):
    import numpy as np
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    v = np.random.default_rng(7).uniform(-1.0, 1.0, (24, stride))
    v[:, :3] = [[2 * (c & 1) - 1, 2 * ((c >> 1) & 1) - 1, 2 * ((c >> 2) & 1) - 1] for q in quads for c in q]
    f = [[4 * q + k for k in t] for q in range(6) for t in ((0, 1, 2), (0, 2, 3))]
    return np.ascontiguousarray(v), np.array(f, np.uint32)


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api
    from tinyrenderder_amd.api import Context
    if not torch.cuda.is_available():
        raise SystemExit("weld_probe: no GPU; there is nothing to measure without one")
    res = {}
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    with Context(512, 512, 3) as ctx:
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
                    ctx.sync(); torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); ctx.sync(); torch.cuda.synchronize()
                    if rep >= 1:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return {k: stat(v) for k, v in ts.items()}

        cases = []
        for stride in (14, 3):
            cases.append(("%d distinct" % stride, stride) + distinct(998784, stride))
            cases.append(("%d soup" % stride, stride) + torus_soup(408, 408, stride))
        cases.append(("cube", 8) + split_cube(8))
        for name, stride, v, f in cases:
            n, F = v.shape[0], f.shape[0]
            P = api.make_weld_params(stride, 0, 3)
            want, U = api.mesh_weld(P, v, f)
            d_v, d_f = torch.from_numpy(v).cuda(), torch.from_numpy(f.view(np.int32)).cuda()
            out = dict(remap=torch.empty(n, dtype=torch.int32, device="cuda"), firsts=torch.empty(n, dtype=torch.int32, device="cuda"),
                       vertices=torch.empty((n, stride), dtype=torch.float64, device="cuda"), indices=torch.empty((F, 3), dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            _, got_U = ctx.mesh_weld(P, d_v, d_f, device=True, out=out)
            assert got_U == U and all(np.array_equal(out[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)) for k in want), name
            read, write = 8 * stride * n + 12 * F, 8 * n + 8 * stride * n + 12 * F
            half = (read + write) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def copy():
                with torch.cuda.stream(stream):
                    dst.copy_(src)

            rr = dict(vertices=n, stride=stride, faces=F, unique=U, read_bytes=read, write_bytes=write)
            rr["abc"] = alternate(dict(weld=lambda: ctx.mesh_weld(P, d_v, d_f, device=True, out=out, count=False),
                                       sort=lambda: ctx.debug_weld_sort(n), copy=copy))

            def route():
                o, _ = api.mesh_weld(P, v, f)
                return [torch.from_numpy(np.ascontiguousarray(o[k]).view(np.float64 if k == "vertices" else np.int32)).cuda() for k in o]

            rr["d"] = host_ms(dict(route=route), 2)["route"]
            key = d_v[:, :3].contiguous()
            torch.cuda.synchronize()
            rr["e"] = host_ms(dict(unique=lambda: torch.unique(key, dim=0, return_inverse=True)), 3)["unique"]
            res[name] = rr
            print(name, json.dumps(rr), flush=True)
            del d_v, d_f, out, src, dst, key
            ctx._keep.clear()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("weld_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["mesh welding, one MI355X, one run on %s" % time.strftime("%Y-%m-%d"),
             "medians (min .. max) after a warm-up; (a), (b), (c) HIP events on the context's stream, back-to-back calls over the same arrays -",
             "what fits the last-level cache replays from it, for the copy as for the call; (d), (e) the host clock around calls + sync"]
    for name, rr in res.items():
        t = rr["abc"]
        tot = rr["read_bytes"] + rr["write_bytes"]
        w = t["weld"]["median_ms"]
        lines.append("%s: %d vertices at stride %d, position key, %d faces, %d distinct (%.0f %% duplicates)" %
                     (name, rr["vertices"], rr["stride"], rr["faces"], rr["unique"], 100.0 * (1 - rr["unique"] / rr["vertices"])))
        lines.append("(a) trgl_mesh_weld, all outputs    %s" % fmt(t["weld"]))
        lines.append("(b) the sort of its pairs alone    %s  (a)/(b) %.3f" % (fmt(t["sort"]), w / t["sort"]["median_ms"]))
        lines.append("(c) copy of %10d bytes     %s  (a)/(c) %.3f; the copy runs at %.2f TB/s" %
                     (tot, fmt(t["copy"]), w / t["copy"]["median_ms"], tot / (t["copy"]["median_ms"] * 1e-3) / 1e12))
        lines.append("(d) host twin + upload of outputs  %s  %.0f x (a)" % (fmt(rr["d"]), rr["d"]["median_ms"] / w))
        lines.append("(e) torch.unique(dim=0, inverse)   %s  %.1f x (a)" % (fmt(rr["e"]), rr["e"]["median_ms"] / w))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
