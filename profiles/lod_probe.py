"""Times of trgl_mesh_clean and trgl_mesh_simplify on one MI355X (DESIGN.md §6 "Mesh levels of detail" records the results).

  python profiles/lod_probe.py [--reps 8] [--limit 900] [--out profiles/lod_probe_summary.txt] [--small]

Mesh: a closed torus of 1416 x 354 quads - 1 002 528 faces over 501 264 shared vertices, already welded - at stride 14 and stride 3
(position first, noise behind), and the cube of 8 vertices and 12 faces for the launch-bound end.  Medians after a warm-up, with min and max.
  clean, over the torus as it is and over what a grid weld left of it (the cell that keeps about a quarter of its faces; the rest are
  degenerate or repeat an earlier face):
  (a) trgl_mesh_clean with both flags and all outputs, no counts (no wait); HIP events on the context's stream
  (b) the radix sort of its (hash, face) pairs alone (trgl_debug_lod_sort: the floor), alternating with (a) inside one loop
  (c) a device-to-device copy of the distinct bytes the call reads plus those it writes, alternating with (a) and (b)
  simplify, with the cells that keep about 1/4 and about 1/16 of the faces, mean_count 0 and 3:
  (d) trgl_mesh_simplify with all outputs, no counts
  (e) the same work as separate calls: trgl_mesh_weld with all outputs, then trgl_mesh_clean with both flags over them, alternating with (d)
  (f) the route it replaces: the host twin, then an upload of its five outputs; the host clock
  (g) the worst case of the mean: the torus moved so that one cell border cuts it along every axis - the whole mesh in 8 cells, one thread
      walking each; mean_count 3 against mean_count 0
  (h) a frame of trgl_draw_indexed (PHONG, 512 x 512) of the stride-14 torus and of its two levels, the host clock around clear, draw,
      flush and sync
What was timed is compared with the host twin's bytes first.  Every repetition reads and writes the same arrays, so whatever fits the
last-level cache is replayed from it: the copy (c) is measured under the same condition, and neither is a figure for cold HBM.  Two
untimed snapshot copies are queued in front of every event pair so that the events bracket device work.  The measurement runs in one
child process under a time limit of --limit seconds; the parent never touches the GPU and writes the summary as the child reported it.
--small: a torus of 96 x 24 quads, to rehearse the script."""
import argparse
import json
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

WARM = 2


def torus(m, n, stride, shift=0.0, seed=5):
    """a closed torus of m x n quads with shared vertices: ([m n, stride] records - position first, noise behind -, [2 m n, 3] indices)"""
    import numpy as np
    j, i = np.mgrid[0:n, 0:m]
    a, b = 2 * np.pi * i / m, 2 * np.pi * j / n
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, (m * n, stride))
    v[:, 0], v[:, 1], v[:, 2] = ((1 + 0.4 * np.cos(b)) * np.cos(a)).ravel(), ((1 + 0.4 * np.cos(b)) * np.sin(a)).ravel(), (0.4 * np.sin(b)).ravel()
    v[:, :3] += shift
    p = lambda ii, jj: ((jj % n) * m + (ii % m)).ravel()
    f = np.stack([np.stack([p(i, j), p(i + 1, j), p(i + 1, j + 1)], 1), np.stack([p(i, j), p(i + 1, j + 1), p(i, j + 1)], 1)], 1).reshape(-1, 3)
    return np.ascontiguousarray(v), np.ascontiguousarray(f.astype(np.uint32))


def cube(stride):
    import numpy as np
    v = np.random.default_rng(7).uniform(-1.0, 1.0, (8, stride))
    v[:, :3] = [[2 * (c & 1) - 1, 2 * ((c >> 1) & 1) - 1, 2 * ((c >> 2) & 1) - 1] for c in range(8)]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return np.ascontiguousarray(v), np.array([[q[k] for k in t] for q in quads for t in ((0, 1, 2), (0, 2, 3))], np.uint32)


def cell_for(api, v3, f, share):
    """the cell, by bisection on the host twin, after which about `share` of the faces are kept"""
    lo, hi = 1e-4, 1.0
    for _ in range(14):
        mid = (lo * hi) ** 0.5
        kept = api.mesh_simplify(api.make_simplify_params(3, mid, 0), v3, f)[1][0]
        lo, hi = (mid, hi) if kept > share * f.shape[0] else (lo, mid)
    return hi


def child(a):
    import numpy as np
    import torch
    from tinyrenderder_amd import api
    from tinyrenderder_amd.api import Context, PHONG, make_uniforms
    if not torch.cuda.is_available():
        raise SystemExit("lod_probe: no GPU; there is nothing to measure without one")
    res = {}
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda()
    same = lambda got, want: all(np.array_equal(got[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)) for k in want)
    m, n = (96, 24) if a.small else (1416, 354)
    BOTH = api.CLEAN_DUPLICATES | api.CLEAN_VERTICES
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

        def host_ms(fn, reps):
            ts = []
            for rep in range(1 + reps):
                ctx.sync(); torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); ctx.sync(); torch.cuda.synchronize()
                if rep >= 1:
                    ts.append((time.perf_counter() - t0) * 1e3)
                ctx._keep.clear()
            return stat(ts)

        v3, f = torus(m, n, 3)
        cells = {"1/4": cell_for(api, v3, f, 0.25), "1/16": cell_for(api, v3, f, 1.0 / 16)}
        print("cells", cells, flush=True)
        levels = {}
        for stride in (14, 3):
            v, f = torus(m, n, stride)
            V, F = v.shape[0], f.shape[0]
            d_v, d_f = up(v), up(f)
            # ---- clean: the mesh as it is, and after a grid weld
            w, _ = api.mesh_weld(api.make_weld_params(stride, 0, 3, cells["1/4"]), v, f)
            for name, cv, cf in (("clean mesh", v, f), ("after a grid weld", w["vertices"], w["indices"])):
                P = api.make_clean_params(stride, BOTH)
                want, counts = api.mesh_clean(P, cf, cv)
                d_cv, d_cf = up(cv), up(cf)
                out = dict(indices=torch.empty((F, 3), dtype=torch.int32, device="cuda"), face_firsts=torch.empty(F, dtype=torch.int32, device="cuda"),
                           vremap=torch.empty(V, dtype=torch.int32, device="cuda"), vfirsts=torch.empty(V, dtype=torch.int32, device="cuda"),
                           vertices=torch.empty((V, stride), dtype=torch.float64, device="cuda"))
                torch.cuda.synchronize()
                _, got = ctx.mesh_clean(P, d_cf, d_cv, device=True, out=out)
                assert got == counts and same(out, want), name
                # read: the triples and the kept records; written: triples, face firsts, the two vertex maps, all records (kept or zero)
                read, write = 12 * F + 8 * stride * counts[1], 12 * F + 4 * F + 8 * V + 8 * stride * V
                half = (read + write) // 2
                src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()

                def copy():
                    with torch.cuda.stream(stream):
                        dst.copy_(src)

                rr = dict(kind="clean", vertices=V, stride=stride, faces=F, kept_faces=counts[0], kept_vertices=counts[1], bytes=read + write)
                rr["abc"] = alternate(dict(call=lambda: ctx.mesh_clean(P, d_cf, d_cv, device=True, out=out, count=False),
                                           sort=lambda: ctx.debug_lod_sort(F, V), copy=copy))
                res["%d %s" % (stride, name)] = rr
                print(stride, name, json.dumps(rr), flush=True)
                del d_cv, d_cf, out, src, dst
            # ---- simplify
            for share, cell in cells.items():
                for mean_count in (0, 3):
                    P = api.make_simplify_params(stride, cell, mean_count)
                    want, counts = api.mesh_simplify(P, v, f)
                    out = dict(remap=torch.empty(V, dtype=torch.int32, device="cuda"), firsts=torch.empty(V, dtype=torch.int32, device="cuda"),
                               vertices=torch.empty((V, stride), dtype=torch.float64, device="cuda"), indices=torch.empty((F, 3), dtype=torch.int32, device="cuda"),
                               face_firsts=torch.empty(F, dtype=torch.int32, device="cuda"))
                    torch.cuda.synchronize()
                    _, got = ctx.mesh_simplify(P, d_v, d_f, device=True, out=out)
                    assert got == counts and same(out, want), (stride, share, mean_count)
                    rr = dict(kind="simplify", vertices=V, stride=stride, faces=F, cell=cell, mean_count=mean_count, kept_faces=counts[0], kept_vertices=counts[1])
                    sides = dict(call=lambda: ctx.mesh_simplify(P, d_v, d_f, device=True, out=out, count=False))
                    if mean_count == 0:
                        W, C = api.make_weld_params(stride, 0, 3, cell), api.make_clean_params(stride, BOTH)
                        wo = dict(remap=torch.empty(V, dtype=torch.int32, device="cuda"), firsts=torch.empty(V, dtype=torch.int32, device="cuda"),
                                  vertices=torch.empty((V, stride), dtype=torch.float64, device="cuda"), indices=torch.empty((F, 3), dtype=torch.int32, device="cuda"))
                        co = dict(indices=out["indices"], face_firsts=out["face_firsts"], vremap=torch.empty(V, dtype=torch.int32, device="cuda"),
                                  vfirsts=torch.empty(V, dtype=torch.int32, device="cuda"), vertices=out["vertices"])

                        def separate():
                            ctx.mesh_weld(W, d_v, d_f, device=True, out=wo, count=False)
                            ctx.mesh_clean(C, wo["indices"], wo["vertices"], device=True, out=co, count=False)

                        sides["separate"] = separate
                    rr["de"] = alternate(sides)
                    rr["f"] = host_ms(lambda: [up(x) for x in api.mesh_simplify(P, v, f)[0].values()], 2)
                    res["%d simplify %s mean %d" % (stride, share, mean_count)] = rr
                    print(stride, share, mean_count, json.dumps(rr), flush=True)
                    if stride == 14 and mean_count == 3:
                        levels[share] = (out["vertices"][:counts[1]].clone(), out["indices"][:counts[0]].clone(), counts)
                    del out
            # ---- the worst case of the mean: 8 cells
            sv, sf = torus(m, n, stride, shift=1.5)
            d_sv, d_sf = up(sv), up(sf)
            out = dict(vertices=torch.empty((V, stride), dtype=torch.float64, device="cuda"), indices=torch.empty((F, 3), dtype=torch.int32, device="cuda"))
            sides = {}
            for mean_count in (0, 3):
                P = api.make_simplify_params(stride, 3.0, mean_count)
                want, counts = api.mesh_simplify(P, sv, sf)
                torch.cuda.synchronize()
                _, got = ctx.mesh_simplify(P, d_sv, d_sf, device=True, out=out)
                assert got == counts and same(out, {k: want[k] for k in out}), ("8 cells", stride, mean_count)
                sides["mean %d" % mean_count] = (lambda Q: lambda: ctx.mesh_simplify(Q, d_sv, d_sf, device=True, out=out, count=False))(P)
            rr = dict(kind="worst", vertices=V, stride=stride, faces=F, kept_faces=counts[0], kept_vertices=counts[1])
            rr["g"] = alternate(sides)
            res["%d worst" % stride] = rr
            print(stride, "worst", json.dumps(rr), flush=True)
            # ---- drawing
            if stride == 14:
                u = make_uniforms(np.array([[1, 0, 0, 0], [0, 0.8, -0.6, 0], [0, 0.6, 0.8, -4], [0, 0, 0, 1]], np.float64), (0, 0, 1), (0, 0, 1), (0, 0, 1))
                proj = np.array([1.25, 0, 0, 0, 0, 1.25, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64).reshape(4, 4)
                rr = dict(kind="draw")
                for name, (lv, lf, counts) in [("full", (d_v, d_f, (F, V)))] + list(levels.items()):

                    def frame():
                        ctx.clear((0, 0, 0, 255), np.inf)
                        ctx.draw_indexed(PHONG, u, proj, lv, lf, device=True)
                        ctx.flush()

                    rr[name] = dict(host_ms(frame, 3), faces=counts[0], vertices=counts[1])
                res["draw"] = rr
                print("draw", json.dumps(rr), flush=True)
            del d_v, d_f, d_sv, d_sf, out
            ctx._keep.clear()
        # ---- the cube
        v, f = cube(8)
        d_v, d_f = up(v), up(f)
        P, Q = api.make_clean_params(8, BOTH), api.make_simplify_params(8, 0.0, 3)
        torch.cuda.synchronize()
        co, cc = ctx.mesh_clean(P, d_f, d_v, device=True)
        so, sc = ctx.mesh_simplify(Q, d_v, d_f, device=True)
        assert cc == (12, 8) and sc == (12, 8)
        rr = dict(kind="cube")
        rr["t"] = alternate(dict(clean=lambda: ctx.mesh_clean(P, d_f, d_v, device=True, out=co, count=False),
                                 simplify=lambda: ctx.mesh_simplify(Q, d_v, d_f, device=True, out=so, count=False)))
        res["cube"] = rr
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, __file__, "--child", "--reps", str(a.reps)] + (["--small"] if a.small else []), capture_output=True, text=True,
                       timeout=a.limit)
    sys.stdout.write(r.stdout); sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit("lod_probe: the measurement failed (%d)" % r.returncode)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    fmt = lambda v: "%9.3f ms (%.3f .. %.3f, %d reps)" % (v["median_ms"], v["min_ms"], v["max_ms"], v["reps"])
    lines = ["mesh levels of detail, one MI355X, one run on %s" % time.strftime("%Y-%m-%d"),
             "medians (min .. max) after a warm-up; (a)-(e), (g) HIP events on the context's stream, back-to-back calls over the same arrays -",
             "what fits the last-level cache replays from it, for the copy as for the call; (f), (h) the host clock around calls + sync"]
    for name, rr in res.items():
        if rr["kind"] == "clean":
            t = rr["abc"]
            c = t["call"]["median_ms"]
            lines.append("%s: %d faces over %d vertices at stride %d; %d faces (%.0f %%) and %d vertices kept" %
                         (name, rr["faces"], rr["vertices"], rr["stride"], rr["kept_faces"], 100.0 * rr["kept_faces"] / rr["faces"], rr["kept_vertices"]))
            lines.append("(a) trgl_mesh_clean, both flags, all outputs %s" % fmt(t["call"]))
            lines.append("(b) the sort of its pairs alone              %s  (a)/(b) %.3f" % (fmt(t["sort"]), c / t["sort"]["median_ms"]))
            lines.append("(c) copy of %10d bytes               %s  (a)/(c) %.3f; the copy runs at %.2f TB/s" %
                         (rr["bytes"], fmt(t["copy"]), c / t["copy"]["median_ms"], rr["bytes"] / (t["copy"]["median_ms"] * 1e-3) / 1e12))
        elif rr["kind"] == "simplify":
            t = rr["de"]
            c = t["call"]["median_ms"]
            lines.append("%s: stride %d, cell %.6g, mean_count %d; %d of %d faces (1/%.1f) and %d of %d vertices kept" %
                         (name, rr["stride"], rr["cell"], rr["mean_count"], rr["kept_faces"], rr["faces"], rr["faces"] / max(rr["kept_faces"], 1), rr["kept_vertices"],
                          rr["vertices"]))
            lines.append("(d) trgl_mesh_simplify, all outputs          %s" % fmt(t["call"]))
            if "separate" in t:
                lines.append("(e) trgl_mesh_weld + trgl_mesh_clean         %s  (d)/(e) %.3f" % (fmt(t["separate"]), c / t["separate"]["median_ms"]))
            if "f" in rr:
                lines.append("(f) host twin + upload of outputs            %s  %.0f x (d)" % (fmt(rr["f"]), rr["f"]["median_ms"] / c))
        elif rr["kind"] == "worst":
            t = rr["g"]
            lines.append("%s: stride %d, the whole mesh in 8 cells; %d faces and %d vertices kept" % (name, rr["stride"], rr["kept_faces"], rr["kept_vertices"]))
            lines.append("(g) trgl_mesh_simplify, mean_count 0         %s" % fmt(t["mean 0"]))
            lines.append("(g) trgl_mesh_simplify, mean_count 3         %s  %.1f x mean_count 0: the serial walk of 8 threads" %
                         (fmt(t["mean 3"]), t["mean 3"]["median_ms"] / t["mean 0"]["median_ms"]))
        elif rr["kind"] == "draw":
            for level, t in rr.items():
                if level != "kind":
                    lines.append("(h) a 512 x 512 PHONG frame, level %-5s %8d faces %s" % (level, t["faces"], fmt(t)))
        else:
            lines.append("cube, 12 faces over 8 vertices: trgl_mesh_clean %s; trgl_mesh_simplify %s" % (fmt(rr["t"]["clean"]), fmt(rr["t"]["simplify"])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
