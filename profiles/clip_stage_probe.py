"""The clip stage (trgl_clip_stage on device arrays: k_clip_count, k_clip_scan_chunks, k_clip_scan_top, k_clip_scatter and the 8-byte count) on two workloads:
  head : the head stand-in, 327680 faces through k_vertex_stage (K = 24) under a projection whose near plane passes through the mesh,
         clipped at that near plane with the PHONG layout;
  soup : 10 M FLAT triangles (K = 0, colours), clipped at z >= 0, which passes through the soup.
Against it, on the same device in the same process, alternating: k_vertex_stage over as many faces (the head's own mesh; for the soup an
unshared mesh of 10 M faces), and device-to-device copies that move as many bytes as the stage reads plus writes.
Times are HIP events on the context's stream around one call, medians; bytes are the algorithm's, computed from n, n_out and K.
   python profiles/clip_stage_probe.py [--quick] [--kernel-trace]
--quick: smaller workloads, a rehearsal.  --kernel-trace: the measurement runs in a child process, and a second child (--once: one
warm-up and one timed call each) runs under rocprofv3 --kernel-trace, from which the four kernels' own durations are added.
A probe, not a test: it prints its summary."""
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')

QUICK, ONCE = "--quick" in sys.argv, "--once" in sys.argv
if "--kernel-trace" in sys.argv:        # the parent: it never touches the GPU
    import csv, glob, subprocess, tempfile
    extra = ["--quick"] if QUICK else []
    r = subprocess.run([sys.executable, __file__] + extra, timeout=900)
    if r.returncode != 0:
        raise SystemExit("clip_stage_probe: the measuring child failed (%d)" % r.returncode)
    out = tempfile.mkdtemp(prefix="clip_trace_")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, __file__, "--once"] + extra,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("clip_stage_probe: the run under rocprofv3 failed (%d)" % r.returncode)
    rows = []
    for path in glob.glob(out + "/**/*kernel_trace.csv", recursive=True):
        for row in csv.DictReader(open(path)):
            k = {name.lower(): v for name, v in row.items()}
            rows.append((int(k["start_timestamp"]), k["kernel_name"], (int(k["end_timestamp"]) - int(k["start_timestamp"])) / 1e3))
    rows.sort()
    print("kernel durations of a second child under rocprofv3 --kernel-trace (one launch each: the last of the three per workload):")
    for name in ("k_clip_count", "k_clip_scan_chunks", "k_clip_scan_top", "k_clip_scatter"):
        us = [d for _, kn, d in rows if name in kn]
        if len(us) != 6:
            raise SystemExit("clip_stage_probe: %d launches of %s in the trace, 6 expected" % (len(us), name))
        print("  %-20s head %9.1f us   soup %9.1f us" % (name, us[2], us[5]))
    raise SystemExit(0)

import math
import numpy as np, torch
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, PHONG, NEAR_PLANE, clip_layout, make_uniforms
import clip_model as cm
import test_next_rows as T

REPS, WARM = (1, 1) if ONCE else (20, 3)
W = H = 4096


def timed(stream, ctx, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    ctx.sync()
    return e0.elapsed_time(e1)


def report(name, ms, nbytes=None):
    ms = sorted(ms)
    line = f"{name:34s} {np.median(ms):8.3f} ms ({ms[0]:.3f} .. {ms[-1]:.3f}, {len(ms)} reps)"
    if nbytes:
        line += f"  {nbytes} bytes, {nbytes / np.median(ms) / 1e6:.0f} GB/s"
    print(line, flush=True)
    return float(np.median(ms))


def run(ctx, stream, name, plane, attrs, clip, vary, col, vertex_call):
    n, K = clip.shape[0], 0 if vary is None else vary.shape[1]
    outs = (torch.empty((2 * n, 12), dtype=torch.float64, device="cuda"), None if vary is None else torch.empty((2 * n, K), dtype=torch.float64, device="cuda"),
            None if col is None else torch.empty(2 * n, dtype=torch.int32, device="cuda"))
    per_tri = 96 + 8 * K + (4 if col is not None else 0)
    m = ctx.clip_stage(plane, clip, vary, col, attrs=attrs, device=True, out=outs)[3]
    # the stage reads the clip coordinates twice (count, scatter), everything else once, and writes n_out triangles
    nbytes = n * 96 + n * per_tri + m * per_tri
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    half = nbytes // 2
    t = dict(stage=[], vertex=[], copy_full=[], copy_half=[])
    with torch.cuda.stream(stream):
        for it in range(REPS + WARM):
            r = dict(stage=timed(stream, ctx, lambda: ctx.clip_stage(plane, clip, vary, col, attrs=attrs, device=True, out=outs)),
                     vertex=timed(stream, ctx, vertex_call),
                     copy_full=timed(stream, ctx, lambda: dst.copy_(src)),
                     copy_half=timed(stream, ctx, lambda: dst[:half].copy_(src[:half])))
            if it >= WARM or ONCE:
                for k, v in r.items():
                    t[k].append(v)
    print(f"{name}: n = {n}, K = {K}, n_out = {m} ({m / n:.3f} n), {per_tri} bytes per triangle")
    stage = report(f"  clip stage (4 kernels + count)", t["stage"], nbytes)
    report(f"  k_vertex_stage, {n} faces", t["vertex"])
    full = report(f"  D2D copy of the stage's bytes", t["copy_full"], 2 * nbytes)
    halfm = report(f"  D2D copy moving the stage's bytes", t["copy_half"], 2 * half)
    print(f"  stage / copy of its bytes = {stage / full:.2f}, stage / copy moving its bytes = {stage / halfm:.2f}", flush=True)
    # the result is the model's (on a prefix: the model is numpy)
    k = min(n, 20000)
    want = cm.clip_model(plane, clip[:k].cpu().numpy(), None if vary is None else vary[:k].cpu().numpy(), None, attrs)
    assert cm.same_bits(outs[0][:len(want[0])].cpu().numpy(), want[0]), "the stage's clip coordinates differ from the model"
    assert vary is None or cm.same_bits(outs[1][:len(want[0])].cpu().numpy(), want[1]), "the stage's varyings differ from the model"


level = 5 if QUICK else 7
hd, verts, idx = T._indexed_head(level, W, H)
u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
proj = scenes.perspective(math.tan(math.radians(30.0)), W / H, 2.6, 10.0)          # near plane at the head's centre (distance 2.6)
dv, di = torch.from_numpy(verts).cuda(), torch.from_numpy(idx.view(np.int32)).cuda()
nf = idx.shape[0]
with Context(W, H, 3) as ctx:
    stream = torch.cuda.ExternalStream(ctx.stream)
    hclip, hvary = torch.empty((nf, 12), dtype=torch.float64, device="cuda"), torch.empty((nf, 24), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vcall = lambda: ctx.vertex_stage(-1, u, proj, dv, di, device=True, out=(hclip, hvary))
    vcall(); ctx.sync()
    print(f"clip stage probe, one MI355X, one run; medians of {REPS} calls by HIP events on the context's stream", flush=True)
    run(ctx, stream, "head", NEAR_PLANE, clip_layout(PHONG), hclip, hvary, None, vcall)

    ns = 1_000_000 if QUICK else 10_000_000
    sclip, scol = scenes.random_triangles(ns, W, H, seed=12, rmin=1, rmax=16, perspective_w=True)
    dclip, dcol = torch.from_numpy(sclip).cuda(), torch.from_numpy(scol.view(np.int32)).cuda()
    del sclip
    sv = torch.rand((3 * ns, 8), dtype=torch.float64, device="cuda")
    si = torch.arange(3 * ns, dtype=torch.int32, device="cuda").view(ns, 3)
    vo = (torch.empty((ns, 12), dtype=torch.float64, device="cuda"), torch.empty((ns, 24), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    run(ctx, stream, "soup", (0.0, 0.0, 1.0, 0.0), [], dclip, None, dcol, lambda: ctx.vertex_stage(-1, u, proj, sv, si, device=True, out=vo))
