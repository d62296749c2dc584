"""Times of the box-filter resolve and of render-to-texture on one MI355X (profiles/resolve_probe_summary.txt and DESIGN.md §6 record them).

  python profiles/resolve_probe.py [--size 8192] [--reps 200] [--host-reps 3] [--tris 20000]

A --size x --size RGB frame, resolved with factor 2 and factor 4.  Device times are HIP events on the context's stream around --reps
back-to-back calls after a warm-up, divided by --reps; the paths through the host are timed by the host clock, median of --host-reps.
  (a) trgl_texture_from_framebuffer into a slot that already holds a texture of that size (the reuse path: one kernel)
  (b) trgl_framebuffer_resolve into device memory
  (c) a device-to-device hipMemcpyAsync of as many bytes as the kernel reads plus writes (W * H * bpp + that / f^2), on the same stream;
      (c2) one of half as many bytes, which moves the same total traffic (a copy reads and writes every byte)
  (d) the route (a) replaces: read_framebuffer, the host box filter, upload_texture
  (e) a whole SSAA frame - clear, draw --tris triangles at --size, resolve with factor 2, the small image on the host - against the same
      scene drawn at --size / 2 and read back
Every device result is compared with the host filter, byte for byte, before anything is timed.  Under `rocprofv3 --kernel-trace --stats`
the same script lists k_box_filter; counters come from a run of their own."""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tinyrenderder_amd import api, scenes  # noqa: E402
from tinyrenderder_amd.api import FLAT, Context  # noqa: E402


def device_ms(ctx, fn, reps, warm=10):
    """fn() reps times between two events on the context's stream; ms per call"""
    s = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(warm):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    for _ in range(reps):
        fn()
    t1.record(s)
    t1.synchronize()
    ctx.sync()
    return t0.elapsed_time(t1) / reps


def host_ms(fn, reps, warm=1):
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if k >= warm:
            ts.append(dt * 1e3)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--tris", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resolve_probe: no GPU; there is nothing to measure without one")
    n = a.size
    res = {}
    clip, col = scenes.random_triangles(a.tris, n, n, seed=11, rmin=4, rmax=n // 64, perspective_w=True)
    with Context(n, n, 3) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        ctx.clear((20, 40, 60, 255))
        ctx.draw(FLAT, clip, colors=col)
        fb = ctx.read_framebuffer()
        for f in (2, 4):
            n2 = n // f
            t0 = time.perf_counter(); want = api.image_downsample(fb, f); host_filter_ms = (time.perf_counter() - t0) * 1e3
            out = torch.empty((n2, n2, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.framebuffer_resolve(f, device=True, out=out); ctx.sync()
            assert np.array_equal(out.cpu().numpy(), want), f
            ctx.texture_from_framebuffer(0, f)
            assert np.array_equal(ctx.selftest_sampler(0, [[0.5, 0.5]])[0, :3], want[n2 // 2, n2 // 2]), f
            nsrc, ndst = n * n * 3, n2 * n2 * 3
            ca, cb = (torch.empty(nsrc + ndst, dtype=torch.uint8, device="cuda") for _ in range(2))
            torch.cuda.synchronize()

            def copy(nbytes):
                with torch.cuda.stream(stream):
                    cb[:nbytes].copy_(ca[:nbytes], non_blocking=True)

            r = dict(size=n, factor=f, bytes_read=nsrc, bytes_written=ndst, host_filter_once_ms=host_filter_ms)
            r["a_texture_from_framebuffer_ms"] = device_ms(ctx, lambda: ctx.texture_from_framebuffer(0, f), a.reps)
            r["b_framebuffer_resolve_device_ms"] = device_ms(ctx, lambda: ctx.framebuffer_resolve(f, device=True, out=out), a.reps)
            r["c_memcpy_read_plus_written_bytes_ms"] = device_ms(ctx, lambda: copy(nsrc + ndst), a.reps)
            r["c2_memcpy_same_traffic_ms"] = device_ms(ctx, lambda: copy((nsrc + ndst) // 2), a.reps)
            r["d_read_host_filter_upload"] = host_ms(lambda: ctx.upload_texture(1, api.image_downsample(ctx.read_framebuffer(), f)), a.host_reps)
            r["kernel_GBps"] = (nsrc + ndst) / (r["b_framebuffer_resolve_device_ms"] * 1e-3) / 1e9
            r["b_over_c"] = r["b_framebuffer_resolve_device_ms"] / r["c_memcpy_read_plus_written_bytes_ms"]
            r["b_over_c2"] = r["b_framebuffer_resolve_device_ms"] / r["c2_memcpy_same_traffic_ms"]
            res["factor_%d" % f] = r
            print("factor_%d" % f, json.dumps(r), flush=True)
            del out, ca, cb, want

        def ssaa_frame():
            ctx.clear((20, 40, 60, 255))
            ctx.draw(FLAT, clip, colors=col)
            return ctx.framebuffer_resolve(2)

        e = dict(ssaa_draw_at_size_resolve_read=host_ms(ssaa_frame, a.host_reps + 2))
    half = n // 2
    clip2, col2 = scenes.random_triangles(a.tris, half, half, seed=11, rmin=4, rmax=half // 64, perspective_w=True)
    with Context(half, half, 3) as ctx:
        def plain_frame():
            ctx.clear((20, 40, 60, 255))
            ctx.draw(FLAT, clip2, colors=col2)
            return ctx.read_framebuffer()

        e["plain_draw_at_half_size_read"] = host_ms(plain_frame, a.host_reps + 2)
    res["e_whole_frame"] = e
    print("e_whole_frame", json.dumps(e), flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
