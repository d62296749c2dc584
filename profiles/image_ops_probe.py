"""Times of trgl_framebuffer_blur and trgl_image_scale on one MI355X (DESIGN.md §6 records the results).

  python profiles/image_ops_probe.py [--reps 50] [--host-reps 2] [--size 4096]

A --size x --size RGB frame.  Blur at radius 2, 8 and 32: the device call is `framebuffer_blur(r)` followed by a sync, by the host clock;
next to it what a caller had to do before for the same bytes - read_framebuffer, the host loop (trgl_image_blur with TRGL_MEM_HOST, one
core), write_framebuffer.  Scale to half and to twice the size: `image_scale(device=True)` + sync against the copy to the host, the host
loop (trgl_image_scale with TRGL_MEM_HOST) and the copy back.  Every device result is compared with the host's, byte for byte, before
anything is timed.  Warm-up first, then medians over --reps repetitions (--host-reps for the paths through the host; one for radius 32);
the spread is printed as min / max.  pixel_taps_per_s = size^2 * (2 r + 1) * 2 passes / median.
Under `rocprofv3 --kernel-trace --stats` the same script lists k_blur_h, k_blur_v and k_scale: take kernel times from that run and the
call times from a run without the profiler."""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tinyrenderder_amd import api  # noqa: E402
from tinyrenderder_amd.api import Context  # noqa: E402


def timed(fn, reps, warm=3):
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if k >= warm:
            ts.append(dt)
    return dict(median_ms=statistics.median(ts) * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_ops_probe: no GPU; there is nothing to measure without one")
    n = a.size
    img = np.random.default_rng(5).integers(0, 256, (n, n, 3), dtype=np.uint8)
    res = {}
    with Context(n, n, 3) as ctx:
        for r in (2, 8, 32):
            t0 = time.perf_counter(); want = api.image_blur(img, r); host_once = time.perf_counter() - t0
            ctx.write_framebuffer(img)
            ctx.framebuffer_blur(r)
            assert np.array_equal(ctx.read_framebuffer(), want), r

            def device():
                ctx.framebuffer_blur(r); ctx.sync()

            def through_host():
                ctx.write_framebuffer(api.image_blur(ctx.read_framebuffer(), r)); ctx.sync()

            dev = timed(device, a.reps)
            host_reps = 1 if r >= 32 else a.host_reps
            res["blur_r%d" % r] = dict(device=dev, read_host_loop_write=timed(through_host, host_reps, warm=0 if r >= 32 else 1),
                                       host_loop_once_ms=host_once * 1e3, pixel_taps_per_s=n * n * (2 * r + 1) * 2 / (dev["median_ms"] * 1e-3))
            print("blur_r%d" % r, json.dumps(res["blur_r%d" % r]), flush=True)
        src = torch.from_numpy(img).cuda()
        for n2 in (n // 2, n * 2):
            out = torch.empty((n2, n2, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter(); want = api.image_scale(img, n2, n2); host_once = time.perf_counter() - t0
            ctx.image_scale(src, n2, n2, device=True, out=out); ctx.sync()
            assert np.array_equal(out.cpu().numpy(), want), n2

            def device():
                ctx.image_scale(src, n2, n2, device=True, out=out); ctx.sync()

            def through_host():
                out.copy_(torch.from_numpy(api.image_scale(src.cpu().numpy(), n2, n2))); torch.cuda.synchronize()

            key = "scale_%d_to_%d" % (n, n2)
            res[key] = dict(device=timed(device, a.reps), copy_host_loop_copy=timed(through_host, a.host_reps, warm=1), host_loop_once_ms=host_once * 1e3)
            print(key, json.dumps(res[key]), flush=True)
            del out, want
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
