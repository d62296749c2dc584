"""Times of the scene entry points on one MI355X (DESIGN.md §6 records the results).

  python profiles/scene_probe.py [--reps 50] [--size 4096]

* trgl_mesh_bounds on meshes in device memory: the vertex buffer of the 327 k-face head stand-in (one record per face corner, stride
  14) and a 10 M-vertex buffer at stride 14.  The call is synchronous, so a host clock around it is the time of two launches, the
  48-byte copy and the stream sync; bytes/s is over n * stride * 8 (records of 112 bytes are read 24 bytes at a time, which touches
  every line: the whole buffer is the honest count).
* snapshot + restore of a size x size z-buffer (two device-to-device copies, then one sync) against read_zbuffer + write_zbuffer on
  the same context, the only way to do main.cpp:700,730 without them.
* the z-range pass of trgl_postprocess (k_zrange, the project's other streaming reduction) runs here too, once per repetition, so
  that a run of this script under `rocprofv3 --kernel-trace --stats` lists k_mesh_bounds, k_mesh_bounds_fold and k_zrange side by
  side; take kernel times from that run and the call times from a run without the profiler.
Warm-up first, then medians over --reps repetitions; the spread is printed as min / max."""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tinyrenderder_amd import scenes  # noqa: E402
from tinyrenderder_amd.api import FLAT, Context  # noqa: E402


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return dict(median_us=statistics.median(ts) * 1e6, min_us=min(ts) * 1e6, max_us=max(ts) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_probe: no GPU; there is nothing to measure without one")
    res = {}
    S = a.size
    with Context(S, S, 3) as ctx:
        hd = scenes.head_standin(7, S, S)                                   # 327 680 faces
        head = np.zeros((hd["positions"].shape[0] * 3, 14)); head[:, :3] = hd["positions"].reshape(-1, 3)
        big = np.random.default_rng(1).standard_normal((10_000_000, 14))
        for name, v in (("head_standin", head), ("10M_stride14", big)):
            t = torch.from_numpy(v).cuda(); torch.cuda.synchronize()
            want = ctx.mesh_bounds(v)
            got = ctx.mesh_bounds(t, device=True)
            assert all(np.array_equal(g.view(np.uint64), w.view(np.uint64)) for g, w in zip(got, want)), name
            r = timed(lambda: ctx.mesh_bounds(t, device=True), a.reps)
            r["bytes"] = v.nbytes; r["GB_per_s_of_call"] = v.nbytes / r["median_us"] / 1e3
            res["mesh_bounds_" + name] = r
            t0 = time.perf_counter(); ctx.mesh_bounds(v); res["mesh_bounds_host_" + name] = dict(once_us=(time.perf_counter() - t0) * 1e6)
            del t

        clip, col = scenes.random_triangles(20000, S, S, seed=3, rmin=8, rmax=256)
        ctx.draw(FLAT, clip, colors=col); ctx.sync()

        def on_device():
            ctx.zbuffer_snapshot(0); ctx.zbuffer_restore(0); ctx.sync()

        def through_host():
            ctx.write_zbuffer(ctx.read_zbuffer())

        z0 = ctx.read_zbuffer()
        res["snapshot_restore_device"] = timed(on_device, a.reps)
        res["read_write_zbuffer_host"] = timed(through_host, max(5, a.reps // 5), warm=2)
        assert np.array_equal(ctx.read_zbuffer().view(np.uint64), z0.view(np.uint64))
        res["zbuffer_bytes"] = S * S * 8
        # k_zrange + k_zimage + one S*S*3 copy to the host: listed for the kernel trace, not a like-for-like call time
        res["postprocess_zimage_call"] = timed(lambda: ctx.postprocess(zbuffer_image=True, ao=False, final=False), max(5, a.reps // 5), warm=2)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
