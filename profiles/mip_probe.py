"""Times of the mip chain build, of the filtered samplers and of the LOD stage on one MI355X (profiles/mip_probe_summary.txt and DESIGN.md §6
record them).

  python profiles/mip_probe.py [--reps 200] [--frame 4096] [--tris 1000000]

Device times are HIP events on the context's stream around --reps back-to-back calls after a warm-up, divided by --reps.
Chain builds, for a 4096 x 4096 and a 1024 x 1024 RGB texture:
  (a) trgl_texture_mipmaps on a slot that already has room for the levels (the reuse path: kernels and no host wait)
  (b) the same levels by successive trgl_image_downsample(..., 2) calls on device images, where that call is defined (both sides >= 2):
      the route k_mip_chain replaces
  (c) a device-to-device copy of as many bytes as (a) reads plus writes
Sampling cost, on a --frame x --frame RGB frame covered by one textured quad under perspective (a 1024 x 1024 texture with a chain):
  (d) the flush of a user kind that calls trgl_sample2D_trilinear(..., trgl_mip_lod(...)) against the same body with trgl_sample2D; the
      context's own phase clocks give the raster phase and the raster kernel alone, so phase minus kernel is the shade kernel plus the
      two small bookkeeping kernels
  (e) trgl_lod_stage over --tris triangles (K = 24) against a device-to-device copy of the bytes it moves (96 + 48 read, 32 written each)
Every device result is compared with the host path, byte for byte, before anything is timed.  Repeated calls over the same buffers
replay from the last-level cache; the figures are those of that replay."""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tinyrenderder_amd import api  # noqa: E402
from tinyrenderder_amd.api import Context, make_uniforms  # noqa: E402

NEAREST = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    return trgl_sample2D(in, 0, uv).bgra | 0xff000000u;
}
"""
TRILINEAR = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    int w = 1, h = 1;
    trgl_texture_levels(in, 0, &w, &h);
    return trgl_sample2D_trilinear(in, 0, uv, trgl_mip_lod(in.bar, v + 20, w, h)).bgra | 0xff000000u;
}
"""


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


def chain_builds(ctx, n, reps):
    stream = torch.cuda.ExternalStream(ctx.stream)
    img = np.random.default_rng(n).integers(0, 256, (n, n, 3), dtype=np.uint8)
    want = api.image_mipmaps(img)
    ws, hs, offs, total = api.mip_layout(n, n, 3)
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    got = ctx.image_mipmaps(d_img, device=True)
    ctx.sync()
    assert np.array_equal(got.cpu().numpy(), want)
    ctx.upload_texture(0, img)
    ctx.texture_mipmaps(0)                                   # the first build allocates; every later one reuses
    for l in (1, len(ws) - 1):
        uv = [[0.5, 0.5]]
        assert np.array_equal(ctx.selftest_sampler_lod(0, uv, float(l), api.SAMPLE_LEVEL), api.image_sample(img, want, uv, float(l), api.SAMPLE_LEVEL))
    levels = [d_img] + [torch.empty((hs[l], ws[l], 3), dtype=torch.uint8, device="cuda") for l in range(1, len(ws))]
    torch.cuda.synchronize()

    def successive():
        for l in range(1, len(levels)):
            ctx.image_downsample(levels[l - 1], 2, device=True, out=levels[l])
    successive(); ctx.sync()
    for l in range(1, len(levels)):
        assert np.array_equal(levels[l].cpu().numpy().reshape(-1), want[offs[l]:offs[l] + levels[l].numel()]), l
    written = sum(ws[l] * hs[l] * 3 for l in range(1, len(ws)))
    moved = n * n * 3 + written                              # level 0 read once, every level written once (the later launches re-read a few KB)
    ca, cb = (torch.empty(moved, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()

    def copy():
        with torch.cuda.stream(stream):
            cb.copy_(ca, non_blocking=True)
    r = dict(size=n, levels=len(ws), bytes_read=n * n * 3, bytes_written=written)
    r["a_texture_mipmaps_reuse_ms"] = device_ms(ctx, lambda: ctx.texture_mipmaps(0), reps)
    r["a2_image_mipmaps_device_ms"] = device_ms(ctx, lambda: ctx.image_mipmaps(d_img, device=True, out=got), reps)
    r["b_successive_image_downsample_ms"] = device_ms(ctx, successive, reps)
    r["c_memcpy_read_plus_written_bytes_ms"] = device_ms(ctx, copy, reps)
    r["a_over_b"] = r["a_texture_mipmaps_reuse_ms"] / r["b_successive_image_downsample_ms"]
    r["a_over_c"] = r["a_texture_mipmaps_reuse_ms"] / r["c_memcpy_read_plus_written_bytes_ms"]
    r["a_GBps"] = moved / (r["a_texture_mipmaps_reuse_ms"] * 1e-3) / 1e9
    return r


def sampling_cost(frame, reps):
    f = 3.0
    proj = np.eye(4); proj[3, 2] = -1.0 / f
    verts = np.zeros((4, 14))
    verts[:, :3] = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (9.0, 9.0, -24.0), (-9.0, 9.0, -24.0)]      # fills the frame, w from 1 to 9
    verts[:, 4] = 1.0
    verts[:, 6:8] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    tex = np.random.default_rng(5).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    vp = np.eye(4); vp[0, 0] = vp[0, 3] = frame / 2.0; vp[1, 1] = vp[1, 3] = frame / 2.0
    out = {}
    with Context(frame, frame, 3) as ctx:
        ctx.init_viewport(0, 0, frame, frame)
        ctx.upload_texture(0, tex)
        ctx.texture_mipmaps(0)
        clip, vary = ctx.vertex_stage(-1, make_uniforms(np.eye(4)), proj, verts, faces)
        vary = api.lod_stage(vp, clip, np.ascontiguousarray(vary), 0, 20)
        d_clip, d_vary = torch.from_numpy(clip).cuda(), torch.from_numpy(vary).cuda()
        torch.cuda.synchronize()
        for name, src in (("nearest", NEAREST), ("trilinear", TRILINEAR)):
            kind = ctx.register_shader(src, 24)

            def draw():
                ctx.clear((0, 0, 0, 255))
                ctx.draw(kind, d_clip, d_vary, device=True)
                ctx.flush()
            draw(); ctx.sync()
            fb = ctx.read_framebuffer()
            covered = int((fb.reshape(-1, 3) != (0, 0, 0)).any(axis=1).sum())
            ms = device_ms(ctx, draw, reps)
            ctx.set_profiling(True)
            ctx.reset_phase_ms()
            for _ in range(reps):
                draw()
            ctx.sync()
            phases, flushes = ctx.phase_ms()
            ctx.set_profiling(False)
            out[name] = dict(flush_ms=ms, covered_pixels=covered, raster_phase_ms=phases[2] / flushes, raster_kernel_ms=phases[4] / flushes,
                             shade_and_bookkeeping_ms=(phases[2] - phases[4]) / flushes)
    out["trilinear_minus_nearest_shade_ms"] = out["trilinear"]["shade_and_bookkeeping_ms"] - out["nearest"]["shade_and_bookkeeping_ms"]
    out["trilinear_over_nearest_shade"] = out["trilinear"]["shade_and_bookkeeping_ms"] / out["nearest"]["shade_and_bookkeeping_ms"]
    return out


def lod_stage_cost(ctx, n, reps):
    stream = torch.cuda.ExternalStream(ctx.stream)
    rng = np.random.default_rng(3)
    W = rng.uniform(0.5, 5.0, (n, 3))
    clip = np.zeros((n, 3, 4))
    clip[..., :3] = rng.uniform(-1, 1, (n, 3, 3)) * W[..., None]
    clip[..., 3] = W
    clip = clip.reshape(n, 12)
    vary = rng.uniform(0, 1, (n, 24))
    vp = np.eye(4); vp[0, 0] = vp[0, 3] = 512.0; vp[1, 1] = vp[1, 3] = 384.0
    d_clip, d_vary = torch.from_numpy(clip).cuda(), torch.from_numpy(vary).cuda()
    torch.cuda.synchronize()
    ctx.lod_stage(vp, d_clip, d_vary, 0, 20, device=True); ctx.sync()
    want = api.lod_stage(vp, clip, vary, 0, 20)
    assert np.array_equal(d_vary.cpu().numpy().view(np.uint64), want.view(np.uint64))
    moved = n * (96 + 48 + 32)
    ca, cb = (torch.empty(moved, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()

    def copy():
        with torch.cuda.stream(stream):
            cb.copy_(ca, non_blocking=True)
    r = dict(triangles=n, bytes_moved=moved)
    r["lod_stage_ms"] = device_ms(ctx, lambda: ctx.lod_stage(vp, d_clip, d_vary, 0, 20, device=True), reps)
    r["memcpy_moved_bytes_ms"] = device_ms(ctx, copy, reps)
    r["stage_over_copy"] = r["lod_stage_ms"] / r["memcpy_moved_bytes_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frame", type=int, default=4096)
    ap.add_argument("--tris", type=int, default=1000000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mip_probe: no GPU; there is nothing to measure without one")
    res = {}
    with Context(64, 64, 3) as ctx:
        for n in (4096, 1024):
            res["chain_%d" % n] = chain_builds(ctx, n, a.reps)
            print("chain_%d" % n, json.dumps(res["chain_%d" % n]), flush=True)
        res["lod_stage"] = lod_stage_cost(ctx, a.tris, a.reps)
        print("lod_stage", json.dumps(res["lod_stage"]), flush=True)
    res["sampling"] = sampling_cost(a.frame, max(a.reps // 4, 10))
    print("sampling", json.dumps(res["sampling"]), flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
