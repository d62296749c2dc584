"""The box filter on the device (kernels_resolve.hip) and what is built on it - trgl_image_downsample with TRGL_MEM_DEVICE,
trgl_framebuffer_resolve, trgl_texture_from_image / trgl_texture_from_framebuffer, the shim's gl_resolve / gl_texture_from_framebuffer -
against tests/box_model.py, byte for byte, and against the route they replace: read_framebuffer -> host filter -> upload_texture.

The kernel's own edges (read out of kernels_resolve.hip): a workgroup owns RES_BYTES consecutive bytes of RES_ROWS output rows, a thread
four of those bytes; no shape takes another path, factor 1 is a device-to-device copy."""
import os
import re
import subprocess

import numpy as np
import pytest

import box_model
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, PHONG, Context, make_uniforms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_rtt")
_SRC = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "kernels_resolve.hip")).read()
K = {n: int(v) for n, v in re.findall(r"\b(RES_BYTES|RES_ROWS|RES_THREADS) = (\d+)", _SRC)}
BPPS = (1, 3, 4)
FACTORS = (1, 2, 3, 4, 7, 16)
E_INVALID, E_STATE = -1, -4
MAX_IMAGE = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    with Context(50, 38, 3, device=0) as c:
        yield c


def to_device(img):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img, np.uint8)).cuda()
    torch.cuda.synchronize()                 # the upload ran on torch's stream; the context's own stream waits for nobody
    return t


def random_image(w, h, bpp, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, bpp), dtype=np.uint8)


def device_filter(ctx, img, f):
    out = ctx.image_downsample(to_device(img), f, device=True)
    ctx.sync()
    return out.cpu().numpy()


def test_constants_were_found():
    assert len(K) == 3 and K["RES_BYTES"] == 4 * K["RES_THREADS"] and K["RES_ROWS"] >= 2


def edge_shapes(bpp, f):
    """(w2, h2) of the outputs: a row of one tile - 1, exact, + 1 bytes (in whole pixels: for bpp = 3 a pixel straddles the tile edge);
    one tile - 1, exact, + 1 rows; both + 1; two tiles and a bit; one output byte, one output row."""
    tb, tr = K["RES_BYTES"], K["RES_ROWS"]
    px = tb // bpp
    out = [(px + d, 2) for d in (-1, 0, 1)] + [(5, tr + d) for d in (-1, 0, 1)]
    out += [(px + 1, tr + 1), ((2 * tb + 5) // bpp + 1, 1), (1, 1), (37, 1), (1, 9)]
    return out


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("bpp", BPPS)
def test_device_filter_equals_the_model_at_the_tile_edges(ctx, bpp, f):
    ran = 0
    for n, (w2, h2) in enumerate(edge_shapes(bpp, f)):
        w, h = w2 * f + (f - 1), h2 * f + (f - 1)             # w % f != 0 wherever f > 1
        if w * h * bpp > MAX_IMAGE:
            w, h = w2 * f + 1, h2 * f                          # the largest: no spare rows
        if w * h * bpp > MAX_IMAGE:
            continue                                           # (both + 1 at f = 16: each edge is covered on its own above)
        img = random_image(w, h, bpp, 100 * f + 10 * bpp + n)
        got, want = device_filter(ctx, img, f), box_model.box_filter(img, f)
        assert got.shape == (h2, w2, bpp) and np.array_equal(got, want), (w, h, bpp, f, np.argwhere(got != want)[:5])
        ran += 1
    assert ran >= 10
    img = random_image(f, f, bpp, 7)                           # f x f: one pixel
    assert np.array_equal(device_filter(ctx, img, f), box_model.box_filter(img, f))


@pytest.mark.parametrize("bpp,f,w2,h2", [(3, 2, 350, 5), (1, 3, 1031, 3), (4, 16, 23, 5), (3, 7, 9, 6), (3, 1, 41, 7), (1, 2, 3, 3)])
def test_any_alignment_and_the_bytes_around_dst_survive(ctx, bpp, f, w2, h2):
    """src and dst carved out of larger tensors at every byte offset 0..16 (each paired with a few offsets of the other); the bytes
    around dst keep their pattern."""
    import torch
    w, h = w2 * f + (f > 1), h2 * f + (f > 1)
    img = random_image(w, h, bpp, 300 + f)
    want = box_model.box_filter(img, f)
    nsrc, ndst = img.size, want.size
    pattern = np.random.default_rng(9).integers(0, 256, ndst + 96, dtype=np.uint8)
    sbuf = to_device(np.zeros(nsrc + 32, np.uint8))
    pairs = [(so, (5 * so + 3) % 17) for so in range(17)] + [((7 * do + 1) % 17, do) for do in range(17)]
    assert {p[0] for p in pairs} == set(range(17)) and {p[1] for p in pairs} == set(range(17))
    for so, do in pairs:
        src = sbuf[so:so + nsrc].view(h, w, bpp)
        src.copy_(torch.from_numpy(img))
        dbuf = to_device(pattern)
        dst = dbuf[32 + do:32 + do + ndst].view(h2, w2, bpp)
        assert src.data_ptr() % 16 == so % 16 and dst.data_ptr() % 16 == do % 16
        ctx.image_downsample(src, f, device=True, out=dst)
        ctx.sync()
        back = dbuf.cpu().numpy()
        assert np.array_equal(back[32 + do:32 + do + ndst].reshape(want.shape), want), (so, do)
        assert np.array_equal(back[:32 + do], pattern[:32 + do]) and np.array_equal(back[32 + do + ndst:], pattern[32 + do + ndst:]), (so, do)


@pytest.mark.parametrize("bpp", BPPS)
def test_extremes_on_the_device(ctx, bpp):
    w2 = K["RES_BYTES"] // bpp + 3
    img = np.full((16 * 2 + 5, 16 * w2 + 3, bpp), 255, np.uint8)               # the largest sum, across a tile edge
    got = device_filter(ctx, img, 16)
    assert got.shape == (2, w2, bpp) and (got == 255).all()
    rng = np.random.default_rng(40 + bpp)
    for f in (2, 4, 16):
        for offset in (-1, 0, 1):                                              # one below the tie, the tie (rounds up), one above
            sums = box_model.tie_sums((6, 45, bpp), f, rng, offset)
            img = box_model.image_with_sums(sums, f, rng)
            got = device_filter(ctx, img, f)
            assert np.array_equal(got, sums // (f * f) + (offset >= 0)) and np.array_equal(got, box_model.box_filter(img, f)), (f, offset)


def draw_flat(c, seed=3, n=40):
    clip, col = scenes.random_triangles(n, c.width, c.height, seed=seed, rmin=2, rmax=20, perspective_w=True)
    c.draw(FLAT, clip, colors=col)


@pytest.mark.parametrize("bpp", [3, 1, 4])
def test_framebuffer_resolve(bpp):
    W, H = 50, 38
    with Context(W, H, bpp, device=0) as c:
        c.clear()
        c.reset_stats()
        draw_flat(c)
        fb, z, st = c.read_framebuffer(), c.read_zbuffer(), c.stats()
        assert len(np.unique(fb.reshape(-1, bpp), axis=0)) > 5
        for f in (2, 3):
            want = box_model.box_filter(fb, f)
            assert np.array_equal(c.framebuffer_resolve(f), want)
            dev = c.framebuffer_resolve(f, device=True)
            c.sync()
            assert np.array_equal(dev.cpu().numpy(), want)
        assert np.array_equal(c.framebuffer_resolve(1), fb)
        assert np.array_equal(c.read_framebuffer(), fb) and np.array_equal(c.read_zbuffer().view(np.uint64), z.view(np.uint64)) and c.stats() == st
        # a pending clear and queued draws are honoured: clear + draw + resolve without a flush in between
        c.clear((9, 60, 200, 255))
        draw_flat(c, seed=4)
        got = c.framebuffer_resolve(2)
        fb2 = c.read_framebuffer()
        assert not np.array_equal(fb2, fb) and np.array_equal(got, box_model.box_filter(fb2, 2))
        c.clear((1, 2, 3, 4))                                  # a clear alone
        assert np.array_equal(c.framebuffer_resolve(16), box_model.box_filter(c.read_framebuffer(), 16))


def texel_grid(w, h):
    """uv that hit every texel once, row by row (the centre of each)."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([(xs.ravel() + 0.5) / w, (ys.ravel() + 0.5) / h], -1)


def sampled(c, slot, w, h, bpp):
    """The texture of `slot` as the device sampler fetches it, [h, w, bpp]; asserts its size and bpp through the fetch itself."""
    out = c.selftest_sampler(slot, texel_grid(w, h))
    assert (out[:, 4] == bpp).all() and (out[:, bpp:4] == 0).all()
    # a uv of exactly 1.0 clamps to the last texel: the texture is w x h and no larger
    assert np.array_equal(c.selftest_sampler(slot, [[1.0, 1.0]])[0], out[-1])
    return out[:, :bpp].reshape(h, w, bpp)


HEAD = {}


def head(W, H, distance):
    if (W, H, distance) not in HEAD:
        HEAD[(W, H, distance)] = scenes.head_standin(2, W, H, distance=distance)
    return HEAD[(W, H, distance)]


def draw_textured(c, slot, seed=0, distance=2.6):
    """A PHONG draw whose diffuse map is `slot` (a smaller distance: a larger head in front of the other)."""
    hd = head(c.width, c.height, distance)
    key = (0.3 + 0.1 * seed, 0.2, 1.0)
    c.draw(PHONG, hd["clip"], hd["varyings"], uniforms=make_uniforms(hd["model_view"], key, hd["fill"], hd["rim"], 1.0, tex_diffuse=slot))


def frame_state(c):
    return c.read_framebuffer(), c.read_zbuffer().view(np.uint64), c.stats()


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("bpp", BPPS)
def test_texture_content(bpp):
    W, H = 50, 38
    with Context(W, H, bpp, device=0) as c:
        c.clear((10, 20, 30, 255))
        draw_flat(c)
        fb = c.read_framebuffer()
        for slot, f in ((0, 1), (1, 2), (2, 3)):
            c.texture_from_framebuffer(slot, f)
            assert np.array_equal(sampled(c, slot, W // f, H // f, bpp), box_model.box_filter(fb, f)), f
        img = random_image(67, 45, bpp, 50 + bpp)
        for slot, f in ((3, 1), (4, 2), (1, 7)):               # slot 1: another size than it held
            c.texture_from_image(slot, to_device(img), f, device=True)
            assert np.array_equal(sampled(c, slot, 67 // f, 45 // f, bpp), box_model.box_filter(img, f)), f
        c.texture_from_image(5, img, 4)                        # the host path: upload_texture of the host-filtered image
        assert np.array_equal(sampled(c, 5, 16, 11, bpp), box_model.box_filter(img, 4))
        c.texture_from_image(5, img[..., 0] if bpp == 1 else img)
        assert np.array_equal(sampled(c, 5, 67, 45, bpp), img)
        assert np.array_equal(c.read_framebuffer(), fb)


@pytest.mark.parametrize("bpp", [3, 4])
def test_a_draw_sampling_the_capture_equals_the_host_route(bpp):
    W, H = 96, 72
    with Context(W, H, bpp, device=0) as a, Context(W, H, bpp, device=0) as b:
        for c in (a, b):
            c.clear((40, 90, 160, 255))
            c.reset_stats()
            draw_flat(c, seed=8, n=60)
        a.texture_from_framebuffer(2, 3)
        b.upload_texture(2, box_model.box_filter(b.read_framebuffer(), 3))
        for c in (a, b):
            c.clear()
            draw_textured(c, 2)
        sa, sb = frame_state(a), frame_state(b)
        assert same_state(sa, sb)
        assert len(np.unique(sa[0].reshape(-1, bpp), axis=0)) > 20           # the draw shows the texture, not one colour


def test_ordering_and_snapshot():
    """Draw A samples the slot and stays queued; the frame is captured into that very slot; draw B samples it.  A saw the old texels,
    B the new ones - as the immediate host route does.  Afterwards the frame changes and the texture does not."""
    W, H = 96, 72
    old = random_image(32, 24, 3, 61)
    with Context(W, H, 3, device=0) as a, Context(W, H, 3, device=0) as b:
        for c in (a, b):
            c.upload_texture(0, old)
            c.clear((5, 5, 5, 255))
            c.reset_stats()
        draw_textured(a, 0)                                    # queued, not flushed
        a.texture_from_framebuffer(0, 2)
        draw_textured(a, 0, seed=3, distance=2.0)
        draw_textured(b, 0)
        after_a = b.read_framebuffer()
        b.upload_texture(0, box_model.box_filter(after_a, 2))
        draw_textured(b, 0, seed=3, distance=2.0)
        sa, sb = frame_state(a), frame_state(b)
        assert same_state(sa, sb) and not np.array_equal(sa[0], after_a)      # B drew
        texels = sampled(a, 0, W // 2, H // 2, 3)
        assert np.array_equal(texels, box_model.box_filter(after_a, 2))
        # B did see new texels: with the old ones the frame is another
        b.clear((5, 5, 5, 255))
        b.upload_texture(0, old)
        draw_textured(b, 0)
        draw_textured(b, 0, seed=3, distance=2.0)
        assert not np.array_equal(b.read_framebuffer(), sa[0])
        # snapshot: clear, draw something else, blur - the slot keeps its texels
        a.clear((200, 100, 50, 255))
        draw_flat(a, seed=12)
        a.framebuffer_blur(3)
        assert not np.array_equal(a.read_framebuffer(), sa[0])
        assert np.array_equal(sampled(a, 0, W // 2, H // 2, 3), texels)


def test_feedback_loop_reuse_release_and_upload_compatibility():
    W, H = 96, 72
    with Context(W, H, 3, device=0) as a, Context(W, H, 3, device=0) as b:
        def frame(n, f):
            """frame n samples the capture of frame n - 1 (slot 1), then is captured itself with factor f"""
            for c in (a, b):
                c.clear((30 * n % 256, 80, 120, 255))
                draw_flat(c, seed=20 + n, n=10)
                draw_textured(c, 1, seed=n)
            a.texture_from_framebuffer(1, f)
            fb = b.read_framebuffer()
            b.upload_texture(1, box_model.box_filter(fb, f))
            assert np.array_equal(a.read_framebuffer(), fb), (n, f)
            assert np.array_equal(sampled(a, 1, W // f, H // f, 3), box_model.box_filter(fb, f)), (n, f)
        for n in range(3):                                     # the same size each time: the slot's memory is reused
            frame(n, 2)
        frame(3, 3)                                            # another size: the slot is released and allocated anew
        frame(4, 3)
        frame(5, 1)
        # upload_texture into a captured slot, a capture into an uploaded slot
        img = random_image(20, 10, 3, 71)
        a.upload_texture(1, img)
        assert np.array_equal(sampled(a, 1, 20, 10, 3), img)
        a.upload_texture(6, random_image(W // 2, H // 2, 3, 72))               # the capture's size: reused
        a.upload_texture(7, img)                                               # another size: released
        fb = a.read_framebuffer()
        for slot in (6, 7, 1):
            a.texture_from_framebuffer(slot, 2)
            assert np.array_equal(sampled(a, slot, W // 2, H // 2, 3), box_model.box_filter(fb, 2)), slot
        assert a.L.trgl_upload_texture(a.h, 6, None, 0, 0, 0) == 0              # emptied by upload_texture, filled by a capture
        assert (a.selftest_sampler(6, [[0.5, 0.5]])[0] == (255, 255, 255, 255, 4)).all()
        a.texture_from_framebuffer(6, 4)
        assert np.array_equal(sampled(a, 6, W // 4, H // 4, 3), box_model.box_filter(fb, 4))


def test_refusals_queue_nothing():
    import torch
    L = api.load_library()
    tex = random_image(8, 8, 3, 80)
    with Context(64, 64, 3, device=0) as c, Context(64, 64, 3, device=0) as control:
        for x in (c, control):
            x.clear((1, 2, 3, 255))
            x.reset_stats()
            draw_flat(x)
            x.upload_texture(0, tex)
            draw_flat(x, seed=5, n=25)                         # stays queued: a refused call neither drops nor reorders it
        out = torch.zeros(2 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p, n = out.data_ptr(), 64 * 64 * 3
        for slot in (-1, 16, 1 << 20):
            assert L.trgl_texture_from_framebuffer(c.h, slot, 1) == E_INVALID
            assert L.trgl_texture_from_image(c.h, slot, p, 8, 8, 3, 1, 1) == E_INVALID
        for f in (0, -2, 17, 65):                              # outside 1..16, and above W
            assert L.trgl_texture_from_framebuffer(c.h, 0, f) == E_INVALID
            assert L.trgl_texture_from_image(c.h, 0, p, 64, 64, 3, f, 1) == E_INVALID
            assert L.trgl_framebuffer_resolve(c.h, f, p, 1) == E_INVALID
            assert L.trgl_image_downsample(c.h, p, 64, 64, 3, f, p + n, 1) == E_INVALID
        assert L.trgl_framebuffer_resolve(c.h, 2, None, 1) == E_INVALID and L.trgl_framebuffer_resolve(c.h, 2, p, 5) == E_INVALID
        assert L.trgl_texture_from_image(c.h, 0, p, 8, 8, 2, 1, 1) == E_INVALID
        assert L.trgl_texture_from_image(c.h, 0, None, 8, 8, 3, 1, 1) == E_INVALID
        assert L.trgl_texture_from_image(c.h, 0, p, 8, 8, 3, 1, 9) == E_INVALID
        # overlapping device images: dst == src, dst beginning on the last byte of src, dst ending one byte into src; the frame itself
        assert L.trgl_image_downsample(c.h, p, 32, 32, 3, 2, p, 1) == E_INVALID
        assert L.trgl_image_downsample(c.h, p, 32, 32, 3, 2, p + 32 * 32 * 3 - 1, 1) == E_INVALID
        assert L.trgl_image_downsample(c.h, p + 16 * 16 * 3 - 1, 32, 32, 3, 2, p, 1) == E_INVALID
        assert b"overlap" in L.trgl_last_error(c.h)
        assert L.trgl_framebuffer_resolve(c.h, 2, c.L.trgl_framebuffer_device_ptr(c.h) + 100, 1) == E_INVALID
        c.sync()
        # nothing ran: no refused call wrote, the slot holds its texture, and the frame with the queued draw is the control's
        assert (out == 0).all().item()
        assert np.array_equal(sampled(c, 0, 8, 8, 3), tex)
        assert same_state(frame_state(c), frame_state(control))
    with Context(16, 8, 3, device=0) as c:                     # f > W, f > H
        assert L.trgl_texture_from_framebuffer(c.h, 0, 9) == E_INVALID and L.trgl_texture_from_framebuffer(c.h, 0, 16) == E_INVALID
        assert L.trgl_framebuffer_resolve(c.h, 9, 1, 1) == E_INVALID
        assert L.trgl_texture_from_framebuffer(c.h, 0, 8) == 0
        assert sampled(c, 0, 2, 1, 3).shape == (1, 2, 3)


def test_strip_and_band_contexts_are_refused():
    L = api.load_library()
    with Context(64, 64, 3, device=0) as c:
        host = np.zeros((32, 32, 3), np.uint8)
        c.set_strip(0, 32)
        assert L.trgl_texture_from_framebuffer(c.h, 0, 2) == E_STATE and L.trgl_framebuffer_resolve(c.h, 2, host.ctypes.data, 0) == E_STATE
        c.set_strip(0, 64)
        assert L.trgl_texture_from_framebuffer(c.h, 0, 2) == 0 and L.trgl_framebuffer_resolve(c.h, 2, host.ctypes.data, 0) == 0
        c.set_interleave(32, 1, 2)
        assert L.trgl_texture_from_framebuffer(c.h, 0, 2) == E_STATE and L.trgl_framebuffer_resolve(c.h, 2, host.ctypes.data, 0) == E_STATE
        c.texture_from_image(1, host, 2)                       # an image is nobody's rows: allowed
        assert sampled(c, 1, 16, 16, 3).shape == (16, 16, 3)


def test_shim_gl_resolve_and_gl_texture_from_framebuffer(tmp_path):
    """examples/demo_rtt.cpp in a child process: a frame drawn at twice the size through the shim, gl_resolve() into the small image,
    gl_texture_from_framebuffer() into a slot, a second frame with a quad that samples the slot.  Its files against the model, and
    against the same program taking the host route (gl_flush, gl_downsample, gl_upload_texture)."""
    assert os.path.exists(DEMO), "examples/demo_rtt not built: run __graft_entry__.build()"
    files = {}
    for mode in ("device", "host"):
        names = [str(tmp_path / f"{mode}_{n}.tga") for n in ("big", "ssaa", "screen")]
        r = subprocess.run([DEMO, mode] + names, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        # (write_tga_file stores the rows bottom-up and read_tga_file flips them back on top: [::-1] is TGAImage::buffer() order again)
        files[mode] = [np.ascontiguousarray(api.tga_decode(open(n, "rb").read())[::-1]) for n in names]
    big, ssaa, screen = files["device"]
    assert big.shape == (119, 163, 3) and len(np.unique(big.reshape(-1, 3), axis=0)) > 10
    want = box_model.box_filter(big, 2)
    assert ssaa.shape == (59, 81, 3) and np.array_equal(ssaa, want)
    assert len(np.unique(ssaa.reshape(-1, 3), axis=0)) > len(np.unique(big.reshape(-1, 3), axis=0))      # blended edges: colours the frame lacks
    hbig, hssaa, hscreen = files["host"]
    assert np.array_equal(hbig, big) and np.array_equal(hssaa, want) and np.array_equal(hscreen, screen)
    # the screen shows the texture: every colour inside the quad is one of its texels, and most texels appear
    inside = screen[40:90, 40:120].reshape(-1, 3)
    texels = {tuple(t) for t in want.reshape(-1, 3)}
    assert all(tuple(p) in texels for p in inside) and len({tuple(p) for p in inside}) > 10
