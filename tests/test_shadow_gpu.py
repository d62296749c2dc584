"""The shadow post-pass on the device (kernels_shadow.hip): trgl_shadow_mask_image / trgl_image_modulate through TRGL_MEM_DEVICE, the
resident forms trgl_shadow_mask / trgl_framebuffer_modulate, their place in the context's stream, and the shim's demo, all against
tests/shadow_model.py bit for bit.

The kernels' own edges (csrc/launch.h, kernels_shadow.hip): k_shadow_mask works on blocks of SHADOW_TILE_W x SHADOW_TILE_H pixels, four
pixels per thread, each row shifted so that the mask's words are aligned - what is ragged depends on w, on the mask's address and on
the depths' offset modulo 16; a block without a finite depth leaves early.  k_modulate works on groups of four pixels from the first
word-aligned one, with the pixels before and behind them done by one thread."""
import os
import struct
import subprocess

import numpy as np
import pytest

import shadow_cases
import shadow_model
from tinyrenderder_amd import api
from tinyrenderder_amd.api import FLAT, Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_shadow")
E_INVALID, E_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    with Context(70, 45, 3, device=0) as c:
        yield c


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                 # the upload ran on torch's stream; the context's own stream waits for nobody
    return t


def params_of(case):
    _, _, M, _, bias, darkness, r = case
    return api.make_shadow_params(M, bias, darkness, r)


def model_mask(case):
    _, depth, M, zmap, bias, darkness, r = case
    return shadow_model.shadow_mask(depth, M, zmap, bias, darkness, r)


def device_mask(ctx, case):
    out = ctx.shadow_mask_image(params_of(case), to_device(case[1]), to_device(case[3]), device=True)
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", shadow_cases.threshold_cases() + shadow_cases.corner_tap_cases(), ids=lambda c: c[0])
def test_device_mask_equals_the_model_on_the_thresholds(ctx, case):
    got, want = device_mask(ctx, case), model_mask(case)
    assert np.array_equal(got, want), (case[0], got, want)


@pytest.mark.parametrize("frame", [(70, 45), (129, 67), (1, 1), (7, 300)], ids=lambda s: "%dx%d" % s)
def test_device_mask_on_ragged_frames_and_maps_of_other_sizes(ctx, frame):
    for k, (mw, mh) in enumerate(((33, 20), (200, 150), (1, 1), frame)):
        for r in (0, 1, 4):
            case = shadow_cases.random_case(*frame, mw, mh, r, 0.35 if r else 1.0, seed=50 + 3 * k + r)
            got, want = device_mask(ctx, case), model_mask(case)
            assert np.array_equal(got, want), (case[0], np.argwhere(got != want)[:5])
            assert np.array_equal(got, api.shadow_mask_image(params_of(case), case[1], case[3]))      # and the host path


def test_device_mask_background_blocks_next_to_live_ones(ctx):
    """129 x 67 is 5 x 3 blocks: only the pixels of x in 40..89, y in 5..29 have a depth, so whole blocks are background (they leave
    early), others hold a few live pixels, and the live region's edges cut through threads' groups of four."""
    name, depth, M, zmap, bias, darkness, r = shadow_cases.random_case(129, 67, 64, 64, 1, 0.8, seed=77)
    live = np.zeros(depth.shape, bool); live[5:30, 40:90] = True
    depth = np.where(live, np.where(np.isfinite(depth), depth, 0.25), np.inf)
    case = (name, depth, M, zmap, bias, darkness, r)
    got = device_mask(ctx, case)
    assert np.array_equal(got, model_mask(case))
    assert (got[~live] == 255).all() and (got[live] < 255).any()


def test_device_mask_at_every_base_offset_leaves_its_surroundings_alone(ctx):
    case = shadow_cases.random_case(70, 45, 33, 20, 1, 0.6, seed=5)
    want, n = model_mask(case), 70 * 45
    d, m = to_device(case[1]), to_device(case[3])
    for off in range(4):
        surround = np.random.default_rng(off).integers(0, 256, n + 40, dtype=np.uint8)
        buf = to_device(surround)
        out = buf[8 + off:8 + off + n].view(45, 70)
        assert out.data_ptr() % 4 == off
        ctx.shadow_mask_image(params_of(case), d, m, device=True, out=out)
        ctx.sync()
        back = buf.cpu().numpy()
        assert np.array_equal(back[8 + off:8 + off + n].reshape(45, 70), want), off
        assert np.array_equal(back[:8 + off], surround[:8 + off]) and np.array_equal(back[8 + off + n:], surround[8 + off + n:]), off


def test_device_mask_with_depths_8_but_not_16_byte_aligned(ctx):
    import torch
    for w, h in ((70, 45), (129, 67)):
        case = shadow_cases.random_case(w, h, 33, 20, 1, 0.6, seed=6)
        dbuf, mbuf = torch.zeros(w * h + 1, dtype=torch.float64, device="cuda"), torch.zeros(33 * 20 + 1, dtype=torch.float64, device="cuda")
        d, m = dbuf[1:].view(h, w), mbuf[1:].view(20, 33)
        d.copy_(torch.from_numpy(case[1])); m.copy_(torch.from_numpy(case[3]))
        torch.cuda.synchronize()
        assert d.data_ptr() % 16 == 8 and m.data_ptr() % 16 == 8
        out = ctx.shadow_mask_image(params_of(case), d, m, device=True)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy(), model_mask(case))


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_device_modulate_at_every_base_offset(ctx, bpp):
    rng = np.random.default_rng(40 + bpp)
    for (w, h) in ((70, 45), (129, 67), (1, 1), (3, 1), (5, 2)):
        img = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
        mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
        mask[rng.random((h, w)) < 0.3] = 255
        want = shadow_model.modulate(img, mask)
        assert np.array_equal(api.image_modulate(img, mask), want)
        for off in range(4):
            surround = rng.integers(0, 256, img.size + 40, dtype=np.uint8)
            buf = to_device(surround)
            t = buf[8 + off:8 + off + img.size].view(h, w, bpp)
            t.copy_(to_device(img))
            mbuf = to_device(np.concatenate([np.zeros(3 - off, np.uint8), mask.reshape(-1)]))       # the mask at the opposite offset
            import torch
            torch.cuda.synchronize()
            ctx.image_modulate(t, mbuf[3 - off:].view(h, w), device=True)
            ctx.sync()
            back = buf.cpu().numpy()
            assert np.array_equal(back[8 + off:8 + off + img.size].reshape(img.shape), want), (w, h, off)
            assert np.array_equal(back[:8 + off], surround[:8 + off]) and np.array_equal(back[8 + off + img.size:], surround[8 + off + img.size:])


def draw_view(c, sc, view):
    c.draw(FLAT, sc[view]["clip"], colors=sc[view]["colors"])


@pytest.mark.parametrize("bpp", [3, 1, 4])
def test_resident_mask_and_framebuffer_modulate(bpp):
    W, H = 129, 67
    sc = shadow_cases.demo_scene(W, H)
    M = api.shadow_matrix(sc["light"]["mv"], sc["light"]["proj"], sc["vp"], sc["cam"]["mv"], sc["cam"]["proj"], sc["vp"])
    p = api.make_shadow_params(M, 0.01, 0.6, 1)
    with Context(W, H, bpp, device=0) as c:
        draw_view(c, sc, "light")
        zl = c.read_zbuffer()
        c.zbuffer_snapshot(1)
        c.clear()
        draw_view(c, sc, "cam")
        fb, zc = c.read_framebuffer(), c.read_zbuffer()
        want = shadow_model.shadow_mask(zc, M, zl, 0.01, 0.6, 1)
        assert (want < 255).any() and (want[np.isfinite(zc)] == 255).any()
        host = c.shadow_mask(p, slot=1)
        dev = c.shadow_mask(p, slot=1, device=True)
        c.sync()
        assert np.array_equal(host, want) and np.array_equal(dev.cpu().numpy(), want)
        # queued draws and a pending clear come first: the same sequence without a read in between
        c.clear()
        draw_view(c, sc, "cam")
        assert np.array_equal(c.shadow_mask(p, slot=1), want)
        st = c.stats()                                                        # (the second camera pass counted its triangles too)
        c.framebuffer_modulate(dev, device=True)
        got = c.read_framebuffer()
        assert np.array_equal(got, shadow_model.modulate(fb, want)) and not np.array_equal(got, fb)
        assert np.array_equal(c.read_zbuffer().view(np.uint64), zc.view(np.uint64)) and c.stats() == st
        c.write_framebuffer(fb)
        c.framebuffer_modulate(want)                                          # a host mask
        assert np.array_equal(c.read_framebuffer(), shadow_model.modulate(fb, want))


def test_mask_blur_modulate_back_to_back(ctx):
    """mask -> image_blur (bpp 1) -> modulate queued without a sync in between equal the same three steps on the host."""
    case = shadow_cases.random_case(70, 45, 33, 20, 1, 0.9, seed=9)
    img = np.random.default_rng(10).integers(0, 256, (45, 70, 3), dtype=np.uint8)
    d, m, t = to_device(case[1]), to_device(case[3]), to_device(img)
    mask = ctx.shadow_mask_image(params_of(case), d, m, device=True)
    ctx.image_blur(mask.view(45, 70, 1), 3, device=True)
    ctx.image_modulate(t, mask, device=True)
    ctx.sync()
    host_mask = api.image_blur(api.shadow_mask_image(params_of(case), case[1], case[3])[..., None], 3)
    assert np.array_equal(mask.cpu().numpy(), host_mask[..., 0]) and not np.array_equal(host_mask[..., 0], model_mask(case))
    assert np.array_equal(t.cpu().numpy(), api.image_modulate(img, host_mask[..., 0]))


def test_state_and_argument_errors():
    p = api.make_shadow_params(np.eye(4))
    out = np.zeros((64, 64), np.uint8)
    call = lambda c, slot, params=p: c.L.trgl_shadow_mask(c.h, params, slot, out.ctypes.data, api.MEM_HOST)
    with Context(64, 64, 3, device=0) as c:
        assert call(c, 2) == E_STATE                                          # an empty slot
        assert call(c, -1) == E_INVALID and call(c, api.MAX_Z_SNAPSHOTS) == E_INVALID
        c.zbuffer_snapshot(2)
        assert call(c, 2) == 0 and (out == 255).all()                         # nothing was drawn: all background
        assert call(c, 2, api.make_shadow_params(np.eye(4), pcf_radius=5)) == E_INVALID
        assert c.L.trgl_shadow_mask(c.h, p, 2, None, api.MEM_DEVICE) == E_INVALID
        assert c.L.trgl_framebuffer_modulate(c.h, None, api.MEM_HOST) == E_INVALID
        assert c.L.trgl_framebuffer_modulate(c.h, out.ctypes.data, 5) == E_INVALID
        c.set_strip(0, 32)
        assert call(c, 2) == E_STATE                                          # a strip context
        c.set_strip(0, 64)
        assert call(c, 2) == 0
        c.set_interleave(32, 1, 2)
        assert call(c, 2) == E_STATE                                          # a band context


def test_shim_demo_equals_the_python_sequence(tmp_path):
    """examples/demo_shadow.cpp: light pass, snapshot, camera pass, gl_shadow_mask, TGAImage::gaussian_blur, gl_modulate.  Its three TGAs
    against the same sequence through Python on the scene the demo dumped."""
    assert os.path.exists(DEMO), "examples/demo_shadow not built: run __graft_entry__.build()"
    W, H = 160, 120
    prefix = str(tmp_path / "shadow")
    r = subprocess.run([DEMO, prefix, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(prefix + "_scene.bin", "rb").read()
    assert raw[:8] == b"TRSHSC01"
    w, h, ntri, pcf, blur, _ = struct.unpack_from("<6i", raw, 8)
    assert (w, h) == (W, H)
    off = 32
    take = lambda dtype, n: np.frombuffer(raw, dtype, n, off)
    bias, darkness = take(np.float64, 2); off += 16
    M = take(np.float64, 16).reshape(4, 4); off += 128
    vps = []
    for _ in range(2):
        vps.append(take(np.float64, 16).reshape(4, 4)); off += 128
    passes = []
    for _ in range(2):
        clip = take(np.float64, ntri * 12).reshape(ntri, 12); off += ntri * 96
        col = take(np.uint32, ntri); off += ntri * 4
        passes.append((clip, col))
    assert off == len(raw)
    sc = shadow_cases.demo_scene(W, H)
    assert np.allclose(passes[0][0], sc["light"]["clip"], rtol=1e-12, atol=1e-12) and np.allclose(passes[1][0], sc["cam"]["clip"], rtol=1e-12, atol=1e-12)
    p = api.make_shadow_params(M, bias, darkness, pcf)
    with Context(W, H, 3, device=0) as c:
        c.set_viewport(vps[0])
        c.draw(FLAT, passes[0][0], colors=passes[0][1])
        c.zbuffer_snapshot(1)
        c.clear()
        c.set_viewport(vps[1])
        c.draw(FLAT, passes[1][0], colors=passes[1][1])
        frame = c.read_framebuffer()
        mask = c.shadow_mask(p, slot=1, device=True)
        c.image_blur(mask.view(H, W, 1), blur, device=True)
        c.framebuffer_modulate(mask, device=True)
        shadowed = c.read_framebuffer()
        mask = mask.cpu().numpy()
    assert (mask < 255).any() and not np.array_equal(frame, shadowed)
    for name, img in (("frame", frame), ("mask", mask[..., None]), ("shadowed", shadowed)):
        assert open(prefix + "_%s.tga" % name, "rb").read() == api.tga_encode(img), name
