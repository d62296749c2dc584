"""trgl_image_blur / trgl_image_scale on images in device memory and trgl_framebuffer_blur on the resident frame (kernels_image.hip) against
the golden file of the reference's own compiled tgaimage.cpp:246-324 and against tests/image_ops_model.py fed trgl_gaussian_kernel's
weights, byte for byte; their place in the context's stream; the shim's gl_gaussian_blur.

The kernels' own edges (csrc/launch.h): the horizontal pass works on tiles of BLUR_H_BYTES bytes of a row x BLUR_H_ROWS rows, the vertical
pass on BLUR_V_BYTES bytes x BLUR_V_ROWS rows, the scale on SCALE_BYTES x SCALE_ROWS; up to BLUR_LDS_RADIUS the taps come from LDS, above
it from global memory."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import image_ops_model
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_image_ops")
G = np.load(os.path.join(ROOT, "tests", "golden", "image_ops_golden.npz"))
META = json.loads(str(G["meta"]))
_LAUNCH_H = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "launch.h")).read()
K = {n: int(v) for n, v in re.findall(r"\b(BLUR_LDS_RADIUS|BLUR_H_BYTES|BLUR_H_ROWS|BLUR_V_BYTES|BLUR_V_ROWS|SCALE_BYTES|SCALE_ROWS) = (\d+)", _LAUNCH_H)}
SW = K["BLUR_LDS_RADIUS"]
E_STATE = -4


@pytest.fixture(scope="module")
def ctx():
    with Context(101, 67, 3, device=0) as c:
        yield c


def to_device(img):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img, np.uint8)).cuda()
    torch.cuda.synchronize()                 # the upload ran on torch's stream; the context's own stream waits for nobody
    return t


def device_blur(ctx, img, radius):
    t = to_device(img)
    ctx.image_blur(t, radius, device=True)
    ctx.sync()
    return t.cpu().numpy()


def model_blur(img, radius):
    return image_ops_model.gaussian_blur(img, api.gaussian_kernel(radius) if radius > 0 else None)


def random_image(w, h, bpp, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, bpp), dtype=np.uint8)


def test_constants_were_found():
    assert len(K) == 7 and META["switch_radius"] == SW


@pytest.mark.parametrize("name", META["images"])
def test_device_blur_equals_the_reference(ctx, name):
    img = G["img/" + name]
    for r in META["radii"]:
        got = device_blur(ctx, img, r)
        want = G["blur/%s/%d" % (name, r)]
        assert np.array_equal(got, want), (name, r, np.argwhere(got != want)[:5])


def edge_shapes():
    hb, hr, vb, vr = K["BLUR_H_BYTES"], K["BLUR_H_ROWS"], K["BLUR_V_BYTES"], K["BLUR_V_ROWS"]
    out = []
    for d in (-1, 0, 1):
        out.append((hb + d, vr + d, 1))                    # a row of tile - 1, tile, tile + 1 bytes; as many rows
        out.append((vb + d, hr - d, 1))
        out.append((hb // 4 + d, vr - d, 4))               # bpp = 4: whole pixels at the tile edge
        out.append((vb // 4 + d, 2 * vr + d, 4))
    out += [(hb // 3, vr, 3), (hb // 3 + 1, vr + 1, 3)]    # bpp = 3: 255 and 258 bytes, a pixel straddles the tile edge
    out += [(vb // 3, 2 * vr - 1, 3), (vb // 3 + 1, hr + 1, 3), (2 * hb // 3 + 1, 3, 3)]
    out += [(1, 200, 3), (300, 1, 3), (1, 1, 4), (1, 1, 1), (2, 2, 3)]
    return out


@pytest.mark.parametrize("radius", [1, 7, SW, SW + 1])
def test_device_blur_equals_the_model_at_the_tile_edges(ctx, radius):
    for n, (w, h, bpp) in enumerate(edge_shapes()):
        img = random_image(w, h, bpp, 100 + n)
        got, want = device_blur(ctx, img, radius), model_blur(img, radius)
        assert np.array_equal(got, want), (w, h, bpp, radius, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_device_blur_largest_image_both_sides_of_the_switch(ctx, bpp):
    img = random_image(300, 200, bpp, 7 + bpp)
    a, b = device_blur(ctx, img, SW), device_blur(ctx, img, SW + 1)
    assert np.array_equal(a, model_blur(img, SW)) and np.array_equal(b, model_blur(img, SW + 1))
    assert not np.array_equal(a, b) and not np.array_equal(a, img)


def test_device_blur_host_path_agrees_and_radius_zero_does_nothing(ctx):
    img = random_image(97, 45, 3, 5)
    assert np.array_equal(device_blur(ctx, img, 4), api.image_blur(img, 4))
    assert np.array_equal(device_blur(ctx, img, 0), img) and np.array_equal(device_blur(ctx, img, -3), img)


def test_device_blur_at_an_odd_address_leaves_its_surroundings_alone(ctx):
    import torch
    img = random_image(67, 41, 3, 11)
    n = img.size
    surround = np.random.default_rng(12).integers(0, 256, n + 600, dtype=np.uint8)
    buf = to_device(surround)
    t = buf[1:1 + n].view(41, 67, 3)
    t.copy_(torch.from_numpy(img))
    torch.cuda.synchronize()
    assert t.data_ptr() % 2 == 1
    ctx.image_blur(t, 5, device=True)
    ctx.sync()
    back = buf.cpu().numpy()
    assert np.array_equal(back[1:1 + n].reshape(img.shape), model_blur(img, 5))
    assert back[0] == surround[0] and np.array_equal(back[1 + n:], surround[1 + n:])


@pytest.mark.parametrize("k", [i for i, c in enumerate(META["scale"]) if c[3]])
def test_device_scale_equals_the_reference(ctx, k):
    name, w2, h2, _ = META["scale"][k]
    out = ctx.image_scale(to_device(G["img/" + name]), w2, h2, device=True)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), G["scale/%d" % k])


def test_device_scale_equals_the_model_at_the_tile_edges(ctx):
    sb, sr = K["SCALE_BYTES"], K["SCALE_ROWS"]
    shapes = [(sb + d, sr + d, 1) for d in (-1, 0, 1)] + [(sb // 4 + d, 2 * sr - d, 4) for d in (-1, 0, 1)]
    shapes += [(sb // 3, sr, 3), (sb // 3 + 1, 3 * sr + 1, 3), (1, 1, 3), (300, 200, 3), (7, 300, 4)]
    for n, (w2, h2, bpp) in enumerate(shapes):
        img = random_image(67 + n, 41 + 2 * n, bpp, 200 + n)
        out = ctx.image_scale(to_device(img), w2, h2, device=True)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy(), image_ops_model.scale(img, w2, h2)), (w2, h2, bpp)
    # into the middle of a larger tensor, one byte off: the bytes around the result stay
    img = random_image(67, 41, 3, 31)
    surround = np.random.default_rng(32).integers(0, 256, 40 * 30 * 3 + 300, dtype=np.uint8)
    buf = to_device(surround)
    out = buf[1:1 + 40 * 30 * 3].view(30, 40, 3)
    ctx.image_scale(to_device(img), 40, 30, device=True, out=out)
    ctx.sync()
    back = buf.cpu().numpy()
    assert np.array_equal(back[1:1 + 3600].reshape(30, 40, 3), image_ops_model.scale(img, 40, 30))
    assert back[0] == surround[0] and np.array_equal(back[3601:], surround[3601:])


def test_device_scale_false_cases_raise(ctx):
    t = to_device(G["img/random_bpp3"])
    for w2, h2 in ((0, 10), (10, -1)):
        with pytest.raises(api.TrglError, match=r"\(-1\)"):
            ctx.image_scale(t, w2, h2, device=True)
    with pytest.raises(api.TrglError, match=r"\(-1\)"):                       # overlapping images
        ctx.image_scale(t, 67, 41, device=True, out=t)


def test_framebuffer_blur_after_a_draw(ctx):
    W, H = 101, 67
    clip, col = scenes.random_triangles(300, W, H, seed=3, rmin=2, rmax=30, perspective_w=True)
    ctx.clear()
    ctx.reset_stats()
    ctx.draw(FLAT, clip, colors=col)
    before, z, st = ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats()
    assert len(np.unique(before.reshape(-1, 3), axis=0)) > 10
    ctx.framebuffer_blur(6)
    got = ctx.read_framebuffer()
    assert np.array_equal(got, model_blur(before, 6)) and not np.array_equal(got, before)
    assert np.array_equal(ctx.read_zbuffer().view(np.uint64), z.view(np.uint64)) and ctx.stats() == st
    # queued draws and a pending clear come first: clear + draw + blur without a read in between gives the same frame
    ctx.clear()
    ctx.draw(FLAT, clip, colors=col)
    ctx.framebuffer_blur(6)
    assert np.array_equal(ctx.read_framebuffer(), got)
    ctx.framebuffer_blur(0)                                                    # radius <= 0: nothing happens
    assert np.array_equal(ctx.read_framebuffer(), got)


def test_framebuffer_blur_refused_on_a_strip_or_bands():
    with Context(64, 64, 3, device=0) as c:
        c.set_strip(0, 32)
        assert c.L.trgl_framebuffer_blur(c.h, 2) == E_STATE
        c.set_strip(0, 64)
        assert c.L.trgl_framebuffer_blur(c.h, 2) == 0
        c.set_interleave(32, 1, 2)
        assert c.L.trgl_framebuffer_blur(c.h, 2) == E_STATE


def test_back_to_back_calls_compose(ctx):
    """Two blurs of one image and a scale of the result, queued without a sync between them: the scratch image and the weights (another
    radius each time) are reused in stream order."""
    img = random_image(131, 77, 3, 21)
    t = to_device(img)
    ctx.image_blur(t, 2, device=True)
    ctx.image_blur(t, SW + 2, device=True)
    ctx.image_blur(t, 5, device=True)
    out = ctx.image_scale(t, 50, 90, device=True)
    ctx.sync()
    want = model_blur(model_blur(model_blur(img, 2), SW + 2), 5)
    assert np.array_equal(t.cpu().numpy(), want)
    assert np.array_equal(out.cpu().numpy(), image_ops_model.scale(want, 50, 90))


def test_shim_gl_gaussian_blur(tmp_path):
    """examples/demo_image_ops.cpp in device mode: the image is the shim's framebuffer, gl_gaussian_blur() then gl_flush()."""
    assert os.path.exists(DEMO), "examples/demo_image_ops not built: run __graft_entry__.build()"
    img = G["img/random_bpp3"]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(b"TRGIMG01" + struct.pack("<6i", 67, 41, 3, 9, 1, 1) + img.tobytes())
    r = subprocess.run([DEMO, "device", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(img.shape), G["blur/random_bpp3/9"])
