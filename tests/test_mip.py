"""The host paths of the mipmapped textures (include/trgl.h, "Mipmapped textures") against tests/mip_model.py, byte for byte and bit for
bit: trgl_mip_layout, trgl_image_mipmaps, trgl_image_sample, trgl_lod_stage, the host's compile of trgl_mip_lod, and every refusal.
Needs no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import box_model
import mip_cases as cases
import mip_model as model
from tinyrenderder_amd import api

E_INVALID, E_UNSUPPORTED = -1, -5
MEM_HOST, MEM_DEVICE = 0, 1


# ---- layout and chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp", cases.BPPS)
def test_layout_equals_the_model(bpp):
    for w, h in cases.SIZES + [(65535, 1), (1, 65535), (4096, 4096), (1000, 600)]:
        ws, hs, offs, total = api.mip_layout(w, h, bpp)
        assert (ws, hs, offs, total) == model.layout(w, h, bpp), (w, h)
        assert len(ws) == 1 + int(math.floor(math.log2(max(w, h)))) and all(o % 16 == 0 for o in offs) and (len(ws) < 2 or offs[1] == 0)


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_random_chains_equal_the_model(bpp):
    for w, h in cases.SIZES:
        img = cases.texture(w, h, bpp)
        levels = model.chain(img)
        got = api.image_mipmaps(img)
        assert np.array_equal(got, model.pack(levels)), (w, h, bpp)
        if w >= 2 and h >= 2:
            l1 = got[:levels[1].size].reshape(levels[1].shape)
            assert np.array_equal(l1, api.image_downsample(img, 2)) and np.array_equal(l1, box_model.box_filter(img, 2))


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_the_padding_between_levels_is_not_touched(bpp):
    L = api.load_library()
    for w, h in cases.SIZES:
        img = cases.texture(w, h, bpp, seed=5)
        total = api.mip_layout(w, h, bpp)[3]
        buf = np.full(total + 32, 0xA5, np.uint8)
        assert L.trgl_image_mipmaps(None, img.ctypes.data, w, h, bpp, buf[16:].ctypes.data, MEM_HOST) == 0
        want = np.full(total + 32, 0xA5, np.uint8)
        want[16:16 + total] = model.pack(model.chain(img), fill=0xA5)
        assert np.array_equal(buf, want), (w, h, bpp)


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_all_255_stays_255_at_every_level(bpp):
    for w, h in [(65, 63), (1, 130), (257, 3)]:
        got = api.image_mipmaps(np.full((h, w, bpp), 255, np.uint8))
        assert (got[model.level_mask(w, h, bpp)] == 255).all()


@pytest.mark.parametrize("offset", (-1, 0, 1))
@pytest.mark.parametrize("bpp", cases.BPPS)
def test_sums_around_the_rounding_threshold(bpp, offset):
    """2 x 2 sums one below, on and one above q * 4 + 2 (the tie rounds up), and 2 x 1 / 1 x 2 sums around q * 2 + 1."""
    rng = np.random.default_rng(10 * bpp + offset)
    img = box_model.image_with_sums(box_model.tie_sums((9, 11, bpp), 2, rng, offset), 2, rng)
    q = model.chain(img)[1]
    assert np.array_equal(api.image_mipmaps(img)[:q.size].reshape(q.shape), q)
    for shape in ((1, 24, bpp), (24, 1, bpp)):                                   # a side of 1: pairs
        pairs = rng.integers(0, 255, (12, bpp)) * 2 + 1 + offset
        a = rng.integers(0, 2, (12, bpp)) + pairs // 2 - (pairs % 2 == 0)
        a = np.clip(a, np.maximum(pairs - 255, 0), np.minimum(pairs, 255))
        strip = np.stack([a, pairs - a], axis=1).reshape(shape).astype(np.uint8)
        lv = model.chain(strip)[1]
        assert np.array_equal(lv.reshape(12, bpp).astype(np.int64), (pairs + 1) // 2)
        assert np.array_equal(api.image_mipmaps(strip)[:lv.size].reshape(lv.shape), lv)


# ---- filtered samples ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=cases.SAMPLE_TEXTURES, ids=lambda p: "%dx%dx%d" % p)
def sampled(request):
    w, h, bpp = request.param
    img = cases.texture(w, h, bpp, seed=9)
    levels = model.chain(img)
    return img, levels, api.image_mipmaps(img), cases.sample_uv(w, h, len(levels))


@pytest.mark.parametrize("mode", (api.SAMPLE_LEVEL, api.SAMPLE_LINEAR))
def test_level_and_linear_samples_equal_the_model(sampled, mode):
    img, levels, chain, uv = sampled
    for lod in cases.level_lods(len(levels)):
        got, want = api.image_sample(img, chain, uv, lod, mode), model.sample(levels, uv, lod, mode)
        assert np.array_equal(got, want), (mode, lod, uv[np.argwhere((got != want).any(axis=1))[:3, 0]])


def test_trilinear_samples_equal_the_model(sampled):
    img, levels, chain, uv = sampled
    uv = uv[::3]
    for lod in cases.trilinear_lods(len(levels)):
        got, want = api.image_sample(img, chain, uv, lod, api.SAMPLE_TRILINEAR), model.sample(levels, uv, lod, 2)
        assert np.array_equal(got, want), (lod, uv[np.argwhere((got != want).any(axis=1))[:3, 0]])


def test_level_zero_nearest_is_the_unfiltered_sampler(sampled):
    """mode 0 at level 0 is IShader::sample2D's rule: at texel centres it returns the texel itself, channels above bpp zero."""
    img, levels, chain, _ = sampled
    h, w, bpp = img.shape
    uv = np.array([((x + 0.5) / w, (y + 0.5) / h) for y in range(h) for x in range(w)])
    got = api.image_sample(img, chain, uv, 0.0, api.SAMPLE_LEVEL)
    assert np.array_equal(got[:, :bpp], img.reshape(-1, bpp)) and (got[:, bpp:4] == 0).all() and (got[:, 4] == bpp).all()


def test_a_texture_without_a_chain_has_one_level():
    img = cases.texture(13, 7, 3, seed=9)
    uv = cases.sample_uv(13, 7, 1)
    for mode, lod in ((0, 3.0), (1, 2.0), (2, 2.5)):
        assert np.array_equal(api.image_sample(img, None, uv, lod, mode), model.sample([img], uv, lod, mode))


# ---- the LOD stage ------------------------------------------------------------------------------------------------------------------
VP = cases.viewport(48, 40)


@pytest.mark.parametrize("K,uv_offset,out_offset", cases.LOD_LAYOUTS)
def test_lod_stage_equals_the_model(K, uv_offset, out_offset):
    clip, uv = cases.all_lod_cases()
    vary = cases.lod_rows(K, uv_offset, out_offset, clip, uv, seed=K + uv_offset)
    want = model.lod_stage(VP, clip, vary, uv_offset, out_offset)
    before = vary.copy()
    got = api.lod_stage(VP, clip, vary, uv_offset, out_offset)
    assert got is vary and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    keep = np.ones(K, bool); keep[out_offset:out_offset + 4] = False
    assert np.array_equal(got[:, keep].view(np.uint64), before[:, keep].view(np.uint64))      # the other doubles keep their bits


def test_lod_stage_zeroing_cases_write_positive_zeros():
    clip, uv, names = cases.lod_zeroing_cases()
    vary = cases.lod_rows(10, 0, 6, clip, uv, seed=3)
    api.lod_stage(VP, clip, vary)
    for t, name in enumerate(names):
        assert (vary[t, 6:10].view(np.uint64) == 0).all(), name
        assert model.lod_constants(VP, clip[t], uv[t]) == (0.0, 0.0, 0.0, 0.0), name


def test_lod_constant_times_w_cubed_is_the_uv_footprint():
    """The identity behind the stage, checked on the model against central differences of the perspective-correct uv over the screen:
    |det d(u, v) / d(x, y)| = c * wp^3 (to 6 digits; the stage itself is compared bit for bit above)."""
    clip, uv = cases.lod_triangles(8, 11, True)
    for t in range(8):
        c, W0, W1, W2 = model.lod_constants(VP, clip[t], uv[t])
        v = clip[t].reshape(3, 4)
        s = np.array([(VP @ (p / p[3]))[:2] for p in v])
        T = np.array([[s[0, 0], s[1, 0], s[2, 0]], [s[0, 1], s[1, 1], s[2, 1]], [1, 1, 1]])

        def at(x, y):
            b = np.linalg.solve(T, [x, y, 1.0])
            pc = b / v[:, 3] / (b / v[:, 3]).sum()
            return pc @ uv[t].reshape(3, 2), pc @ v[:, 3]
        x, y = s.mean(axis=0)
        e = 1e-4
        du = (at(x + e, y)[0] - at(x - e, y)[0]) / (2 * e)
        dv = (at(x, y + e)[0] - at(x, y - e)[0]) / (2 * e)
        det = abs(du[0] * dv[1] - du[1] * dv[0])
        assert det == pytest.approx(c * at(x, y)[1] ** 3, rel=1e-6)


# ---- trgl_mip_lod -------------------------------------------------------------------------------------------------------------------
def lod_of_r(r):
    """k and bar such that the function sees exactly r: wp = 1, k[0] = r, a 1 x 1 texture."""
    return [1.0, 0.0, 0.0], [r, 1.0, 1.0, 1.0]


def test_mip_lod_at_and_around_powers_of_two():
    rs = [1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.0, -4.0, np.nan, np.inf, 1e308, 1e-300]
    for k in (1, 2, 3, 10, 52, 53, 100, 1023):
        p = 2.0 ** k
        rs += [p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)]
    bar = np.array([lod_of_r(r)[0] for r in rs]); kk = np.array([lod_of_r(r)[1] for r in rs])
    got = api.mip_lod(bar, kk, 1, 1)
    want = np.array([model.mip_lod(bar[i], kk[i], 1, 1) for i in range(len(rs))])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[0] == 0.0 and got[1] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and got[5] == 0.0 and got[6] == 64.0
    assert api.mip_lod([lod_of_r(4.0)[0]], [lod_of_r(4.0)[1]], 1, 1)[0] == 1.0 and api.mip_lod([[1, 0, 0]], [[1.0, 1, 1, 1]], 4, 4)[0] == 2.0


def test_mip_lod_is_within_a_twentieth_of_half_log2():
    """0.5 * (e + m) against 0.5 * log2(r): the chord of log2 over one octave lies below it by at most 0.0861, half of that is 0.043."""
    rng = np.random.default_rng(8)
    n = 4000
    bar = rng.dirichlet((1, 1, 1), n)
    k = np.concatenate([10.0 ** rng.uniform(-12, 0, (n, 1)), rng.uniform(0.5, 20.0, (n, 3))], axis=1)
    got = api.mip_lod(bar, k, 512, 256)
    want = np.array([model.mip_lod(bar[i], k[i], 512, 256) for i in range(n)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    wp = (bar[:, 0] * k[:, 1] + bar[:, 1] * k[:, 2]) + bar[:, 2] * k[:, 3]
    r = k[:, 0] * wp ** 3 * 512 * 256
    big = r > 1.0
    assert big.sum() > n // 4 and (~big).sum() > n // 20 and (got[~big] == 0.0).all()
    assert np.abs(got[big] - 0.5 * np.log2(r[big])).max() < 0.05


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = api.load_library()
    img = np.zeros((4, 4, 3), np.uint8)
    buf = np.zeros(256, np.uint8)
    n, tot = C.c_int(), C.c_size_t()
    for w, h, bpp, rc in ((0, 4, 3, E_INVALID), (4, -1, 3, E_INVALID), (4, 4, 2, E_INVALID), (4, 4, 0, E_INVALID),
                          (65536, 1, 1, E_UNSUPPORTED), (1, 65536, 4, E_UNSUPPORTED), (65535, 65535, 1, E_UNSUPPORTED)):
        assert L.trgl_mip_layout(w, h, bpp, C.byref(n), None, None, None, C.byref(tot)) == rc, (w, h, bpp)
        assert L.trgl_image_mipmaps(None, img.ctypes.data, w, h, bpp, buf.ctypes.data, MEM_HOST) == rc, (w, h, bpp)
    assert L.trgl_mip_layout(4, 4, 3, None, None, None, None, None) == 0
    p, q = img.ctypes.data, buf.ctypes.data
    assert L.trgl_image_mipmaps(None, p, 4, 4, 3, q, 7) == E_INVALID                      # bad mem_kind
    assert L.trgl_image_mipmaps(None, p, 4, 4, 3, q, MEM_DEVICE) == E_INVALID             # a device call without a context
    assert L.trgl_image_mipmaps(None, None, 4, 4, 3, q, MEM_HOST) == E_INVALID
    assert L.trgl_image_mipmaps(None, p, 4, 4, 3, None, MEM_HOST) == E_INVALID
    assert L.trgl_image_mipmaps(None, p, 4, 4, 3, p + 40, MEM_HOST) == E_INVALID          # overlap
    assert L.trgl_image_mipmaps(None, p, 1, 1, 3, None, MEM_HOST) == 0                    # L = 1: nothing to write
    uv, lod, out = np.zeros((1, 2)), np.zeros(1), np.zeros(5, np.uint8)
    args = (uv.ctypes.data, lod.ctypes.data)
    assert L.trgl_image_sample(p, q, 4, 4, 3, 3, *args, 3, 1, out.ctypes.data) == E_INVALID          # bad mode
    assert L.trgl_image_sample(p, q, 4, 4, 3, 0, *args, 0, 1, out.ctypes.data) == E_INVALID          # no level
    assert L.trgl_image_sample(p, None, 4, 4, 3, 3, *args, 0, 1, out.ctypes.data) == E_INVALID       # levels without a chain
    assert L.trgl_image_sample(None, q, 4, 4, 3, 3, *args, 0, 1, out.ctypes.data) == E_INVALID
    assert L.trgl_image_sample(p, q, 4, 4, 5, 3, *args, 0, 1, out.ctypes.data) == E_INVALID
    assert L.trgl_image_sample(p, None, 4, 4, 3, 1, *args, 0, 1, out.ctypes.data) == 0


def test_lod_stage_refusals():
    L = api.load_library()
    vp = np.ascontiguousarray(VP).ctypes.data_as(C.POINTER(C.c_double))
    clip, vary = np.zeros((2, 12)), np.zeros((2, 64))
    c, v = clip.ctypes.data, vary.ctypes.data

    def call(K=10, uo=0, oo=6, n=2, cp=c, vptr=v, mem=MEM_HOST, m=vp):
        return L.trgl_lod_stage(None, m, cp, vptr, n, K, uo, oo, mem)
    assert call() == 0
    assert call(mem=5) == E_INVALID and call(mem=MEM_DEVICE) == E_INVALID and call(m=None) == E_INVALID
    assert call(K=-1) == E_INVALID and call(K=65) == E_INVALID and call(K=9) == E_INVALID
    for uo, oo in ((-1, 6), (0, -1), (5, 6), (0, 7), (0, 5), (3, 0), (0, 0), (2, 4)):
        assert call(K=10, uo=uo, oo=oo) == E_INVALID, (uo, oo)
    assert call(K=10, uo=4, oo=0) == 0 and call(K=64, uo=58, oo=0) == 0 and call(K=64, uo=0, oo=60) == 0
    assert call(cp=None) == E_INVALID and call(vptr=None) == E_INVALID and call(cp=c + 4) == E_INVALID and call(vptr=v + 4) == E_INVALID
    assert call(n=2 ** 31) == E_UNSUPPORTED
    assert call(n=0, cp=None, vptr=None) == 0                                            # no array is read


# ---- the shim's host side -----------------------------------------------------------------------------------------------------------
SHIM_PROGRAM = r"""
#include <cstdio>
#include "trgl_shaders.h"
int main(int argc, char** argv) {
    TGAImage img(13, 7, TGAImage::RGB);
    for (int y = 0; y < 7; ++y) for (int x = 0; x < 13; ++x) img.set(x, y, TGAColor(uint8_t(x * 7 + y * 13), uint8_t(x * y + 58), uint8_t(200 - 9 * x + y), 255));
    std::vector<uint8_t> chain;
    int levels = 0;
    if (!trgl_image::mipmaps(img, &chain, &levels) || levels != 4) return 2;
    double uv[40][2], lod[40];
    for (int i = 0; i < 40; ++i) { uv[i][0] = (i % 8) / 7.0; uv[i][1] = (i / 8) / 4.0; lod[i] = i * 0.085 - 0.2; }
    uint8_t texels[40 * 5];
    if (!gl_image_sample(img, chain, &uv[0][0], lod, 2, 40, texels)) return 3;
    init_viewport(0, 0, 48, 40);
    double clip[2][12] = { { -0.5, -0.5, 0.1, 1.0, 1.2, -0.8, 0.2, 2.0, 0.3, 2.1, -0.4, 3.0 }, { -0.9, -0.9, 0.0, 1.0, 0.9, -0.9, 0.0, 1.0, 0.0, 0.9, 0.0, 1.0 } };
    double vary[2][10] = { { 0, 0, 1, 0, 0.5, 1, 7, 7, 7, 7 }, { 0.25, 0.5, 2, 0.5, 1, 3, 7, 7, 7, 7 } };
    if (!gl_lod_stage(&clip[0][0], &vary[0][0], 2, 10, 0, 6)) return 4;
    if (gl_lod_stage(&clip[0][0], &vary[0][0], 2, 10, 0, 3)) return 5;      // overlapping ranges are refused
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 6;
    std::fwrite(img.buffer(), 1, 13 * 7 * 3, f); std::fwrite(chain.data(), 1, chain.size(), f);
    std::fwrite(texels, 1, sizeof(texels), f); std::fwrite(vary, 1, sizeof(vary), f);
    return std::fclose(f) == 0 ? 0 : 7;
}
"""


def test_shim_host_functions_give_the_same_bytes(tmp_path):
    """trgl_image::mipmaps, gl_image_sample and gl_lod_stage of the shim, compiled with g++ and run without a GPU."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "tinyrenderder_amd")
    src, exe, out = tmp_path / "shim_mip.cpp", tmp_path / "shim_mip", tmp_path / "out.bin"
    src.write_text(SHIM_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(lib, "shim"), "-o", str(exe), str(src),
                        "-L", lib, "-ltrgl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    data = np.fromfile(out, np.uint8)
    img = data[:273].reshape(7, 13, 3)
    levels = model.chain(img)
    total = model.layout(13, 7, 3)[3]
    assert np.array_equal(data[273:273 + total], model.pack(levels))
    i = np.arange(40)
    uv = np.stack([(i % 8) / 7.0, (i // 8) / 4.0], -1)
    assert np.array_equal(data[273 + total:273 + total + 200].reshape(40, 5), model.sample(levels, uv, i * 0.085 - 0.2, 2))
    vary = data[273 + total + 200:].view(np.float64).reshape(2, 10)
    clip = [[-0.5, -0.5, 0.1, 1.0, 1.2, -0.8, 0.2, 2.0, 0.3, 2.1, -0.4, 3.0], [-0.9, -0.9, 0.0, 1.0, 0.9, -0.9, 0.0, 1.0, 0.0, 0.9, 0.0, 1.0]]
    before = np.array([[0, 0, 1, 0, 0.5, 1, 7, 7, 7, 7], [0.25, 0.5, 2, 0.5, 1, 3, 7, 7, 7, 7]], np.float64)
    assert np.array_equal(vary.view(np.uint64), model.lod_stage(VP, clip, before, 0, 6).view(np.uint64)) and (vary[:, 6] > 0).all()
