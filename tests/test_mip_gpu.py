"""The device paths of the mipmapped textures (include/trgl.h, "Mipmapped textures") on a real GPU, byte for byte and bit for bit against
tests/mip_model.py and against the host paths: trgl_image_mipmaps in device memory, trgl_texture_mipmaps and its ordering, the filtered
samplers of the user shaders, trgl_lod_stage, one frame end to end, and examples/demo_mipmap.

The kernel's own edges (read out of kernels_mip.hip): a workgroup owns a MIP_TILE x MIP_TILE block of a source level and writes the next
MIP_STEP levels of it; one launch per MIP_STEP levels."""
import os
import re
import subprocess

import numpy as np
import pytest

import box_model
import mip_cases as cases
import mip_model as model
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import FLAT, Context, make_uniforms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_mipmap")
_SRC = open(os.path.join(ROOT, "tinyrenderder_amd", "csrc", "kernels_mip.hip")).read()
K = {n: int(v) for n, v in re.findall(r"\b(MIP_TILE|MIP_STEP|MIP_THREADS) = (\d+)", _SRC)}
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def ctx():
    with Context(50, 38, 3, device=0) as c:
        yield c


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                 # the upload ran on torch's stream; the context's own stream waits for nobody
    return t


def test_constants_were_found():
    assert len(K) == 3 and K["MIP_TILE"] == 1 << K["MIP_STEP"] and K["MIP_STEP"] >= 2


# ---- trgl_image_mipmaps in device memory ---------------------------------------------------------------------------------------------
def edge_sizes():
    T = K["MIP_TILE"]
    sides = (T - 1, T, T + 1)
    return [(w, h) for w in sides for h in sides] + [(2 * T + 1, 3), (1, T + 2), (T + 2, 1), (2 * T + 3, T + 5)] + cases.SIZES


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_device_chains_equal_the_model_at_the_block_edges(ctx, bpp):
    T, S = K["MIP_TILE"], K["MIP_STEP"]
    sizes = edge_sizes()
    assert any(model.num_levels(w, h) - 1 > S and min(w, h) >> S == 0 for w, h in sizes)      # a second launch, and a side of 1 in it
    for w, h in sizes:
        img = cases.texture(w, h, bpp, seed=1)
        out = ctx.image_mipmaps(to_device(img), device=True)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy(), model.pack(model.chain(img))), (w, h, bpp)


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_extremes_on_the_device(ctx, bpp):
    T = K["MIP_TILE"]
    w, h = T + 3, T + 1
    out = ctx.image_mipmaps(to_device(np.full((h, w, bpp), 255, np.uint8)), device=True)
    ctx.sync()
    assert (out.cpu().numpy()[model.level_mask(w, h, bpp)] == 255).all()
    rng = np.random.default_rng(bpp)
    for offset in (-1, 0, 1):                                                  # one below the tie, the tie (rounds up), one above
        img = box_model.image_with_sums(box_model.tie_sums((T // 2 + 1, T // 2 + 2, bpp), 2, rng, offset), 2, rng)
        out = ctx.image_mipmaps(to_device(img), device=True)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy(), model.pack(model.chain(img))), offset


def _shapes_for_alignment():
    T = K["MIP_TILE"]
    return [(3, 2 * T + 1, 3), (1, T + 2, 1), (4, T + 1, 5), (3, 7, T + 3)]


@pytest.mark.parametrize("case", range(4))
def test_any_alignment_and_the_bytes_around_and_between_the_levels_survive(ctx, case):
    """src and dst carved out of larger tensors at every byte offset 0..16 (each paired with a few offsets of the other); the bytes
    around dst and the padding between the levels keep their pattern."""
    import torch
    bpp, w, h = _shapes_for_alignment()[case]
    img = cases.texture(w, h, bpp, seed=2)
    levels = model.chain(img)
    total = model.layout(w, h, bpp)[3]
    mask = model.level_mask(w, h, bpp)
    assert (~mask).any()                                                       # there is padding to protect
    pattern = np.random.default_rng(9).integers(0, 256, total + 96, dtype=np.uint8)
    sbuf = to_device(np.zeros(img.size + 32, np.uint8))
    pairs = [(so, (5 * so + 3) % 17) for so in range(17)] + [((7 * do + 1) % 17, do) for do in range(17)]
    assert {p[0] for p in pairs} == set(range(17)) and {p[1] for p in pairs} == set(range(17))
    for so, do in pairs:
        src = sbuf[so:so + img.size].view(h, w, bpp)
        src.copy_(torch.from_numpy(img))
        dbuf = to_device(pattern)
        dst = dbuf[32 + do:32 + do + total]
        assert src.data_ptr() % 16 == so % 16 and dst.data_ptr() % 16 == do % 16
        ctx.image_mipmaps(src, device=True, out=dst)
        ctx.sync()
        want = pattern.copy()
        want[32 + do:32 + do + total][mask] = model.pack(levels)[mask]
        assert np.array_equal(dbuf.cpu().numpy(), want), (so, do)


def test_device_refusals(ctx):
    import torch
    L = api.load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    assert L.trgl_image_mipmaps(ctx.h, p, 8, 8, 3, p + 100, 1) == E_INVALID and b"overlap" in L.trgl_last_error(ctx.h)
    assert L.trgl_image_mipmaps(ctx.h, p, 8, 8, 2, p + 1024, 1) == E_INVALID
    assert L.trgl_image_mipmaps(ctx.h, p, 65536, 1, 1, p + 1024, 1) == E_UNSUPPORTED
    assert L.trgl_image_mipmaps(ctx.h, None, 8, 8, 3, p + 1024, 1) == E_INVALID
    for slot in (-1, 16):
        assert L.trgl_texture_mipmaps(ctx.h, slot) == E_INVALID
    assert L.trgl_texture_mipmaps(ctx.h, 15) == E_STATE                          # an empty slot
    ctx.sync()
    assert (buf == 0).all().item()


# ---- trgl_texture_mipmaps ------------------------------------------------------------------------------------------------------------
def texel_grid(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([(xs.ravel() + 0.5) / w, (ys.ravel() + 0.5) / h], -1)


def slot_levels(c, slot, levels):
    """Asserts that texture `slot` holds exactly `levels` (every texel of every level through the level sampler)."""
    bpp = levels[0].shape[2]
    for l, lv in enumerate(levels):
        out = c.selftest_sampler_lod(slot, texel_grid(lv.shape[1], lv.shape[0]), float(l), api.SAMPLE_LEVEL)
        assert (out[:, 4] == bpp).all() and (out[:, bpp:4] == 0).all()
        assert np.array_equal(out[:, :bpp].reshape(lv.shape), lv), (slot, l)
    # no level behind the last: L is clamped
    last = levels[-1]
    top = c.selftest_sampler_lod(slot, [[0.5, 0.5]], float(len(levels) + 2), api.SAMPLE_LEVEL)[0]
    assert np.array_equal(top[:bpp], last[last.shape[0] // 2, last.shape[1] // 2])


def draw_flat(c, seed=3, n=40):
    clip, col = scenes.random_triangles(n, c.width, c.height, seed=seed, rmin=2, rmax=20, perspective_w=True)
    c.draw(FLAT, clip, colors=col)


@pytest.mark.parametrize("bpp", cases.BPPS)
def test_texture_chains_of_uploaded_captured_and_filtered_textures(bpp):
    W, H = 50, 38
    with Context(W, H, bpp, device=0) as c:
        img = cases.texture(67, 45, bpp, seed=3)
        c.upload_texture(0, img[..., 0] if bpp == 1 else img)
        slot_levels(c, 0, [img])                                               # one level until the call
        c.texture_mipmaps(0)
        slot_levels(c, 0, model.chain(img))
        c.clear((10, 20, 30, 255))
        draw_flat(c)
        fb = c.read_framebuffer()
        assert len(np.unique(fb.reshape(-1, bpp), axis=0)) > 5
        c.texture_from_framebuffer(1, 1)
        c.texture_mipmaps(1)
        slot_levels(c, 1, model.chain(fb))
        c.texture_from_image(2, to_device(img), 2, device=True)
        c.texture_mipmaps(2)
        slot_levels(c, 2, model.chain(box_model.box_filter(img, 2)))
        one = cases.texture(1, 1, bpp)
        c.upload_texture(3, one[..., 0] if bpp == 1 else one)
        c.texture_mipmaps(3)                                                   # L = 1: nothing to build
        slot_levels(c, 3, [one])
        slot_levels(c, 0, model.chain(img))                                    # the other slots kept theirs
        assert (c.selftest_sampler_lod(9, [[0.5, 0.5]], 1.5, api.SAMPLE_TRILINEAR)[0] == (255, 255, 255, 255, 4)).all()      # an empty slot


LEVELS_KIND = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double uv[2] = { 0.5, 0.5 };
    return trgl_sample2D_level(in, 0, uv, 99).bgra | 0xff000000u;
}
"""


def test_ordering_recapture_and_reuse():
    """A draw queued before trgl_texture_mipmaps samples one level, a draw after it the chain; a re-capture drops the chain; a second
    build on the reused slot equals the model; trgl_upload_texture on another slot leaves the chain intact."""
    W, H = 64, 48
    with Context(W, H, 3, device=0) as c:
        kind = c.register_shader(LEVELS_KIND, 0)
        c.clear((1, 2, 3, 255))
        draw_flat(c, seed=6)
        c.texture_from_framebuffer(0, 1)                                        # slot 0: this frame, one level
        first = c.read_framebuffer()
        chain = model.chain(first)
        left = np.array([[-1, -1, 0, 1, 0, -1, 0, 1, -1, 1, 0, 1]], np.float64)   # x in [-1, 0]: the left half, counter-clockwise on screen
        right = left.copy(); right[0, [0, 4, 8]] += 1.0
        c.clear((0, 0, 0, 255))
        c.draw(kind, left)                                                     # queued, not flushed
        c.texture_mipmaps(0)
        c.draw(kind, right)
        fb = c.read_framebuffer()
        centre0 = first[H // 2, W // 2]
        assert tuple(chain[-1].shape[:2]) == (1, 1) and not np.array_equal(chain[-1][0, 0], centre0)
        assert np.array_equal(fb[H // 2, 4], centre0) and np.array_equal(fb[H // 2, W // 2 + 8], chain[-1][0, 0])
        slot_levels(c, 0, chain)
        # a re-capture at the same size: one level again, the same memory
        c.clear((9, 9, 9, 255))
        draw_flat(c, seed=7)
        second = c.read_framebuffer()
        c.texture_from_framebuffer(0, 1)
        slot_levels(c, 0, [second])
        c.texture_mipmaps(0)
        slot_levels(c, 0, model.chain(second))
        # an upload into another slot rewrites the table from the host's mirror: the chain stays
        c.upload_texture(5, cases.texture(9, 5, 3))
        slot_levels(c, 0, model.chain(second))
        # an upload into the slot itself drops it
        img = cases.texture(W, H, 3, seed=4)
        c.upload_texture(0, img)
        slot_levels(c, 0, [img])
        c.texture_mipmaps(0)
        slot_levels(c, 0, model.chain(img))


# ---- the filtered samplers on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tex", cases.SAMPLE_TEXTURES, ids=lambda p: "%dx%dx%d" % p)
def test_device_samplers_equal_the_model(ctx, tex):
    w, h, bpp = tex
    img = cases.texture(w, h, bpp, seed=9)
    levels = model.chain(img)
    uv = cases.sample_uv(w, h, len(levels))
    ctx.upload_texture(4, img[..., 0] if bpp == 1 else img)
    ctx.texture_mipmaps(4)
    chain = api.image_mipmaps(img)
    for lod in cases.level_lods(len(levels)):
        for mode in (api.SAMPLE_LEVEL, api.SAMPLE_LINEAR):
            got = ctx.selftest_sampler_lod(4, uv, lod, mode)
            assert np.array_equal(got, api.image_sample(img, chain, uv, lod, mode)), (mode, lod)      # the host twin
            if mode == api.SAMPLE_LINEAR:
                assert np.array_equal(got, model.sample(levels, uv, lod, mode)), lod
    sub = uv[::3]
    for lod in cases.trilinear_lods(len(levels)):
        got = ctx.selftest_sampler_lod(4, sub, lod, api.SAMPLE_TRILINEAR)
        assert np.array_equal(got, model.sample(levels, sub, lod, 2)), lod
    # without a chain every function works on one level
    ctx.upload_texture(4, img[..., 0] if bpp == 1 else img)
    for mode, lod in ((0, 3.0), (1, 2.0), (2, 2.5)):
        assert np.array_equal(ctx.selftest_sampler_lod(4, sub, lod, mode), model.sample([img], sub, lod, mode))


# ---- trgl_lod_stage ------------------------------------------------------------------------------------------------------------------
def at_8_mod_16(a):
    """A device copy of the float64 array `a` whose first element lies at 8 mod 16."""
    import torch
    buf = torch.empty(a.size + 2, dtype=torch.float64, device="cuda")
    start = 1 if buf.data_ptr() % 16 == 0 else 0
    t = buf[start:start + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 8
    return t


@pytest.mark.parametrize("K_,uv_offset,out_offset", cases.LOD_LAYOUTS)
def test_device_lod_rows_equal_the_host_rows(K_, uv_offset, out_offset):
    vp = cases.viewport(48, 40)
    clip, uv = cases.all_lod_cases()
    vary = cases.lod_rows(K_, uv_offset, out_offset, clip, uv, seed=K_ + uv_offset)
    want = api.lod_stage(vp, clip, vary.copy(), uv_offset, out_offset)
    assert np.array_equal(want.view(np.uint64), model.lod_stage(vp, clip, vary, uv_offset, out_offset).view(np.uint64))
    with Context(48, 40, 3, device=0) as c:
        d_clip, d_vary = at_8_mod_16(clip), at_8_mod_16(vary)
        c.clear((3, 3, 3, 255))
        draw_flat(c, seed=1)                                                   # queued around the stage: it neither flushes nor waits
        c.lod_stage(vp, d_clip, d_vary, uv_offset, out_offset, device=True)
        draw_flat(c, seed=2)
        c.sync()
        assert np.array_equal(d_vary.cpu().numpy().view(np.uint64), want.view(np.uint64))
        L = api.load_library()
        p, q = d_clip.data_ptr(), d_vary.data_ptr()
        vpp = np.ascontiguousarray(vp).ctypes.data_as(api.C.POINTER(api.C.c_double))
        assert L.trgl_lod_stage(c.h, vpp, p + 4, q, 1, K_, uv_offset, out_offset, 1) == E_INVALID
        assert L.trgl_lod_stage(c.h, vpp, p, q + 4, 1, K_, uv_offset, out_offset, 1) == E_INVALID
        assert L.trgl_lod_stage(c.h, vpp, p, q, 1, K_, uv_offset, uv_offset + 2, 1) == E_INVALID
        c.sync()
        assert np.array_equal(d_vary.cpu().numpy().view(np.uint64), want.view(np.uint64))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
W2, H2 = 48, 40
BAR_PROBE = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    return (uint32_t)((unsigned long long)__double_as_longlong(in.bar[%d]) >> %d);
}
"""
TRILINEAR_KIND = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    double uv[2];
    uv[0] = (in.bar[0] * in.vary[0] + in.bar[1] * in.vary[2]) + in.bar[2] * in.vary[4];
    uv[1] = (in.bar[0] * in.vary[1] + in.bar[1] * in.vary[3]) + in.bar[2] * in.vary[5];
    int w = 1, h = 1;
    trgl_texture_levels(in, 0, &w, &h);
    return trgl_sample2D_trilinear(in, 0, uv, trgl_mip_lod(in.bar, in.vary + 20, w, h)).bgra;
}
"""


def perspective_quad():
    """A quad receding from z = 0 (w = 1) to z = -1.5 (w = 2): vertices [4, 14] (pos3, normal3, uv2, tangent3, bitangent3), faces, mv, proj."""
    f = 1.5
    proj = np.eye(4); proj[3, 2] = -1.0 / f
    verts = np.zeros((4, 14))
    verts[:, :3] = [(-0.9, -0.8, 0.0), (0.9, -0.8, 0.0), (1.7, 1.5, -1.5), (-1.7, 1.5, -1.5)]
    verts[:, 3:6] = (0, 0, 1)
    verts[:, 6:8] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.eye(4), proj


def test_one_frame_end_to_end_equals_the_model():
    import torch
    verts, faces, mv, proj = perspective_quad()
    vp = cases.viewport(W2, H2)
    tex = cases.texture(256, 256, 4, seed=12)
    levels = model.chain(tex)
    with Context(W2, H2, 4, device=0) as c:
        c.init_viewport(0, 0, W2, H2)
        c.upload_texture(0, tex)
        c.texture_mipmaps(0)
        clip = torch.empty((2, 12), dtype=torch.float64, device="cuda")
        vary = torch.empty((2, 24), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.vertex_stage(-1, make_uniforms(mv), proj, to_device(verts), to_device(faces), device=True, out=(clip, vary))
        c.lod_stage(vp, clip, vary, 0, 20, device=True)
        c.sync()
        h_clip, h_vary = clip.cpu().numpy(), vary.cpu().numpy()
        assert (h_clip[:, 3::4] >= 1.0).all() and h_clip[:, 3::4].max() == 2.0                     # perspective
        assert np.array_equal(h_vary.view(np.uint64), model.lod_stage(vp, h_clip, h_vary, 0, 20).view(np.uint64))
        assert (h_vary[:, 20] > 0).all()

        def frame(kind, **kw):
            c.clear((7, 7, 7, 7), np.inf)
            c.reset_stats()
            c.draw(kind, clip, vary if kind != FLAT else None, device=True, **kw)
            return c.read_framebuffer().copy(), c.read_zbuffer().view(np.uint64).copy(), c.stats()
        words = {}
        for i in range(3):
            for shift in (32, 0):
                fb, z, st = frame(c.register_shader(BAR_PROBE % (i, shift), 24))
                words[(i, shift)] = fb.reshape(H2, W2, 4).copy().view(np.uint32)[..., 0].astype(np.uint64)
        ids, z_ids, _ = frame(FLAT, colors=to_device(np.array([0xff000001, 0xff000002], np.uint32)))
        got, z_got, st_got = frame(c.register_shader(TRILINEAR_KIND, 24))
        assert np.array_equal(z_got, z) and st_got == st and np.array_equal(z_ids, z)
    covered = np.isfinite(z.view(np.float64)).reshape(H2, W2)
    assert covered.sum() > W2 * H2 // 3 and (~covered).any()
    tri = ids.reshape(H2, W2, 4)[..., 0].astype(int) - 1
    bar = np.stack([((words[(i, 32)] << np.uint64(32)) | words[(i, 0)]).view(np.float64) for i in range(3)], -1)
    want = np.full((H2, W2, 4), 7, np.uint8)
    lods = []
    for y, x in np.argwhere(covered):
        b, v = [model.F(t) for t in bar[y, x]], [model.F(t) for t in h_vary[tri[y, x]]]
        uv = ((b[0] * v[0] + b[1] * v[2]) + b[2] * v[4], (b[0] * v[1] + b[1] * v[3]) + b[2] * v[5])
        lod = model.mip_lod(b, v[20:24], 256, 256)
        lods.append(lod)
        want[y, x] = model.sample_trilinear(levels, uv, lod)[:4]
    assert min(lods) > 1.0 and max(lods) - min(lods) > 0.5                     # minified, and more so far away
    assert np.array_equal(got.reshape(H2, W2, 4), want)


# ---- the example ---------------------------------------------------------------------------------------------------------------------
DEMO_NEAREST = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    return trgl_sample2D(in, in.u->tex_diffuse, uv).bgra | 0xff000000u;
}
"""
DEMO_TRILINEAR = """
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (in.bar[0] * v[0] + in.bar[1] * v[2]) + in.bar[2] * v[4], (in.bar[0] * v[1] + in.bar[1] * v[3]) + in.bar[2] * v[5] };
    int w = 1, h = 1;
    trgl_texture_levels(in, in.u->tex_diffuse, &w, &h);
    return trgl_sample2D_trilinear(in, in.u->tex_diffuse, uv, trgl_mip_lod(in.bar, v + 20, w, h)).bgra | 0xff000000u;
}
"""


def demo_quad(corners):
    verts = np.zeros((4, 14))
    verts[:, :3] = corners
    verts[:, 4] = 1.0
    verts[:, 6:8] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    return verts


def test_demo_mipmap_equals_the_python_route(tmp_path):
    """examples/demo_mipmap.cpp in a child process: a checkerboard ground plane under perspective and a small screen that shows the
    captured frame, through trgl_vertex_stage, trgl_lod_stage and trgl_draw, once with a nearest user kind and once with a trilinear
    one.  Both frames against the same calls made from Python (the scene is restated here)."""
    assert os.path.exists(DEMO), "examples/demo_mipmap not built: run __graft_entry__.build()"
    names = [str(tmp_path / n) for n in ("nearest.tga", "trilinear.tga")]
    r = subprocess.run([DEMO] + names, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # (the TGA rows are stored bottom-up and decoded back on top: [::-1] is the framebuffer's row order again)
    files = [np.ascontiguousarray(api.tga_decode(open(n, "rb").read())[::-1]) for n in names]
    W, H, T = 160, 120, 256
    ys, xs = np.mgrid[0:T, 0:T]
    light = (((xs // 8) + (ys // 8)) & 1)[..., None] == 1
    board = np.where(light, np.array([230, 230, 230]), np.array([30, 40, 200])).astype(np.uint8)
    proj = np.eye(4); proj[3, 2] = -1.0 / 3.0
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    quads = [demo_quad([(-1.2, -0.9, 0.5), (1.2, -0.9, 0.5), (14.0, 0.6, -24.0), (-14.0, 0.6, -24.0)]),
             demo_quad([(0.30, 0.30, 0.0), (0.90, 0.30, 0.0), (0.90, 0.85, 0.0), (0.30, 0.85, 0.0)])]
    frames = []
    with Context(W, H, 3, device=0) as c:
        c.init_viewport(0, 0, W, H)
        c.upload_texture(0, board)
        c.texture_mipmaps(0)
        kinds = [c.register_shader(DEMO_NEAREST, 24), c.register_shader(DEMO_TRILINEAR, 24)]
        rows = []
        for q in quads:
            clip, vary = c.vertex_stage(-1, make_uniforms(np.eye(4)), proj, q, faces)
            rows.append((clip, api.lod_stage(cases.viewport(W, H), clip, np.ascontiguousarray(vary), 0, 20)))
        for kind in kinds:
            c.clear((40, 30, 20, 255), np.inf)
            c.draw(kind, rows[0][0], rows[0][1], uniforms=make_uniforms(np.eye(4), tex_diffuse=0))
            c.texture_from_framebuffer(1, 1)
            c.texture_mipmaps(1)
            c.draw(kind, rows[1][0], rows[1][1], uniforms=make_uniforms(np.eye(4), tex_diffuse=1))
            frames.append(c.read_framebuffer())
    nearest, trilinear = files
    assert nearest.shape == (H, W, 3) and np.array_equal(nearest, frames[0]) and np.array_equal(trilinear, frames[1])
    # near the horizon the nearest frame shows the board's two colours and nothing else; the trilinear frame shows their blends
    far = slice(H // 2 - 8, H // 2)
    colours = lambda f: len(np.unique(f[far, :W // 4].reshape(-1, 3), axis=0))
    assert colours(nearest) == 2 < colours(trilinear)
