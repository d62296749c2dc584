"""The clip stage on the device (kernels_clip.hip) against the numpy model of its specification (tests/clip_model.py), bit for bit, and
the clipped draws - from host arrays, from device arrays, behind the built-in vertex stage and behind a user vertex shader - against the
oracle drawing the model-clipped lists."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import clip_model as cm
import vertex_shader_sources as V
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, CHECKER, make_uniforms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_clip")
PLANE = (1.0, 0.5, 0.0, 0.1)          # cuts the middle of the frame: x + 0.5 y + 0.1 w >= 0 in clip space
FRAMES = ((96, 64, 3), (101, 67, 4))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _device(a, off=0):
    import torch
    if a is None:
        return None
    if a.shape[0] == 0:
        return torch.empty(a.shape, dtype=torch.int32 if a.dtype == np.uint32 else torch.float64, device="cuda")
    return cases.device_array(a, off)


@pytest.mark.parametrize("n,K,colors", [(0, 3, True), (1, 24, True), (63, 0, False), (64, 7, True), (65, 24, False), (255, 24, True),
                                         (256, 3, True), (257, 7, False), (70000, 24, True)])
def test_device_stage_equals_the_model(n, K, colors):
    """k_clip_count / k_clip_scatter take CLIP_BLOCK_TRIS = 256 triangles per block (n = 255, 256, 257 sit around it; 63, 64, 65 around
    a wave), and a block of the scan's lower level takes CLIP_SCAN_CHUNK = 256 block sums: n = 70000 is 274 blocks in 2 chunks, so the
    offsets of the last 18 blocks need the scan's upper level (k_clip_scan_top)."""
    import torch
    clip, vary, col = cm.soup(n, K, seed=2000 + n, colors=colors)
    attrs = cm.SOUP_LAYOUTS[K]
    want = cm.clip_model(cm.NEAR, clip, vary, col, attrs)
    with Context(8, 8) as ctx:
        d = (_device(clip), _device(vary), _device(col))
        torch.cuda.synchronize()
        oclip, ovary, ocol, m = ctx.clip_stage(cm.NEAR, *d, attrs=attrs, device=True)
        ctx.sync()
        assert m == len(want[0])
        assert cm.same_bits(oclip[:m].cpu().numpy(), want[0]), "clip differs from the model"
        if K:
            assert cm.same_bits(ovary[:m].cpu().numpy(), want[1]), "varyings differ from the model"
        if colors:
            assert cm.same_bits(_u32(ocol[:m]), want[2]), "colours differ from the model"
    if n:
        assert 0 < m != n                   # (the seeds are chosen so: the single triangle of n = 1 is split)


def test_odd_offsets_and_untouched_surroundings():
    """Inputs 8 (doubles) and 4 (colours) bytes into their allocations; outputs likewise, inside buffers of a sentinel: the first n_out
    triangles equal the model, every other word of the output buffers - ahead of them, and behind n_out up to the 2 n the call may use
    and beyond - still holds the sentinel."""
    import torch
    n, K = 1000, 24
    clip, vary, col = cm.soup(n, K, seed=4242)
    attrs = cm.SOUP_LAYOUTS[K]
    want = cm.clip_model(cm.NEAR, clip, vary, col, attrs)
    m_want = len(want[0])
    SENT_D, SENT_C = -12345.6789, 0x5EA7BEEF
    bufs = (torch.full((1 + 2 * n * 12 + 3,), SENT_D, dtype=torch.float64, device="cuda"),
            torch.full((1 + 2 * n * K + 3,), SENT_D, dtype=torch.float64, device="cuda"),
            torch.full((1 + 2 * n + 3,), SENT_C, dtype=torch.int32, device="cuda"))
    outs = (bufs[0][1:1 + 2 * n * 12].view(2 * n, 12), bufs[1][1:1 + 2 * n * K].view(2 * n, K), bufs[2][1:1 + 2 * n])
    assert all(o.data_ptr() % 16 == b.element_size() for o, b in zip(outs, bufs))
    with Context(8, 8) as ctx:
        d = (cases.device_array(clip, 8), cases.device_array(vary, 8), cases.device_array(col, 4))
        assert d[0].data_ptr() % 16 == 8 and d[1].data_ptr() % 16 == 8 and d[2].data_ptr() % 8 == 4
        torch.cuda.synchronize()
        _, _, _, m = ctx.clip_stage(cm.NEAR, *d, attrs=attrs, device=True, out=outs)
        ctx.sync()
    assert m == m_want and m < 2 * n
    flat = [b.cpu().numpy() for b in bufs]
    for f, width, w, name in zip(flat, (12, K, 1), want, ("clip", "varyings", "colours")):
        body = f[1:1 + m * width]
        assert cm.same_bits(body.view(np.uint32) if name == "colours" else body, w.reshape(-1)), f"{name} differ from the model"
        rest = np.concatenate([f[:1], f[1 + m * width:]])
        assert (rest == (SENT_C if name == "colours" else SENT_D)).all(), f"{name}: written outside the first n_out triangles"


# ---- clipped draws -------------------------------------------------------------------------------------------------------------------
def _result(ctx):
    return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def _oracle(W, H, bpp, draws, textures=None):
    from oracle import orc
    fb, z, st = cases.run_oracle(cases.make_case(W, H, draws, bpp=bpp, textures=textures))
    return fb, z, st, orc.format_stats_line(st).strip()


def _scene(W, H):
    """Six draws that overlap in the frame: (kind, uniforms, clip, vary, colors, clipped?).  FLAT, GOURAUD, PHONG and the discarding
    CHECKER clipped, between unclipped FLAT and GOURAUD draws."""
    hd, tex = cases._head(2, W, H, 32)
    up = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
    tri = lambda n, seed, **kw: scenes.random_triangles(n, W, H, seed=seed, rmin=3, rmax=max(W, H) // 3, **kw)
    c0, k0 = tri(40, 501)
    c1, k1 = tri(120, 502, perspective_w=True)
    c2, k2 = tri(90, 503, perspective_w=True)
    v2 = scenes.SplitMix64(504).uniform(90 * 3, 0.1, 1.2).reshape(90, 3)
    c3, k3 = tri(70, 505, perspective_w=True)
    c5, k5 = tri(30, 506, perspective_w=True)
    v5 = scenes.SplitMix64(507).uniform(30 * 3, 0.1, 1.2).reshape(30, 3)
    draws = [(FLAT, None, c0, None, k0, False), (FLAT, None, c1, None, k1, True), (GOURAUD, None, c2, v2, k2, True),
             (CHECKER, make_uniforms(cells=3), c3, None, k3, True), (PHONG, up, hd["clip"], hd["varyings"], None, True),
             (GOURAUD, None, c5, v5, k5, False)]
    return draws, tex


def _expected_draws(draws, plane):
    out = []
    for kind, u, clip, vary, col, clipped in draws:
        if clipped:
            clip, vary, col = cm.clip_model(plane, clip, vary, col, cm.LAYOUTS[kind])
        out.append((kind, u, clip, vary, col))
    return out


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("W,H,bpp", FRAMES)
def test_clipped_draws_equal_the_oracle_on_the_model_clipped_lists(W, H, bpp, device):
    """draw(..., clip_plane=) of FLAT, GOURAUD, PHONG and CHECKER lists with their built-in layouts, interleaved with unclipped draws in
    one flush: frame, depths, counters and stats line are the oracle's on the lists the model clips."""
    import torch
    draws, tex = _scene(W, H)
    expected = _expected_draws(draws, PLANE)
    assert all(len(e[2]) != len(d[2]) for d, e in zip(draws, expected) if d[5]), "the plane must cut every clipped draw"
    with Context(W, H, bpp) as ctx:
        for slot, t in tex.items():
            ctx.upload_texture(slot, t)
        for kind, u, clip, vary, col, clipped in draws:
            arrays = (clip, vary, col)
            if device:
                arrays = tuple(None if a is None else _device(a, 8 if a.dtype == np.float64 else 4) for a in arrays)
                torch.cuda.synchronize()
            ctx.draw(kind, arrays[0], arrays[1], arrays[2], u, device=device, clip_plane=PLANE if clipped else None)
        got = _result(ctx)
    cases.assert_same_frame(got, _oracle(W, H, bpp, expected, tex), what="clipped draws")
    assert got[2][0] == sum(len(e[2]) for e in expected) != sum(len(d[2]) for d in draws)


def _mesh(W, H):
    """The head stand-in as an indexed mesh [nv, 8] (position, normal, uv) with shared vertices, its uniforms and projection."""
    hd = scenes.head_standin(2, W, H)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    verts = np.concatenate([pos, nrm, uv], 1).astype(np.float32).astype(np.float64)
    uniq, inv = np.unique(verts, axis=0, return_inverse=True)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.8, 0, 1, 2)
    return np.ascontiguousarray(uniq), np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32)), u, hd["projection"]


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("W,H,bpp", FRAMES)
def test_clipped_indexed_draws_equal_the_oracle(W, H, bpp, device):
    """draw_indexed(..., clip_plane=) behind the built-in vertex stage (PHONG) and behind a user vertex shader (a Gouraud intensity per
    vertex, K = 3, with per-face colours), between unclipped FLAT draws: the oracle on the model-clipped output of vertex_stage()."""
    import torch
    verts, idx, u, proj = _mesh(W, H)
    nf = idx.shape[0]
    _, tex = cases._head(2, W, H, 32)
    col = scenes.SplitMix64(610).u64(nf).astype(np.uint32) | np.uint32(0xff000000)
    c0, k0 = scenes.random_triangles(40, W, H, seed=611, rmin=3, rmax=W // 3)
    c1, k1 = scenes.random_triangles(40, W, H, seed=612, rmin=3, rmax=W // 3, perspective_w=True)
    plane2 = (-0.4, 1.0, 0.0, 0.05)
    with Context(W, H, bpp) as ctx:
        for slot, t in tex.items():
            ctx.upload_texture(slot, t)
        vs = ctx.register_vertex_shader(V.GOURAUD, 3)
        pclip, pvary = ctx.vertex_stage(-1, u, proj, verts, idx)
        gclip, gvary = ctx.vertex_stage(vs, u, proj, verts, idx)
        mesh = (verts, idx, col)
        if device:
            mesh = (cases.device_array(verts, 8), cases.device_array(idx, 4), cases.device_array(col, 4))
            torch.cuda.synchronize()
        ctx.draw(FLAT, c0, colors=k0)
        ctx.draw_indexed(PHONG, u, proj, mesh[0], mesh[1], device=device, clip_plane=PLANE)
        ctx.draw(FLAT, c1, colors=k1)
        ctx.draw_indexed(GOURAUD, u, proj, mesh[0], mesh[1], device=device, vertex_shader=vs, colors=mesh[2], clip_plane=plane2)
        got = _result(ctx)
    e1 = cm.clip_model(PLANE, pclip, pvary, None, cm.LAYOUTS[PHONG])
    e2 = cm.clip_model(plane2, gclip, gvary, col, cm.LAYOUTS[GOURAUD])
    assert 0 < len(e1[0]) != nf and 0 < len(e2[0]) != nf
    expected = [(FLAT, None, c0, None, k0), (PHONG, u, e1[0], e1[1], None), (FLAT, None, c1, None, k1), (GOURAUD, u, e2[0], e2[1], e2[2])]
    cases.assert_same_frame(got, _oracle(W, H, bpp, expected, tex), what="clipped indexed draws")


@pytest.mark.parametrize("device", (False, True))
def test_keep_all_plane_gives_the_plain_frame_and_drop_all_leaves_everything_alone(device):
    import torch
    W, H, bpp = FRAMES[1]
    draws, tex = _scene(W, H)
    keep_all, drop_all = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, -1.0)        # every w of the scene is > 0
    assert all((d[2][:, 3::4] > 0).all() for d in draws)

    def frame(plane, then_drop=False):
        with Context(W, H, bpp) as ctx:
            for slot, t in tex.items():
                ctx.upload_texture(slot, t)
            for kind, u, clip, vary, col, _ in draws:
                ctx.draw(kind, clip, vary, col, u, clip_plane=plane)
            if not then_drop:
                return _result(ctx)
            before = _result(ctx)
            for kind, u, clip, vary, col, _ in draws:
                arrays = tuple(None if a is None else _device(a) for a in (clip, vary, col)) if device else (clip, vary, col)
                if device:
                    torch.cuda.synchronize()
                ctx.draw(kind, *arrays, u, device=device, clip_plane=drop_all)
            return before, _result(ctx)

    plain = frame(None)
    cases.assert_same_frame(frame(keep_all), plain, what="keep-all plane against the plain draws")
    before, after = frame(None, then_drop=True)
    cases.assert_same_frame(before, plain, what="plain draws")
    cases.assert_same_frame(after, before, what="after draws that a drop-all plane empties")


def test_a_user_kind_with_varyings_needs_its_layout():
    import user_shader_sources as F
    clip, col = scenes.random_triangles(50, 96, 64, seed=700, rmin=3, rmax=30, perspective_w=True)
    inten = scenes.SplitMix64(701).uniform(50 * 3, 0.1, 1.2).reshape(50, 3)
    with Context(96, 64, 3) as ctx:
        kind = ctx.register_shader(F.GOURAUD, 3)
        with pytest.raises(api.TrglError):
            ctx.draw(kind, clip, inten, col, clip_plane=PLANE)
        ctx.draw(kind, clip, inten, col, clip_plane=PLANE, clip_attrs=[(0, 1)])
        got = _result(ctx)
    e = cm.clip_model(PLANE, clip, inten, col, [(0, 1)])
    cases.assert_same_frame(got, _oracle(96, 64, 3, [(GOURAUD, None, e[0], e[1], e[2])]), what="user kind with its layout")


def test_demo_clip_frames_equal_the_model(tmp_path):
    """examples/demo_clip.cpp through the shim: its reference frame is the oracle's on the room as it is, its clipped frame the oracle's on
    the model-clipped room, which has no background pixel left."""
    assert os.path.exists(DEMO), "examples/demo_clip not built: run __graft_entry__.build()"
    W, H = 160, 120
    prefix = str(tmp_path / "clip")
    r = subprocess.run([DEMO, prefix, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(prefix + "_scene.bin", "rb").read()
    assert raw[:8] == b"TRCLSC01"
    w, h, ntri, _ = struct.unpack_from("<4i", raw, 8)
    assert (w, h) == (W, H)
    vp = np.frombuffer(raw, np.float64, 16, 24).reshape(4, 4)
    plane = np.frombuffer(raw, np.float64, 4, 24 + 128)
    clip = np.frombuffer(raw, np.float64, ntri * 12, 24 + 160).reshape(ntri, 12)
    col = np.frombuffer(raw, np.uint32, ntri, 24 + 160 + ntri * 96)
    assert 24 + 160 + ntri * 100 == len(raw) and tuple(plane) == cm.NEAR
    sc = cm.room_scene(W, H)
    assert np.allclose(clip, sc["clip"], rtol=1e-12, atol=1e-12) and np.array_equal(col, sc["colors"])
    ref = cases.run_oracle(cases.make_case(W, H, [(FLAT, None, clip, None, col)], viewport=vp))
    e = cm.clip_model(plane, clip, None, col)
    clipped = cases.run_oracle(cases.make_case(W, H, [(FLAT, None, e[0], None, e[2])], viewport=vp))
    assert open(prefix + "_reference.tga", "rb").read() == api.tga_encode(ref[0])
    assert open(prefix + "_clipped.tga", "rb").read() == api.tga_encode(clipped[0])
    background = lambda fb: int((fb.reshape(-1, 3) == 0).all(axis=1).sum())
    assert background(ref[0]) > 0 and background(clipped[0]) == 0
