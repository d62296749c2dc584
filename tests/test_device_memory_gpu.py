"""Draws from caller-owned device memory (TRGL_MEM_DEVICE, include/trgl.h:39-46): the path bench.py times.  The kernels read the
caller's pointers as they are, so every read below is checked from a caller's buffer, at every alignment the header allows.

  a. every built-in kind: GOURAUD's d->vary + local * 3 (resolve() in kernels_raster.hip), k_shade's d.vary + local * 24
     (kernels_raster.hip), k_setup's d.colors[i] (kernels_bin.hip), alone and in the mixed flush (k_raster<ANY>,
     k_shade<ANY>), whole, in three flushes, in an odd-row strip and in one rank's bands;
  b. user kinds: in.vary = d.vary + local * K (trgl_shade_user in shade_user.h; trgl_raster_user in raster_user.h for kinds that may
     discard), K = 24 and K = 5;
  c. alignment: k_setup's copy of a clip stream that is not 16-byte aligned (its staging loop in kernels_bin.hip: only a caller's device
     pointer reaches it, the host path stages into 256-byte aligned chunks, stage_alloc in trgl_api.cpp), whole and partial blocks,
     8-aligned varyings, 4-aligned colours, the literal records;
  d. host and device draws in one flush (trgl_draw in trgl_api.cpp), and more device draws than a flush has descriptors
     (its cut at TRGL_MAX_DRAWS) while Context._keep holds the tensors;
  e. arrays are read by the flush and not afterwards: buffers reused between frames as bench.py's loop reuses them, and
     overwritten once the flush has completed;
  f. stream ordering: the context's own stream is hipStreamNonBlocking (init_ctx in trgl_api.cpp) and waits for nobody; on a shared
     stream (trgl_set_stream) producers, flush and overwrites line up without a host sync, as bench.py and shard.StripLoop rely on;
  g. trgl_draw_indexed(TRGL_MEM_DEVICE): k_vertex_stage gathers through the caller's pointers (kernels_post.hip), whole
     meshes and the block edges of 64 faces (trgl_draw_indexed in trgl_stage_mesh.cpp does not stage or check on this path).

Bar: the device-memory frame equals the host-memory frame of the same GPU bit for bit - z bits, framebuffer bytes, stats tuple and
stats line, EYE included (the same kernels on the same numbers) - and the oracle's / the reference's golden within the suite's bar
(cases.assert_same_frame: exact, EYE colours within 1 LSB on at most 0.1 % of the pixels).
Every array given to a device draw is a live torch CUDA tensor; overwrites use NaN, zeros or another valid scene; indices stay in
range.  No test here relies on the binding's guard against host arrays (tests/test_device_pointer_guard.py covers it without a GPU).
"""
import json
import os

import numpy as np
import pytest

import cases
import discard_shader_sources as D
import user_shader_sources as S
from oracle import orc
from test_next_rows import _indexed_head
from test_raster_paths import LH, LW, MIXED, _kind_case, literal_scene, setup_literal
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, EYE, make_uniforms

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
NEXT_ROWS = json.load(open(os.path.join(HERE, "golden", "next_rows_golden.json")))

same = cases.assert_same_frame

# (source, K[, may_discard]) as cases.run_gpu(shaders=) and Context.register_shader take them
USER_PHONG = (S.PHONG, 24)
USER_GOURAUD5 = (S.GOURAUD_PADDED, 5)                                      # an odd K: rows of 40 bytes
DISCARDING_PHONG = (D.PHONG, 24, True)
DISCARDING_GOURAUD5 = (D.never_discarding(S.GOURAUD_PADDED), 5, True)


def _rank_rows(height, band, rank, world):
    """Rows of the bands that trgl_set_interleave(band, rank, world) gives its rank; the last band may be partial."""
    return [(y, min(y + band, height)) for y in range(rank * band, height, band * world)]


def _device_equals_host(case, dev, shaders=None, oracle_case=None, golden=None, what=""):
    """The device-memory twin `dev` of `case` gives the host-memory frame bit for bit: whole, in three flushes, in an odd-row
    strip and in rank 1 of two ranks' 32-row bands (the last three against the rows of the whole frame); the whole frame also
    equals the oracle's frame of oracle_case (default: case) and the reference's golden.  Returns the host frame."""
    h = case["height"]
    eye = cases.has_eye(oracle_case or case)
    host = cases.run_gpu(case, shaders=shaders)
    got = cases.run_gpu(dev, shaders=shaders)
    same(got, host, what=f"{what} device against host memory")
    same(got, cases.run_oracle(oracle_case or case), eye=eye, what=f"{what} device memory against the oracle")
    if golden is not None:
        cases.assert_golden(got, golden, eye=eye)
    same(cases.run_gpu(dev, shaders=shaders, split=3), host, what=f"{what} three flushes")
    strip = ((h // 3) | 1, (h - 5) | 1)
    same(cases.run_gpu(dev, shaders=shaders, strip=strip), host, rows=strip, stats=False, what=f"{what} strip {strip}")
    il = (32, 1, 2)
    same(cases.run_gpu(dev, shaders=shaders, interleave=il), host, rows=_rank_rows(h, *il), stats=False, what=f"{what} bands {il}")
    return host


# =====================================================================================================================
# a. every built-in kind from device memory
# =====================================================================================================================
KIND_CASES = ["gouraud_256_rgba", "phong_512", "eye_256", "multi_draw_320x200", "checker_mixed_200x120", "shade_uv_extremes_128x64",
              "shade_zero_normals_eye_96x64_rgba", "gray_bpp1_96x64", "huge_depths_128"]


@pytest.mark.parametrize("name", KIND_CASES)
def test_every_kind_from_device_memory(name):
    case = cases.CASES[name]()
    dev = cases.on_device(case)
    for d in dev["draws"]:
        assert all(t is None or t.is_cuda for t in d[2:])
    host = _device_equals_host(case, dev, golden=GOLDEN[name], what=name)
    assert host[2][1] > 500


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_mixed_flush_from_device_memory(bpp):
    """FLAT + GOURAUD + PHONG + CHECKER in one flush (k_raster<ANY>, k_shade<ANY>: every array through the draw descriptor),
    literal triangles among them."""
    clip, col, _, _ = literal_scene(3100 + bpp)
    case = _kind_case(MIXED, clip, col, LW, LH, bpp, seed=3200 + bpp, viewport=cases.UNIT_VIEWPORT)
    host = _device_equals_host(case, cases.on_device(case), what=f"mixed bpp {bpp}")
    assert host[0].shape[-1] == bpp and host[2][1] > 5000


# =====================================================================================================================
# b. user kinds
# =====================================================================================================================
def _padded(case):
    """The GOURAUD case with two leading varyings per triangle (K = 5, user_shader_sources.GOURAUD_PADDED)."""
    return dict(case, draws=[(k, u, clip, np.ascontiguousarray(np.concatenate([np.full((clip.shape[0], 2), 7.5), vary], 1)), col)
                             for k, u, clip, vary, col in case["draws"]])


@pytest.mark.parametrize("src", ["phong24", "gouraud5", "discarding_phong24", "discarding_gouraud5"])
def test_user_kinds_from_device_memory(src):
    """A user kind without and one with TRGL_SHADER_MAY_DISCARD, at K = 24 and at an odd K, each restating a built-in kind:
    device memory == host memory, and both == the built-in kind (whose frame the oracle and the golden pin)."""
    shader = {"phong24": USER_PHONG, "gouraud5": USER_GOURAUD5, "discarding_phong24": DISCARDING_PHONG,
              "discarding_gouraud5": DISCARDING_GOURAUD5}[src]
    name = "phong_512" if shader[1] == 24 else "gouraud_256_rgba"
    builtin = cases.CASES[name]()
    case = builtin if shader[1] == 24 else _padded(builtin)
    dev = cases.on_device(case)
    if shader[1] == 5:
        assert dev["draws"][0][3].shape[1] == 5 and dev["draws"][0][3][1:].data_ptr() % 16 == 8       # 40-byte rows
    host = _device_equals_host(case, dev, shaders=[shader], oracle_case=builtin, golden=GOLDEN[name], what=src)
    same(host, cases.run_gpu(builtin), what=f"{src} against the built-in kind")


# =====================================================================================================================
# c. alignment
# =====================================================================================================================
AW, AH = 128, 96


def _aligned_scene(kind, n, seed):
    """n + 3 triangles of `kind` (the tests draw n of them, from row 0, 1 or 3)."""
    m = n + 3
    clip, col = scenes.random_triangles(m, AW, AH, seed=seed, rmin=6, rmax=40, perspective_w=True)
    if kind == FLAT:
        return clip, None, col, None, {}
    if kind == GOURAUD:
        return clip, scenes.SplitMix64(seed + 1).uniform(m * 3, -0.2, 1.3).reshape(m, 3), col, None, {}
    hd = scenes.head_standin(1, AW, AH)
    d, nm, sp = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.7, 0, 1, 2)
    return clip, cases.phong_soup_varyings(m, seed + 1), None, u, {0: d, 1: nm, 2: sp}


def _rows(case_arrays, kind, u, tex, a, b):
    clip, vary, col = case_arrays
    return cases.make_case(AW, AH, [(kind, u, clip[a:b], None if vary is None else vary[a:b], None if col is None else col[a:b])],
                           bpp=4, textures=tex, clear=(9, 8, 7, 6))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("kind", [FLAT, GOURAUD, PHONG], ids=["flat", "gouraud", "phong"])
def test_naturally_aligned_device_pointers(kind, n):
    """clip 8 bytes, varyings 8 bytes and colours 4, 8 and 12 bytes past a 16-byte boundary, as offsets into a larger allocation
    and as slices t[k:] of one tensor with odd k: whole and partial setup blocks (block b starts b * 256 * 96 bytes on, so every
    block of such a draw takes the scalar copy).  Result == host memory == oracle."""
    clip, vary, col, u, tex = _aligned_scene(kind, n, seed=500 + n)
    runs = 0
    # placed into a larger allocation
    for col_off in ((4, 8, 12) if col is not None else (0,)):
        case = _rows((clip, vary, col), kind, u, tex, 0, n)
        dev = cases.on_device(case, clip_off=8, vary_off=8, col_off=col_off)
        _, _, dclip, dvary, dcol = dev["draws"][0]
        assert dclip.data_ptr() % 16 == 8 and dclip.shape == (n, 12)
        assert dvary is None or dvary.data_ptr() % 16 == 8
        assert dcol is None or dcol.data_ptr() % 16 == col_off
        host = cases.run_gpu(case)
        got = cases.run_gpu(dev)
        same(got, host, what=f"offsets 8 / 8 / {col_off}: device against host memory")
        same(got, cases.run_oracle(case), what=f"offsets 8 / 8 / {col_off}: device memory against the oracle")
        assert host[2][0] >= 1 and host[2][1] > 0
        runs += 1
    # slices of one tensor: clip rows are 96 bytes (a slice keeps the base's residue, so the base sits 8 bytes in), GOURAUD rows
    # 24 bytes and colour rows 4 bytes (an odd k moves them off the 16-byte boundary), PHONG rows 192 bytes
    whole = cases.on_device(_rows((clip, vary, col), kind, u, tex, 0, n + 3), clip_off=8, vary_off=8 if kind == PHONG else 0)
    _, _, wclip, wvary, wcol = whole["draws"][0]
    for k in (1, 3):
        case = _rows((clip, vary, col), kind, u, tex, k, k + n)
        dclip, dvary, dcol = wclip[k:k + n], None if wvary is None else wvary[k:k + n], None if wcol is None else wcol[k:k + n]
        assert dclip.data_ptr() % 16 == 8 and dclip.shape == (n, 12)
        assert dvary is None or dvary.data_ptr() % 16 == 8
        assert dcol is None or dcol.data_ptr() % 16 == 4 * k
        got = cases.run_gpu(dict(case, draws=[(kind, u, dclip, dvary, dcol)]))
        same(got, cases.run_gpu(case), what=f"slice [{k}:]: device against host memory")
        same(got, cases.run_oracle(case), what=f"slice [{k}:]: device memory against the oracle")
        runs += 1
    assert runs == (5 if col is not None else 3)


def test_literal_records_from_an_8_aligned_clip_pointer():
    """A dense 160x128 scene whose every fifth triangle takes the literal path, its clip stream through the scalar copy."""
    clip, col, _, _ = literal_scene(3100)
    assert setup_literal(clip, cases.UNIT_VIEWPORT, LW, LH)[0].sum() >= 150
    case = cases.make_case(LW, LH, [(FLAT, None, clip, None, col)], viewport=cases.UNIT_VIEWPORT)
    dev = cases.on_device(case, clip_off=8, col_off=4)
    assert dev["draws"][0][2].data_ptr() % 16 == 8 and dev["draws"][0][4].data_ptr() % 16 == 4
    got = cases.run_gpu(dev)
    same(got, cases.run_gpu(case), what="literal scene: device against host memory")
    same(got, cases.run_oracle(case), what="literal scene: device memory against the oracle")
    assert got[2][1] > 5000


# =====================================================================================================================
# d. one flush, both memories; descriptor limit
# =====================================================================================================================
def test_host_and_device_draws_share_a_flush():
    """FLAT, GOURAUD and PHONG draws, alternately from host and from device memory, in one flush; then the other way round."""
    w, h = 240, 160
    hd = scenes.head_standin(3, w, h)
    d, n, sp = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
    fc, fcol = scenes.random_triangles(1200, w, h, seed=91, rmin=2, rmax=40, perspective_w=True)
    gc, gcol = scenes.random_triangles(1500, w, h, seed=92, rmin=2, rmax=40, perspective_w=True)
    gi = scenes.SplitMix64(93).uniform(1500 * 3, -0.2, 1.3).reshape(1500, 3)
    half = hd["clip"].shape[0] // 2
    case = cases.make_case(w, h, [(FLAT, None, fc[:600], None, fcol[:600]), (GOURAUD, None, gc[:700], gi[:700], gcol[:700]),
                                  (PHONG, u, hd["clip"][:half], hd["varyings"][:half], None), (FLAT, None, fc[600:], None, fcol[600:]),
                                  (GOURAUD, None, gc[700:], gi[700:], gcol[700:]), (PHONG, u, hd["clip"][half:], hd["varyings"][half:], None)],
                           bpp=4, textures={0: d, 1: n, 2: sp}, clear=(3, 2, 1, 255))
    dev = cases.on_device(case, clip_off=8, vary_off=8, col_off=4)
    want = cases.run_oracle(case)
    for first in (0, 1):
        mixed = dict(case, draws=[dv if i % 2 == first else hv for i, (hv, dv) in enumerate(zip(case["draws"], dev["draws"]))])
        assert sum(not isinstance(dr[2], np.ndarray) for dr in mixed["draws"]) == 3
        same(cases.run_gpu(mixed), want, what=f"device draws at {first}, {first + 2}, {first + 4}")
        same(cases.run_gpu(mixed, halves=True), want, what=f"device draws at {first}, {first + 2}, {first + 4}, flush in halves")


def test_more_device_draws_than_descriptors_between_flushes():
    """70 small trgl_draw calls from device memory without a flush in between: the 65th finds the 64 draw descriptors of a flush
    taken and flushes on its own.  The test keeps no reference to the tensors: Context._keep holds all 70 of them until the
    frame has been read (asserted before the last flush runs)."""
    W, H = 200, 120
    clip, col = scenes.random_triangles(70 * 37, W, H, seed=81, rmin=2, rmax=30, perspective_w=True)
    inten = scenes.SplitMix64(82).uniform(70 * 37 * 3, 0.1, 1.2).reshape(-1, 3)
    import torch
    with Context(W, H, 3) as ctx:
        for i in range(70):
            r = slice(37 * i, 37 * (i + 1))
            arrays = (cases.device_array(clip[r], 8 * (i & 1)), cases.device_array(inten[r], 8 * (i & 1)), cases.device_array(col[r], 4 * (i % 4)))
            torch.cuda.synchronize()                    # the uploads run on torch's stream
            ctx.draw(GOURAUD, *arrays, device=True)
            del arrays
        assert len(ctx._keep) == 70 and all(t.is_cuda for kept in ctx._keep for t in kept)
        got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
    same(got, cases.run_oracle(cases.make_case(W, H, [(GOURAUD, None, clip, inten, col)])))
    assert got[2][0] == 70 * 37


# =====================================================================================================================
# e. read at flush, not later; buffer reuse
# =====================================================================================================================
def test_device_buffers_reused_between_frames():
    """bench.py's loop: one set of device buffers, drawn every frame and, once the frame has completed (sync), overwritten in
    place with the next frame's triangles.  Frame k equals the oracle's frame of content k."""
    import torch
    W, H, n = 256, 192, 6000
    frames = []
    for k in range(3):
        clip, col = scenes.random_triangles(n, W, H, seed=700 + k, rmin=2, rmax=40, perspective_w=bool(k & 1))
        frames.append((clip, scenes.SplitMix64(710 + k).uniform(n * 3, -0.2, 1.3).reshape(n, 3), col))
    bufs = [cases.device_array(a, off) for a, off in zip(frames[0], (8, 8, 4))]
    ptrs = [b.data_ptr() for b in bufs]
    with Context(W, H, 4) as ctx:
        for k, content in enumerate(frames):
            if k:
                for b, a in zip(bufs, content):
                    b.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a))
            torch.cuda.synchronize()                    # the context's own stream does not wait for torch's
            assert [b.data_ptr() for b in bufs] == ptrs
            ctx.clear((k, 2, 3, 255))
            ctx.reset_stats()
            ctx.draw(GOURAUD, *bufs, device=True)
            ctx.flush()
            ctx.sync()                                  # ... nor torch's for the context's: the overwrite comes after this
            got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
            same(got, cases.run_oracle(cases.make_case(W, H, [(GOURAUD, None) + content], bpp=4, clear=(k, 2, 3, 255))), what=f"frame {k}")


def test_arrays_are_not_read_after_the_flush_has_completed():
    """GOURAUD + PHONG + a user kind from device memory: flush, sync, then every array is overwritten with NaN (colours with
    zeros).  What comes after - reading the buffers and the counters, an empty flush, the post-process - gives the oracle's
    frame: nothing goes back to the caller's arrays."""
    import torch
    w, h = 240, 160
    hd = scenes.head_standin(3, w, h)
    small = scenes.head_standin(2, w, h, seed=5, distance=3.0)
    d, n, sp = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
    gc, gcol = scenes.random_triangles(1500, w, h, seed=95, rmin=2, rmax=40, perspective_w=True)
    gi = scenes.SplitMix64(96).uniform(1500 * 3, -0.2, 1.3).reshape(1500, 3)
    case = cases.make_case(w, h, [(GOURAUD, None, gc, gi, gcol), (PHONG, u, hd["clip"], hd["varyings"], None),
                                  (PHONG, u, small["clip"], small["varyings"], None)], textures={0: d, 1: n, 2: sp})
    want = cases.run_oracle(case)
    dev = cases.on_device(case, clip_off=8, vary_off=8, col_off=4)
    with Context(w, h, 3) as ctx:
        user = ctx.register_shader(*USER_PHONG)
        for slot, t in case["textures"].items():
            ctx.upload_texture(slot, t)
        for i, (kind, uu, clip, vary, col) in enumerate(dev["draws"]):
            ctx.draw(user if i == 2 else kind, clip, vary, col, uu, device=True)
        ctx.flush()
        ctx.sync()
        for _, _, clip, vary, col in dev["draws"]:
            clip.fill_(float("nan"))
            vary.fill_(float("nan"))
            if col is not None:
                col.zero_()
        torch.cuda.synchronize()
        assert bool(torch.isnan(dev["draws"][1][3]).all())
        got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
        same(got, want, what="after the overwrite")
        ctx.flush()                                     # nothing is queued: the draws of the completed flush are gone
        post = ctx.postprocess()
        again = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
    same(again, want, what="after an empty flush and the post-process")
    ao = orc.ssao(want[1])
    assert np.array_equal(post["zbuffer_image"], orc.zbuffer_image(want[1]))
    assert np.array_equal(post["ao"], ao)
    assert np.array_equal(post["final"], orc.composite(want[0], ao))


# =====================================================================================================================
# f. stream ordering
# =====================================================================================================================
@pytest.mark.parametrize("stream", ["torch", "own"])
def test_producers_flush_and_overwrites_are_ordered(stream):
    """The arrays are produced by torch kernels (a gather that undoes a row shuffle: a flush that ran ahead of it would draw
    other triangles, not merely old ones) and overwritten with NaN right after the flush.
    torch: the context runs on torch's current stream (set_stream) and nothing synchronises with the host in between;
    own: the context keeps its own stream, which waits for nobody: torch.cuda.synchronize() before the draw and ctx.sync()
    before the overwrite, as include/trgl.h asks."""
    import torch
    W = H = 1024
    fclip, fcol = scenes.random_triangles(200_000, W, H, seed=801, rmin=1, rmax=12)
    gclip, gcol = scenes.random_triangles(50_000, W, H, seed=802, rmin=2, rmax=24, perspective_w=True)
    ginten = scenes.SplitMix64(803).uniform(50_000 * 3, -0.2, 1.3).reshape(-1, 3)
    want = cases.run_oracle(cases.make_case(W, H, [(FLAT, None, fclip, None, fcol), (GOURAUD, None, gclip, ginten, gcol)]))

    def shuffled(arrays, seed):
        """Row-shuffled uploads of the arrays and the device index that undoes the shuffle."""
        n = arrays[0].shape[0]
        perm = np.argsort(scenes.SplitMix64(seed).u64(n), kind="stable")
        inv = np.empty_like(perm); inv[perm] = np.arange(n)
        return [cases.device_array(a[perm]) for a in arrays], torch.from_numpy(inv).cuda()

    uploads = [shuffled((fclip, fcol), 811), shuffled((gclip, ginten, gcol), 812)]
    torch.cuda.synchronize()
    with Context(W, H, 3) as ctx:
        if stream == "torch":
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for kind, (ups, inv) in zip((FLAT, GOURAUD), uploads):
            made = [t.index_select(0, inv) for t in ups]                    # torch kernels on torch's stream
            if stream == "own":
                torch.cuda.synchronize()
            if kind == FLAT:
                ctx.draw(FLAT, made[0], colors=made[1], device=True)
            else:
                ctx.draw(GOURAUD, *made, device=True)
            ctx.flush()
            if stream == "own":
                ctx.sync()
            for t in made:
                if t.dtype == torch.float64:
                    t.fill_(float("nan"))
                else:
                    t.zero_()
        got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
        if stream == "torch":
            ctx.set_stream(None, use_own=True)
    same(got, want, what=f"{stream} stream")
    assert got[2][0] == 250_000


# =====================================================================================================================
# g. draw_indexed from device memory
# =====================================================================================================================
def _mesh(name):
    """(vertices, indices, uniforms, projection, w, h, textures) of the fixture mesh (stride 8) or of the indexed head stand-in
    in the reference's Vertex layout (stride 14), both behind shuffled index buffers."""
    if name == "fixture":
        return cases.fixture_mesh() + (cases.edge_textures(),)
    w, h = 320, 200
    hd, verts, idx = _indexed_head(3, w, h)
    d, n, s = scenes.procedural_textures(64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.8, 0, 1, 2)
    return verts, idx, u, hd["projection"], w, h, {0: d, 1: n, 2: s}


def _draw_indexed(kind, shader, u, proj, verts, idx, w, h, textures, offsets=None):
    """One draw_indexed frame; offsets = (vertex bytes, index bytes): from device tensors placed that far into larger allocations."""
    import torch
    with Context(w, h, 3) as ctx:
        k = ctx.register_shader(*shader) if shader else kind
        for slot, t in textures.items():
            ctx.upload_texture(slot, t)
        if offsets is None:
            ctx.draw_indexed(k, u, proj, verts, idx)
        else:
            dv, di = cases.device_array(verts, offsets[0]), cases.device_array(idx, offsets[1])
            assert dv.data_ptr() % 16 == offsets[0] % 16 and di.data_ptr() % 16 == offsets[1] % 16 and di.shape == idx.shape
            torch.cuda.synchronize()
            ctx.draw_indexed(k, u, proj, dv, di, device=True)
        return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


@pytest.mark.parametrize("kind_name", ["phong", "eye", "user24"])
@pytest.mark.parametrize("mesh", ["fixture", "head14"])
def test_draw_indexed_from_device_memory(mesh, kind_name):
    """Whole meshes and prefixes of 1, 63, 64 and 65 faces (k_vertex_stage's blocks are 64 faces), vertices and indices at the
    start of their allocations and 8 / 4 bytes in: == draw_indexed from host memory bit for bit, == the oracle on
    orc.vertex_stage's arrays, and for the whole fixture mesh == the reference's frame."""
    verts, idx, u, proj, w, h, textures = _mesh(mesh)
    kind = EYE if kind_name == "eye" else PHONG
    shader = USER_PHONG if kind_name == "user24" else None
    assert int(idx.max()) < verts.shape[0] and verts.shape[1] == (8 if mesh == "fixture" else 14)
    mv = np.array(list(u.model_view)).reshape(4, 4)
    for nf in (idx.shape[0], 1, 63, 64, 65):
        part = np.ascontiguousarray(idx[:nf])
        host = _draw_indexed(kind, shader, u, proj, verts, part, w, h, textures)
        clip, vary = orc.vertex_stage(mv, proj, verts, part)
        want = cases.run_oracle(cases.make_case(w, h, [(kind, u, clip, vary, None)], textures=textures))
        assert want[2][0] >= 1
        for offsets in ((0, 0), (8, 4)):
            got = _draw_indexed(kind, shader, u, proj, verts, part, w, h, textures, offsets=offsets)
            same(got, host, what=f"{nf} faces, offsets {offsets}: device against host memory")
            same(got, want, eye=kind == EYE, what=f"{nf} faces, offsets {offsets}: device memory against the oracle")
            if mesh == "fixture" and nf == idx.shape[0]:
                cases.assert_golden(got, NEXT_ROWS["mesh"]["eye" if kind == EYE else "phong"], eye=kind == EYE)
