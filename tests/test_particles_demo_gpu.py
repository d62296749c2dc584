"""examples/demo_particles.cpp - an opaque box, 4096 blended particles expanded, sorted and drawn without leaving device memory, and the
box's wireframe as wide lines - against the same scene restated here and drawn through the Python binding from host arrays."""
import os
import subprocess

import numpy as np
import pytest

import order_model as O
import sprite_model as M
import triangle_order_model as T
from tinyrenderder_amd import api
from tinyrenderder_amd.api import Context, FLAT, make_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_particles")
MV = np.array([0.8, 0, 0.6, 0, 0.36, 0.8, -0.48, 0, -0.48, 0.6, 0.64, -5, 0, 0, 0, 1], np.float64)
PROJ = np.array([1.25, 0, 0, 0, 0, 2, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64)
PARTICLE_SRC = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) {
    const double* v = in.vary;
    double uv[2] = { (v[0] * in.bar[0] + v[2] * in.bar[1]) + v[4] * in.bar[2], (v[1] * in.bar[0] + v[3] * in.bar[1]) + v[5] * in.bar[2] };
    const uint32_t texel = trgl_sample2D(in, in.u->tex_diffuse, uv).bgra;
    const uint32_t a = ((texel >> 24) * (in.color >> 24) + 127u) / 255u;
    return trgl_frag_out{ a == 0u, trgl_blend_over((in.color & 0x00ffffffu) | (a << 24), in.dst) };
}
"""


def fnv1a(fb):
    digest = 1469598103934665603
    for b in fb.reshape(-1).tolist():
        digest = ((digest ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return digest


def demo_scene():
    """The arrays of demo_particles.cpp, with its arithmetic."""
    Cq = 2
    nv, nt = 6 * (Cq + 1) ** 2, 12 * Cq * Cq
    verts, faces, col = np.zeros((nv, 8)), np.zeros((nt, 3), np.uint32), np.zeros(nt, np.uint32)
    for f in range(6):
        axis, side = f // 2, (-1.0 if f % 2 else 1.0)
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for j in range(Cq + 1):
            for i in range(Cq + 1):
                v = verts[(f * (Cq + 1) + j) * (Cq + 1) + i]
                v[axis], v[a1], v[a2] = side, side * (-1.0 + 1.0 * i), -1.0 + 1.0 * j
                v[3 + axis] = side
                v[6], v[7] = 0.5 * i, 0.5 * j
        for j in range(Cq):
            for i in range(Cq):
                q = (f * Cq + j) * Cq + i
                v00 = (f * (Cq + 1) + j) * (Cq + 1) + i
                v10, v01 = v00 + 1, v00 + Cq + 1
                faces[2 * q], faces[2 * q + 1] = (v00, v10, v01 + 1), (v00, v01 + 1, v01)
                col[2 * q:2 * q + 2] = 0xFF000000 | (0x303030 + f * 0x180C06)
    edges = np.stack([faces, np.roll(faces, -1, axis=1)], axis=2).reshape(-1)          # (v0, v1), (v1, v2), (v2, v0) per triangle
    n, state = 4096, [12345]

    def nxt():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return state[0] >> 8

    pts, pcol = np.zeros((n, 4)), np.zeros(n, np.uint32)
    for i in range(n):
        for c in range(3):
            pts[i, c] = nxt() / 4194304.0 - 2.0
        pts[i, 3] = 0.0625 + nxt() / 67108864.0
        bgr = nxt() & 0xFFFFFF
        pcol[i] = bgr | ((96 + (nxt() & 127)) << 24)
    ts = 32
    blob = np.full((ts, ts, 4), 255, np.uint8)
    d = 2 * np.arange(ts) + 1 - ts
    d2 = d[None, :] ** 2 + d[:, None] ** 2
    blob[:, :, 3] = np.where(d2 >= 961, 0, 255 - (255 * d2) // 961)
    return dict(verts=verts, faces=faces, col=col, edges=edges.astype(np.uint32), pts=pts, pcol=pcol, blob=blob)


@pytest.mark.gpu
def test_demo_particles_equals_the_binding_from_host_arrays():
    assert os.path.exists(DEMO), "examples/demo_particles not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    u = make_uniforms(MV, tex_diffuse=0)
    sp = api.make_sprite_params(MV, PROJ, mode=api.SPRITE_VIEW, size_offset=3)
    mv_near = MV.copy()
    mv_near[11] = -5.0 + 0.015625
    lp = api.make_line_params(mv_near, PROJ, 1.5, (0.5 * W, 0.5 * H), 1.0)
    want = {}
    with Context(W, H, 3) as ctx:
        kind = ctx.register_shader(PARTICLE_SRC, 6, True, reads_dest=True, depth_write=False)
        ctx.upload_texture(0, sc["blob"])
        ctx.clear((48, 32, 24, 255), np.inf)
        clip, _ = ctx.vertex_stage(-1, u, PROJ, sc["verts"], sc["faces"])
        ctx.draw(FLAT, clip, colors=sc["col"])
        fb, st = ctx.read_framebuffer(), ctx.stats()
        want["box"] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]}"
        assert st[1] > 1000
        q_clip, q_vary, q_col = api.sprite_stage(sp, sc["pts"], sc["pcol"])
        depths = api.triangle_depths(q_clip, 2, T.CENTROID)
        order = api.depth_order(depths)
        assert np.array_equal(order, O.order(T.depths(q_clip, 2, T.CENTROID)))
        ctx.draw(kind, q_clip, q_vary, q_col, u, order=order, group=2)
        fb, st = ctx.read_framebuffer(), ctx.stats()
        want["particles"] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]}"
        ctx.draw_lines(FLAT, lp, sc["verts"], sc["edges"], np.full(len(sc["edges"]) // 2, 0xFFFFFFFF, np.uint32))
        fb, st = ctx.read_framebuffer(), ctx.stats()
        want["wireframe"] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]}"
        assert st[0] == len(sc["faces"]) + 2 * len(sc["pts"]) + len(sc["edges"])
        white = (fb == 255).all(axis=-1).sum()
        assert white > 100, "the wireframe is not on top of the box"
    # the rows the demo's particles become are the model's (the first 64 points: the model is slow)
    Pm = dict(model_view=MV, projection=PROJ, size=0.0, scale=(0.0, 0.0), mode=M.VIEW, size_offset=3, attr_offset=0, n_attr=0)
    assert np.array_equal(q_clip[:128].view(np.uint64), M.sprites(Pm, sc["pts"][:64])[0].view(np.uint64))
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert got == want


@pytest.mark.gpu
def test_demo_particles_through_the_shim_equals_the_binding():
    """gl_draw_sprites and gl_draw_lines from host arrays under the shim's globals: opaque FLAT squares and the white wireframe."""
    assert os.path.exists(DEMO), "examples/demo_particles not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    # the box's rows: eye = ModelView * (p, 1), clip = Perspective * eye, summed from 0 as the demo's dot4
    mv, pr = MV.reshape(4, 4), PROJ.reshape(4, 4)
    rows = np.array([[c for i in f for c in M.matvec(pr, M.matvec(mv, list(sc["verts"][i, :3]) + [M.ONE]))] for f in sc["faces"]])
    sp = api.make_sprite_params(MV, PROJ, 6.0, (1.0 / (W / 2.0), 1.0 / (H / 2.0)), api.SPRITE_SCREEN)
    mv_near = MV.copy()
    mv_near[11] = -5.0 + 0.015625
    lp = api.make_line_params(mv_near, PROJ, 1.5, (W / 2.0, H / 2.0), 1.0)
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, rows, colors=np.full(len(rows), 0xFF506070, np.uint32))
        ctx.draw_sprites(FLAT, sp, sc["pts"][:512], sc["pcol"][:512])
        ctx.draw_lines(FLAT, lp, sc["verts"], sc["edges"], np.full(len(sc["edges"]) // 2, 0xFFFFFFFF, np.uint32))
        fb, line = ctx.read_framebuffer(), ctx.stats_line()
        assert ctx.stats()[0] == len(rows) + 1024 + len(sc["edges"])
    r = subprocess.run([DEMO, str(W), str(H), "shim"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")] == [line]
    assert dict(ln.split(": ", 1) for ln in r.stdout.splitlines()) == {"frame digest": "%016x" % fnv1a(fb)}
