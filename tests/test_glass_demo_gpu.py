"""examples/demo_glass.cpp - a translucent box drawn in array order and through trgl_vertex_stage, trgl_triangle_depths,
trgl_depth_order and trgl_draw_ordered with everything in device memory, as triangles and as quads (group = 2) - against the same
scene drawn through the Python binding, and against the numpy model of the depths and the order."""
import os
import subprocess

import numpy as np
import pytest

import cases
import order_model as O
import triangle_order_model as T
import vertex_shader_sources as V
from tinyrenderder_amd.api import Context, FLAT, make_uniforms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(ROOT, "examples", "demo_glass")
CELLS = 4
GLASS = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
"""


def demo_scene():
    """The numbers of demo_glass.cpp, in its order and with its arithmetic."""
    mv = np.array([[0.8, 0, 0.6, 0], [0.36, 0.8, -0.48, 0], [-0.48, 0.6, 0.64, -5], [0, 0, 0, 1]], np.float64)
    view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -5], [0, 0, 0, 1]], np.float64)
    proj = np.array([[1.25, 0, 0, 0], [0, 2, 0, 0], [0, 0, -1.125, -2.25], [0, 0, -1, 0]], np.float64)
    wall_v = np.array([[-8, -5, -4], [8, -5, -4], [8, 5, -4], [-8, 5, -4]], np.float64)
    wall_clip, _ = V.expect_clip(view, proj, wall_v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    C = CELLS
    verts = np.zeros((6 * (C + 1) * (C + 1), 8))
    faces, col = [], []
    for f in range(6):
        axis, side = f // 2, -1.0 if f % 2 else 1.0
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for j in range(C + 1):
            for i in range(C + 1):
                v = verts[(f * (C + 1) + j) * (C + 1) + i]
                v[axis], v[a1], v[a2], v[3 + axis], v[6], v[7] = side, -1.0 + 0.5 * i, -1.0 + 0.5 * j, side, 0.25 * i, 0.25 * j
        for j in range(C):
            for i in range(C):
                q = (f * C + j) * C + i
                v00 = (f * (C + 1) + j) * (C + 1) + i
                v10, v01, v11 = v00 + 1, v00 + C + 1, v00 + C + 2
                faces += [[v00, v10, v11], [v00, v11, v01]]
                col += [(((q * 2654435761) & 0xFFFFFFFF) >> 8) | ((64 + (q * 53) % 128) << 24)] * 2
    return dict(mv=mv, proj=proj, wall=wall_clip, wall_col=np.full(2, 0xFF506070, np.uint32), verts=verts, faces=np.array(faces, np.uint32),
                col=np.array(col, np.uint64).astype(np.uint32))


def fnv1a(fb):
    h = 1469598103934665603
    for b in fb.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_demo_glass_equals_the_binding_and_the_model():
    import torch
    assert os.path.exists(DEMO), "examples/demo_glass not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    nt = len(sc["faces"])
    u = make_uniforms(sc["mv"])
    host_clip, _ = V.expect_clip(sc["mv"], sc["proj"], sc["verts"][:, :3], sc["faces"])
    want = {}
    with Context(W, H, 3) as ctx:
        glass = ctx.register_shader(GLASS, 24, True, reads_dest=True, depth_write=False)
        d_verts, d_faces, d_col = cases.device_array(sc["verts"]), cases.device_array(sc["faces"]), cases.device_array(sc["col"])
        clip = torch.empty((nt, 12), dtype=torch.float64, device="cuda")
        vary = torch.empty((nt, 24), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for name, group, mode in (("array order", 0, 0), ("sorted triangles", 1, T.CENTROID), ("sorted quads", 2, T.FARTHEST)):
            ctx.clear((48, 32, 24, 255), np.inf)
            ctx.reset_stats()
            ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
            ctx.vertex_stage(-1, u, sc["proj"], d_verts, d_faces, device=True, out=(clip, vary))
            if group == 0:
                ctx.draw(glass, clip, vary, d_col, u, device=True)
            else:
                depths = ctx.triangle_depths(clip, group, mode, device=True)
                order = ctx.depth_order(depths, device=True)
                ctx.draw(glass, clip, vary, d_col, u, device=True, order=order, order_device=True, group=group)
            fb, st = ctx.read_framebuffer(), ctx.stats()
            assert st[0] == 2 + nt
            want[name] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]}"
            if group:                                                   # the depths and the order the device made are the model's
                rows = clip.cpu().numpy()
                assert np.array_equal(rows.view(np.uint64), host_clip.view(np.uint64))
                d = T.depths(rows, group, mode)
                assert (d < 0).all() and np.array_equal(depths.cpu().numpy().view(np.uint64), d.view(np.uint64))
                assert np.array_equal(order.cpu().numpy().view(np.uint32), O.order(d))
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert got == want
    assert got["array order"].split()[1] != got["sorted triangles"].split()[1], "the translucent frame does not depend on the order"


@pytest.mark.gpu
def test_demo_glass_through_the_shim_equals_the_binding():
    """gl_triangle_depths, gl_depth_order and gl_draw_ordered with host arrays: opaque FLAT quads drawn nearest first."""
    assert os.path.exists(DEMO), "examples/demo_glass not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    clip, _ = V.expect_clip(sc["mv"], sc["proj"], sc["verts"][:, :3], sc["faces"])
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
        order = ctx.depth_order(ctx.triangle_depths(clip, 2, T.NEAREST), front_to_back=True)
        assert np.array_equal(order, O.order(T.depths(clip, 2, T.NEAREST), O.FRONT_TO_BACK))
        ctx.draw(FLAT, clip, colors=np.full(len(clip), 0xFF20A0C0, np.uint32), order=order, group=2)
        fb, line = ctx.read_framebuffer(), ctx.stats_line()
        in_order = ctx.stats()[1]
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
        ctx.draw(FLAT, clip, colors=np.full(len(clip), 0xFF20A0C0, np.uint32))
        assert in_order < ctx.stats()[1], "nearest first does not draw fewer fragments than array order"
    r = subprocess.run([DEMO, str(W), str(H), "shim"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")] == [line]
    out = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert out == {"first drawn": str(int(order[0])), "frame digest": "%016x" % fnv1a(fb)}
