"""examples/demo_sorted.cpp - translucent quads drawn in array order and through trgl_instance_depths, trgl_depth_order and
trgl_draw_instanced_ordered with everything in device memory, then a discarding kind under the three orders - against the same scene
drawn through the Python binding, and against the numpy model of the order."""
import os
import subprocess

import numpy as np
import pytest

import cases
import order_model as O
import vertex_shader_sources as V
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(ROOT, "examples", "demo_sorted")
NX, NY = 16, 12
GLASS = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }
"""
CUTOUT = r"""
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ (in.color >> 24) < 96u, in.color }; }
"""


def demo_scene():
    """The numbers of demo_sorted.cpp, in its order and with its arithmetic (dyadic fractions throughout)."""
    mv = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -5], [0, 0, 0, 1]], np.float64)
    proj = np.array([[1.25, 0, 0, 0], [0, 2, 0, 0], [0, 0, -1.125, -2.25], [0, 0, -1, 0]], np.float64)
    wall_v = np.array([[-8, -5, -4], [8, -5, -4], [8, 5, -4], [-8, 5, -4]], np.float64)
    wall_clip, _ = V.expect_clip(mv, proj, wall_v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    quad = np.array([[-0.5, -0.5, 0, 0, 0, 1, 0, 0], [0.5, -0.5, 0, 0, 0, 1, 1, 0], [0.5, 0.5, 0, 0, 0, 1, 1, 1], [-0.5, 0.5, 0, 0, 0, 1, 0, 1]], np.float64)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    k = np.arange(NX * NY)
    inst = np.zeros((NX * NY, 16))
    inst[:, [0, 5, 10]] = 0.75
    inst[:, 15] = 1.0
    inst[:, 3] = -2.5 + 0.3125 * (k % NX)
    inst[:, 7] = -1.375 + 0.25 * (k // NX)
    inst[:, 11] = -3.0 + ((k * 37) % 64) / 16.0
    col = (((k.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 8) | ((64 + (k * 53) % 128).astype(np.uint64) << 24)
    return dict(mv=mv, proj=proj, wall=wall_clip, wall_col=np.full(2, 0xFF506070, np.uint32), quad=quad, faces=faces, inst=inst,
                col=col.astype(np.uint32))


def fnv1a(fb):
    h = 1469598103934665603
    for b in fb.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_demo_sorted_equals_the_binding_and_the_model():
    import torch
    assert os.path.exists(DEMO), "examples/demo_sorted not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    n = NX * NY
    u = make_uniforms(sc["mv"])
    want = {}
    with Context(W, H, 3) as ctx:
        kinds = dict(translucent=ctx.register_shader(GLASS, 24, True, reads_dest=True, depth_write=False), cutout=ctx.register_shader(CUTOUT, 24, True))
        d_inst, d_col = cases.device_array(sc["inst"]), cases.device_array(sc["col"])
        torch.cuda.synchronize()
        for kind, order in (("translucent", None), ("translucent", False), ("cutout", None), ("cutout", False), ("cutout", True)):
            ctx.clear((48, 32, 24, 255), np.inf)
            ctx.reset_stats()
            ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
            o = None
            if order is not None:
                depths = ctx.instance_depths(sc["mv"], np.zeros(3), d_inst, device=True)
                o = ctx.depth_order(depths, front_to_back=order, device=True)
            ctx.draw_instanced(kinds[kind], u, sc["proj"], sc["quad"], sc["faces"], instances=d_inst, instance_colors=d_col, instances_device=True,
                               order=o, order_device=o is not None)
            fb, st = ctx.read_framebuffer(), ctx.stats()
            assert st[0] == 2 + 2 * n
            name = f"{kind}, " + ("array order" if order is None else "front to back" if order else "back to front")
            want[name] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]}"
            if order is not None:                                       # the order the device made is the model's
                d = O.depths(sc["mv"], np.zeros(3), sc["inst"])
                assert (d < 0).all()
                assert np.array_equal(o.cpu().numpy().view(np.uint32), O.order(d, int(order)))
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert got == want
    frags = {k: int(v.rsplit(" ", 1)[1]) for k, v in got.items()}
    assert frags["cutout, front to back"] < frags["cutout, array order"] < frags["cutout, back to front"]
    assert got["translucent, array order"].split()[1] != got["translucent, back to front"].split()[1], "the translucent frame does not depend on the order"


@pytest.mark.gpu
def test_demo_sorted_through_the_shim_equals_the_binding():
    """gl_instance_depths, gl_depth_order and gl_draw_instanced_ordered with host arrays: an opaque Phong material, whose frame does
    not depend on the order while fragments_drawn does."""
    assert os.path.exists(DEMO), "examples/demo_sorted not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    u = make_uniforms(sc["mv"])
    lines = {}
    for front in (False, True):
        with Context(W, H, 3) as ctx:
            ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
            order = ctx.depth_order(ctx.instance_depths(sc["mv"], np.zeros(3), sc["inst"]), front_to_back=front)
            assert np.array_equal(order, O.order(O.depths(sc["mv"], np.zeros(3), sc["inst"]), int(front)))
            ctx.draw_instanced(PHONG, u, sc["proj"], sc["quad"], sc["faces"], instances=sc["inst"], order=order)
            fb, line = ctx.read_framebuffer(), ctx.stats_line()
        r = subprocess.run([DEMO, str(W), str(H), "shim_front" if front else "shim_back"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")] == [line]
        out = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
        assert out == {"first drawn": str(int(order[0])), "frame digest": "%016x" % fnv1a(fb)}
        lines[front] = line
    assert lines[False] != lines[True], "fragments_drawn does not depend on the order"
