"""examples/demo_instanced.cpp - an occluder wall, trgl_occlusion_boxes with boxes and codes in device memory, one trgl_draw_instanced
of a cube over a grid of matrices gated by those codes - against the same scene drawn through the Python binding, and against the
numpy models of both steps."""
import os
import re
import subprocess

import numpy as np
import pytest

import instance_model as M
import occlusion_model as om
import vertex_shader_sources as V
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(ROOT, "examples", "demo_instanced")
NX, NY = 12, 6


def demo_scene():
    """The numbers of demo_instanced.cpp, in its order and with its arithmetic (dyadic fractions throughout)."""
    mv = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -5], [0, 0, 0, 1]], np.float64)
    proj = np.array([[1.25, 0, 0, 0], [0, 2, 0, 0], [0, 0, -1.125, -2.25], [0, 0, -1, 0]], np.float64)
    wall_v = np.array([[-6, -4, 0], [0, -4, 0], [0, 4, 0], [-6, 4, 0]], np.float64)
    wall_clip, _ = V.expect_clip(mv, proj, wall_v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    p = np.array([[0.5 if k & 1 else -0.5, 0.5 if k & 2 else -0.5, 0.5 if k & 4 else -0.5] for k in range(8)])
    cube = np.concatenate([p, p * 0.5, p[:, :2] + 0.5], 1)
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                     np.uint32)
    centres = np.array([[-2.75 + 0.5 * i, -1.25 + 0.5 * j, -3.0] for j in range(NY) for i in range(NX)])
    inst = np.zeros((NX * NY, 16))
    inst[:, [0, 5, 10]] = 0.25
    inst[:, 15] = 1.0
    inst[:, [3, 7, 11]] = centres
    boxes = np.concatenate([centres - 0.1875, centres + 0.1875], 1)
    return dict(mv=mv, proj=proj, view_proj=M.mat_product(proj, mv).reshape(16), wall=wall_clip, wall_col=np.full(2, 0xFF808890, np.uint32),
                cube=np.ascontiguousarray(cube), faces=faces, inst=inst, boxes=boxes)


def fnv1a(fb):
    h = 1469598103934665603
    for b in fb.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run_demo(*args):
    r = subprocess.run([DEMO, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    stats = [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")]
    out = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    return stats, out


@pytest.mark.gpu
def test_demo_instanced_equals_the_binding_and_the_models():
    assert os.path.exists(DEMO), "examples/demo_instanced not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    n = NX * NY
    u = make_uniforms(sc["mv"])
    with Context(W, H, 3) as ctx:
        ctx.draw(FLAT, sc["wall"], colors=sc["wall_col"])
        z_wall = ctx.read_zbuffer()
        codes = ctx.occlusion_boxes(sc["view_proj"], sc["boxes"])
        ctx.draw_instanced(PHONG, u, sc["proj"], sc["cube"], sc["faces"], instances=sc["inst"], visible=codes)
        fb, stats, line = ctx.read_framebuffer(), ctx.stats(), ctx.stats_line()
    want = om.codes(z_wall, scenes.init_viewport(0, 0, W, H), sc["view_proj"], sc["boxes"])
    assert np.array_equal(codes, want)
    drawn = int((codes & 1).sum())
    assert (want == om.HIDDEN).sum() >= n // 4 and (want == om.VISIBLE).sum() >= n // 4
    assert stats[0] == 2 + 12 * drawn

    lines, out = run_demo(str(W), str(H))
    assert lines == [line]
    assert out["cubes drawn"] == f"{drawn} of {n}"
    assert out["frame digest"] == "%016x" % fnv1a(fb)
    # every cube drawn: the same frame and as many fragments - a skipped cube had none to give
    lines_all, out_all = run_demo(str(W), str(H), "all")
    assert out_all["cubes drawn"] == f"{n} of {n}" and out_all["frame digest"] == out["frame digest"]
    frags = lambda ln: int(re.search(r"fragments_drawn=(\d+)", ln).group(1))
    assert frags(lines_all[0]) == frags(line) == stats[1]
    # the same scene through the shim (gl_occlusion_test + gl_draw_instanced with host matrices and codes)
    lines_shim, out_shim = run_demo(str(W), str(H), "shim")
    assert lines_shim == [line] and out_shim == out
    # and the rows behind the frame are the model's
    with Context(W, H, 3) as ctx:
        clip, vary, col, rows = ctx.instance_stage(-1, u, sc["proj"], sc["cube"], sc["faces"], instances=sc["inst"], visible=codes)
    mclip, mvary, _ = M.builtin_rows(sc["mv"], sc["proj"], sc["cube"], sc["faces"], sc["inst"], codes)
    assert rows == 12 * drawn and col is None
    assert np.array_equal(clip.view(np.uint64), mclip.view(np.uint64)) and np.array_equal(vary.view(np.uint64), mvary.view(np.uint64))
