"""examples/demo_blend.cpp - opaque wedges, then two translucent layers through the shim with trgl_blend_over and depth writes off -
against the same scene drawn through the Python binding, and both against the model."""
import os
import subprocess

import numpy as np
import pytest

import blend_model as B
from tinyrenderder_amd import api, scenes
from tinyrenderder_amd.api import Context, FLAT

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(ROOT, "examples", "demo_blend")
CLEAR = (48, 32, 24, 255)        # TGAColor(24, 32, 48) as B, G, R, A


def tri(x0, y0, x1, y1, x2, y2, z):
    return [x0, y0, z, 1.0, x1, y1, z, 1.0, x2, y2, z, 1.0]


def demo_scene():
    """The triangles of demo_blend.cpp: (opaque clip, colours), (translucent clip, colours), in its order and with its arithmetic."""
    opaque, ocol = [], []
    for i in range(6):
        x = -0.875 + 0.3125 * i
        opaque.append(tri(x, -0.75, x + 0.25, -0.75, x + 0.125, 0.75, 0.0))
        ocol.append(scenes.pack_bgra((255 - 40 * i) & 255, 200, (40 * i) & 255, 255))
    glass = [tri(-1.0, -0.5, 1.0, -0.5, 0.0, 0.25, 0.5), tri(-0.75, 0.5, 0.0, -0.625, 0.75, 0.5, -0.25),
             tri(-0.5, -0.25, 0.5, -0.25, 0.0, 0.625, -0.5), tri(-0.25, -0.875, 0.875, 0.0, -0.25, 0.875, -0.5)]
    gcol = [scenes.pack_bgra(64, 64, 255, 128), scenes.pack_bgra(64, 255, 64, 96), scenes.pack_bgra(255, 64, 64, 160), scenes.pack_bgra(255, 255, 255, 48)]
    return (np.array(opaque, np.float64), np.array(ocol, np.uint32)), (np.array(glass, np.float64), np.array(gcol, np.uint32))


@pytest.mark.gpu
def test_demo_blend_equals_the_binding_and_the_model(tmp_path):
    assert os.path.exists(DEMO), "examples/demo_blend not built: run __graft_entry__.build()"
    W, H = 160, 120
    out = str(tmp_path / "blend.tga")
    r = subprocess.run([DEMO, out, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")]
    (oclip, ocol), (gclip, gcol) = demo_scene()
    with Context(W, H, 3) as ctx:
        glass = ctx.register_shader(B.OVER_SRC, 0, True, reads_dest=True, depth_write=False)
        ctx.clear(CLEAR, np.inf)
        ctx.draw(FLAT, oclip, None, ocol)
        ctx.draw(glass, gclip, None, gcol)
        fb, z, stats, line = ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()
    m = B.Model(W, H, 3, clear=CLEAR)
    m.draw(oclip, ocol, B.f_source)
    opaque_z = m.z.copy()
    m.draw(gclip, gcol, B.f_over, depth_write=False)
    assert (fb == m.fb).all() and (z.view(np.uint64) == opaque_z.view(np.uint64)).all() and stats == m.stats
    assert lines == [line]
    assert open(out, "rb").read() == api.tga_encode(fb)
    # the scene shows what it is meant to: the pane behind the wedges is hidden by them, the panes in front are not
    only_opaque = B.Model(W, H, 3, clear=CLEAR)
    only_opaque.draw(oclip, ocol, B.f_source)
    covered = opaque_z != np.inf
    changed = (fb != only_opaque.fb).any(axis=-1)
    assert (changed & covered).any() and (changed & ~covered).any() and (~changed & covered).any()
