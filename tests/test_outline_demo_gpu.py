"""examples/demo_outline.cpp - a bent arm drawn with PHONG and outlined from an edge list and segments that exist in device memory only -
against the same scene restated here: the host twins' meshes, edges and selections drawn through the Python binding from host arrays."""
import os
import subprocess

import numpy as np
import pytest

import edge_model as M
from tinyrenderder_amd import api
from tinyrenderder_amd.api import Context, FLAT, PHONG, make_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_outline")
MV = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -5, 0, 0, 0, 1], np.float64)
PROJ = np.array([1.25, 0, 0, 0, 0, 2, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64)
EYE = (0.0, 0.0, 5.0, 1.0)
LINE_BIAS, LINE_WIDTH, ZNEAR, CREASE_COS = 1.0 / 64, 2.0, 1.0, 0.5
CLASS_COLORS = (0xFF000000, 0xFF000000, 0xFF000000, 0xFF808080)
SELECT = M.BOUNDARY | M.SILHOUETTE | M.CREASE
FLAGS = api.SKIN_NORMAL | api.SKIN_TANGENT


def fnv1a(fb):
    digest = 1469598103934665603
    for b in fb.reshape(-1).tolist():
        digest = ((digest ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return digest


def turn_about(c, s, px):
    return np.array([c, -s, 0, px - c * px, s, c, 0, -s * px, 0, 0, 1, 0, 0, 0, 0, 1], np.float64)


def demo_scene():
    """The arrays of demo_outline.cpp, with its arithmetic."""
    R, S = 13, 14
    cy, cz = (-0.25, 0.25, 0.25, -0.25), (-0.25, -0.25, 0.25, 0.25)
    verts, joints, weights, faces = np.zeros((4 * R, S)), np.zeros((4 * R, 2), np.uint16), np.zeros((4 * R, 2)), []
    for r in range(R):
        for c in range(4):
            i, bone = 4 * r + c, min(r // 4, 2)
            verts[i, :9] = (-1.5 + r / 4.0, cy[c], cz[c], 0.0, -0.6 if cy[c] < 0 else 0.6, -0.8 if cz[c] < 0 else 0.8, r / 12.0, c / 4.0, 1.0)
            on_joint = r % 4 == 0 and 0 < r < 12
            joints[i] = (bone, max(bone - 1, 0))
            weights[i] = (0.5, 0.5) if on_joint else (1.0, 0.0)
    for r in range(R - 1):
        for c in range(4):
            a, b = 4 * r + c, 4 * r + (c + 1) % 4
            faces += [(a, b + 4, a + 4), (a, b, b + 4)]
    rest = turn_about(1.0, 0.0, 0.0)
    palettes = np.stack([np.stack([rest, rest, rest]), np.stack([rest, turn_about(0.8, 0.6, -0.5), turn_about(0.8, 0.6, -0.5)])])
    return dict(verts=verts, joints=joints, weights=weights, faces=np.array(faces, np.uint32), palettes=palettes)


def line_params(W, H):
    pr = PROJ.copy()
    pr[11] = PROJ[11] - LINE_BIAS
    return api.make_line_params(MV, pr, LINE_WIDTH, (W / 2.0, H / 2.0), ZNEAR)


def edge_params(compact=True):
    return api.make_edge_params(EYE, CREASE_COS, SELECT, CLASS_COLORS, compact)


@pytest.mark.gpu
def test_demo_outline_equals_the_host_twins_drawn_through_the_binding():
    assert os.path.exists(DEMO), "examples/demo_outline not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    nv = sc["verts"].shape[0]
    skinned = api.skin_stage(sc["verts"], sc["joints"], sc["weights"], sc["palettes"], FLAGS)
    edges, E = api.mesh_edges(sc["faces"], nv)
    want_edges, want_E = M.edges(sc["faces"], nv)
    assert E == want_E and np.array_equal(edges, want_edges)
    assert E == 3 * len(sc["faces"]) // 2 + 4, "a tube of quads split in two, open at both ends: 4 boundary edges more than half the half-edges"
    want, selections = {}, []
    with Context(W, H, 3) as ctx:
        for q in range(2):
            codes, seg, col, n = api.edge_select(edge_params(), skinned[q], sc["faces"], edges, E)
            model = M.select(edges[:E], skinned[q], sc["faces"], EYE, CREASE_COS, SELECT, CLASS_COLORS, True)
            assert n == model[3] and np.array_equal(codes, model[0]) and np.array_equal(seg, model[1]) and np.array_equal(col, model[2])
            assert (codes & M.BOUNDARY != 0).sum() == 8 and {0xFF000000, 0xFF808080} == set(col[:n].tolist())
            selections.append(seg[:n].tobytes())
            ctx.clear((200, 208, 216, 255), np.inf)
            ctx.draw_indexed(PHONG, make_uniforms(MV), PROJ, skinned[q], sc["faces"])
            ctx.draw_outline(FLAT, line_params(W, H), edge_params(), skinned[q], sc["faces"], edges, E)
            fb, st = ctx.read_framebuffer(), ctx.stats()
            assert st[1] > 400 * (q + 1)
            dark = (fb.reshape(-1, 3) == 0).all(axis=1).sum()
            assert dark > 100, "the black outline must be visible in front of the surface it lies in"
            want[f"pose {q}"] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]} edges {E} selected {n}"
    assert selections[0] != selections[1] and want["pose 0"].split()[1] != want["pose 1"].split()[1]
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert got == want


@pytest.mark.gpu
def test_demo_outline_through_the_shim_equals_the_binding():
    """gl_skin_stage, gl_draw_skinned, gl_mesh_edges and gl_draw_outline from host arrays under the shim's globals: the bent pose."""
    assert os.path.exists(DEMO), "examples/demo_outline not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    palette = sc["palettes"][1:2]
    skinned = api.skin_stage(sc["verts"], sc["joints"], sc["weights"], palette, FLAGS)[0]
    edges, E = api.mesh_edges(sc["faces"], sc["verts"].shape[0])
    with Context(W, H, 3) as ctx:
        ctx.draw_skinned(PHONG, make_uniforms(MV), PROJ, sc["verts"], sc["joints"], sc["weights"], palette, sc["faces"], FLAGS)
        ctx.draw_outline(FLAT, line_params(W, H), edge_params(), skinned, sc["faces"], edges, E)
        fb, line = ctx.read_framebuffer(), ctx.stats_line()
        assert ctx.stats()[0] > len(sc["faces"]) and ctx.stats()[1] > 400
    r = subprocess.run([DEMO, str(W), str(H), "shim"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")] == [line]
    assert dict(ln.split(": ", 1) for ln in r.stdout.splitlines()) == {"frame digest": "%016x" % fnv1a(fb)}
