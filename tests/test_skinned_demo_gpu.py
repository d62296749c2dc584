"""examples/demo_skinned.cpp - an arm of three bones whose palettes and skinned vertices exist in device memory only, drawn with PHONG
under three poses - against the same scene restated here: the host twins' meshes drawn through the Python binding from host arrays."""
import os
import subprocess

import numpy as np
import pytest

import skin_model as M
from tinyrenderder_amd import api
from tinyrenderder_amd.api import Context, PHONG, make_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_skinned")
MV = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -5, 0, 0, 0, 1], np.float64)
PROJ = np.array([1.25, 0, 0, 0, 0, 2, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64)
FLAGS = M.NORMAL | M.TANGENT


def fnv1a(fb):
    digest = 1469598103934665603
    for b in fb.reshape(-1).tolist():
        digest = ((digest ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return digest


def joint_matrix(c, s, tx):
    return np.array([c, -s, 0, tx, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], np.float64)


def demo_scene():
    """The arrays of demo_skinned.cpp, with its arithmetic."""
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
    parents = np.array([-1, 0, 1], np.int32)
    ib = np.stack([joint_matrix(1.0, 0.0, 1.5 - j) for j in range(3)])
    bend = [[(1, 0), (1, 0), (1, 0)], [(1, 0), (0.8, 0.6), (1, 0)], [(0.96, -0.28), (0.6, 0.8), (0.8, -0.6)]]
    local = np.stack([np.stack([joint_matrix(float(c), float(s), -1.5 if j == 0 else 1.0) for j, (c, s) in enumerate(pose)]) for pose in bend])
    return dict(verts=verts, joints=joints, weights=weights, faces=np.array(faces, np.uint32), parents=parents, ib=ib, local=local)


@pytest.mark.gpu
def test_demo_skinned_equals_the_host_twins_drawn_through_the_binding():
    assert os.path.exists(DEMO), "examples/demo_skinned not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    u = make_uniforms(MV)
    palettes = api.pose_palette(sc["parents"], sc["local"], sc["ib"])
    assert np.array_equal(palettes.view(np.uint64), M.pose_palette(sc["parents"], sc["local"], sc["ib"]).view(np.uint64))
    skinned = api.skin_stage(sc["verts"], sc["joints"], sc["weights"], palettes, FLAGS)
    assert np.array_equal(skinned.view(np.uint64), M.skin(sc["verts"], sc["joints"], sc["weights"], palettes, FLAGS).view(np.uint64))
    # the rest pose is the rest mesh (the palette is identities up to the sign of a zero), the bent ones leave the rest mesh's box
    assert np.array_equal(skinned[0, :, :3], sc["verts"][:, :3]) and skinned[1, :, 1].max() > 0.5 and skinned[2, :, 1].max() > 0.5
    want = {}
    with Context(W, H, 3) as ctx:
        for q in range(3):
            lo, hi = api.mesh_bounds(skinned[q])
            ctx.clear((24, 24, 32, 255), np.inf)
            ctx.draw_indexed(PHONG, u, PROJ, skinned[q], sc["faces"])
            fb, st = ctx.read_framebuffer(), ctx.stats()
            assert st[0] == (q + 1) * len(sc["faces"]) and st[1] > 400 * (q + 1)
            want[f"pose {q}"] = f"digest {fnv1a(fb):016x} fragments_drawn {st[1]} bounds " + " ".join("%.17g" % x for x in list(lo) + list(hi))
    assert len({w.split()[1] for w in want.values()}) == 3
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(": ", 1) for ln in r.stdout.splitlines())
    assert got == want


@pytest.mark.gpu
def test_demo_skinned_through_the_shim_equals_the_binding():
    """gl_pose_palette and gl_draw_skinned from host arrays under the shim's globals: the last pose."""
    assert os.path.exists(DEMO), "examples/demo_skinned not built: run __graft_entry__.build()"
    W, H = 160, 100
    sc = demo_scene()
    palette = api.pose_palette(sc["parents"], sc["local"][2:3], sc["ib"])
    with Context(W, H, 3) as ctx:
        ctx.draw_skinned(PHONG, make_uniforms(MV), PROJ, sc["verts"], sc["joints"], sc["weights"], palette, sc["faces"], FLAGS)
        fb, line = ctx.read_framebuffer(), ctx.stats_line()
        assert ctx.stats()[0] == len(sc["faces"]) and ctx.stats()[1] > 400
    r = subprocess.run([DEMO, str(W), str(H), "shim"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("DEBUG:")] == [line]
    assert dict(ln.split(": ", 1) for ln in r.stdout.splitlines()) == {"frame digest": "%016x" % fnv1a(fb)}
