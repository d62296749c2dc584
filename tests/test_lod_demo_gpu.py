"""examples/demo_lod.cpp - a sphere soup welded and simplified three times in device memory only, each level over the capacities of the
one before, with generated normals and a frame per level - against the same scene restated here: the host twins' weld and levels with
real counts, drawn through the Python binding from host arrays.  The demo itself compares its levels with the shim's host calls
(gl_mesh_weld, gl_mesh_simplify), and gl_mesh_clean - with and without repeated faces, and after a refused call - with trgl_mesh_clean word
for word, and exits with 3 when anything differs; the counts it prints for that are checked here."""
import os
import re
import subprocess

import numpy as np
import pytest

from tinyrenderder_amd import api
from tinyrenderder_amd.api import Context, PHONG, make_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_lod")
MV = np.array([0.8, 0, 0.6, 0, 0.36, 0.8, -0.48, 0, -0.48, 0.6, 0.64, -5, 0, 0, 0, 1], np.float64)
PROJ = np.array([1.25, 0, 0, 0, 0, 2, 0, 0, 0, 0, -1.125, -2.25, 0, 0, -1, 0], np.float64)
CELL = 1.0 / 16


def fnv1a(fb):
    digest = 1469598103934665603
    for b in fb.reshape(-1).tolist():
        digest = ((digest ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return digest


def demo_scene(level=5):
    """The soup of demo_lod.cpp, with its arithmetic: sums, one square root and three divisions per new corner."""
    pos = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    f = [0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5]
    for _ in range(level):
        mid, finer = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x, y, z = (np.float64(pos[key[0]][k]) + np.float64(pos[key[1]][k]) for k in range(3))
                length = np.sqrt(x * x + y * y + z * z)
                pos.append((float(x / length), float(y / length), float(z / length)))
                mid[key] = len(pos) - 1
            return mid[key]

        for i in range(0, len(f), 3):
            a, b, c = f[i:i + 3]
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            finer += [a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca]
        f = finer
    v = np.zeros((len(f), 8))
    v[:, :3] = np.array(pos, np.float64)[f]
    return v, np.arange(len(f), dtype=np.uint32).reshape(-1, 3)


@pytest.mark.gpu
def test_demo_lod_equals_the_host_twins_drawn_through_the_binding():
    assert os.path.exists(DEMO), "examples/demo_lod not built: run __graft_entry__.build()"
    W, H = 160, 100
    v, f = demo_scene()
    r = subprocess.run([DEMO, str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    out, U = api.mesh_weld(api.make_weld_params(8, 0, 3), v, f)
    assert U == 4 ** 6 + 2 and lines[0] == f"level 0: welded, {f.shape[0]} faces, {U} vertices", lines
    verts, faces = np.ascontiguousarray(out["vertices"][:U]), out["indices"]
    counts = [(f.shape[0], U)]
    # the demo's gl_mesh_clean check, restated: level 0 welded again on a grid, between two records nobody names, its first whole face once
    # more rotated and once mirrored
    g, Ug = api.mesh_weld(api.make_weld_params(8, 0, 3, 2 * CELL), verts, faces)
    cv = np.concatenate([np.full((1, 8), 7.0), g["vertices"][:Ug], np.full((1, 8), 7.0)])
    ci = g["indices"] + np.uint32(1)
    t = int(np.argmax((ci[:, 0] != ci[:, 1]) & (ci[:, 1] != ci[:, 2]) & (ci[:, 2] != ci[:, 0])))      # the first face with three distinct corners
    ci = np.concatenate([ci, ci[t][[1, 2, 0]][None], ci[t][[2, 1, 0]][None]]).astype(np.uint32)
    kept = [api.mesh_clean(api.make_clean_params(8, flags), ci, cv)[1] for flags in (api.CLEAN_DUPLICATES | api.CLEAN_VERTICES, api.CLEAN_VERTICES)]
    assert kept[0][0] + 1 == kept[1][0] < ci.shape[0] and kept[0][1] == kept[1][1] == Ug, "degenerate faces, one repeated face, one mirrored one, two unused vertices"
    assert lines[4] == (f"clean: {kept[0][0]} of {ci.shape[0]} faces and {kept[0][1]} of {Ug + 2} vertices; with repeated faces kept "
                        f"{kept[1][0]} of {ci.shape[0]} faces and {kept[1][1]} of {Ug + 2} vertices"), lines
    with Context(W, H, 3) as ctx:
        u = make_uniforms(MV.reshape(4, 4), (0, 0, 1), (0, 0, 1), (0, 0, 1))
        for level in (1, 2, 3):
            cell = CELL * 2 ** (level - 1)
            out, (K, Vk) = api.mesh_simplify(api.make_simplify_params(8, cell, 3), verts, faces)
            verts, faces = np.ascontiguousarray(out["vertices"][:Vk]), np.ascontiguousarray(out["indices"][:K])
            counts.append((K, Vk))
            shaded, generated = api.mesh_normals(verts, faces)
            assert generated, "the kept records carry the soup's zero normals"
            ctx.clear((200, 208, 216, 255), np.inf)
            ctx.draw_indexed(PHONG, u, PROJ.reshape(4, 4), shaded, faces)
            fb, stats = ctx.read_framebuffer(), ctx.stats()
            m = re.fullmatch(r"level (\d): cell (\S+), (\d+) faces, (\d+) vertices, frame digest ([0-9a-f]{16}) fragments_drawn (\d+)", lines[level])
            assert m, lines
            assert (int(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4))) == (level, cell, K, Vk), lines[level]
            assert (int(m.group(5), 16), int(m.group(6))) == (fnv1a(fb), stats[1]), f"level {level}: the demo's frame differs from the host twins' drawn through the binding"
            assert stats[1] > 0 and (fb != np.array([200, 208, 216], np.uint8)).any()
    assert all(a[0] > b[0] > 0 and a[1] > b[1] for a, b in zip(counts, counts[1:])), f"every level is smaller than the one before: {counts}"
