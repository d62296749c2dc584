"""examples/demo_scene.cpp - main.cpp's scene logic over the shim: three models with model matrices, getWorldAABB ->
frustum.intersects -> draw or count, the depth snapshot around the eyes (gl_zbuffer_snapshot / gl_zbuffer_restore in place of
main.cpp:700,730), gl_postprocess, the culling statistics of main.cpp:794-799 - against the CPU oracle drawing the models that
tests/scene_model.py finds visible."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scene_model
from oracle import orc
from tinyrenderder_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "examples", "demo_scene")
W, H, BPP = 320, 240, 3


def _matmul(a, b):
    out = np.zeros((4, 4))
    for i in range(4):                       # summed from 0.0, left to right, as mat * mat does
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc += a[i, k] * b[k, j]
            out[i, j] = acc
    return out


def _indexed(level):
    """A displaced icosphere as an indexed mesh: one 14-double record per face corner (position, normal, uv, zeros)."""
    hd = scenes.head_standin(level, W, H)
    nf = hd["positions"].shape[0]
    v = np.zeros((nf * 3, 14))
    v[:, 0:3] = hd["positions"].reshape(-1, 3); v[:, 3:6] = hd["normals"].reshape(-1, 3); v[:, 6:8] = hd["uvs"].reshape(-1, 2)
    return v, np.arange(nf * 3, dtype=np.uint32).reshape(nf, 3), hd


def _model_matrix(scale, tx, ty, tz):
    m = np.eye(4)
    m[0, 0] = m[1, 1] = m[2, 2] = scale
    m[0, 3], m[1, 3], m[2, 3] = tx, ty, tz
    return m


def _eye_lights(mv, world):
    out = {}
    for k, d in world.items():               # main.cpp:58-68: the upper-left 3x3 of ModelView times the direction, normalized
        e = np.array([((0.0 + mv[r, 0] * d[0]) + mv[r, 1] * d[1]) + mv[r, 2] * d[2] for r in range(3)])
        out[k] = e / np.sqrt((0.0 + e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return out


# where the first model ("sponza") sits: far to the side of the view, or across the frustum's side plane
SPONZA = {"culled": _model_matrix(0.5, 40.0, 0.0, 0.0), "straddling": None}


@pytest.mark.gpu
@pytest.mark.parametrize("sponza_at", sorted(SPONZA))
def test_scene_demo_culls_and_draws_like_the_oracle(tmp_path, sponza_at):
    assert os.path.exists(DEMO), "examples/demo_scene not built: run __graft_entry__.build()"
    sv, si, _ = _indexed(2)
    hv, hi, hd = _indexed(3)
    ev, ei = hv[: 3 * (hi.shape[0] // 3)].copy(), hi[: hi.shape[0] // 3].copy()          # a third of the head's faces stand in for the eyes
    view, proj = hd["model_view"], hd["projection"]
    vp = _matmul(proj, view)
    sponza_m = SPONZA[sponza_at]
    if sponza_m is None:
        # slide the model along +x of the view until its box crosses the frustum's RIGHT plane but its centre is outside
        planes = scene_model.frustum_from_matrix(vp)
        right = view[0, :3]
        for t in np.arange(0.5, 20.0, 0.05):
            cand = _model_matrix(0.5, *(right * t))
            box = scene_model.aabb_transform(*scene_model.compute_aabb(sv), cand)
            centre = (box[0] + box[1]) * 0.5
            if planes[1, :3] @ centre + planes[1, 3] < 0:
                sponza_m = cand
                break
        assert sponza_m is not None and scene_model.frustum_intersects(planes, *box)
    models = [(sv, si, sponza_m), (hv, hi, _model_matrix(1.0, 0.0, 0.0, 0.0)), (ev, ei, _model_matrix(1.02, 0.0, 0.0, 0.0))]

    scene, out = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(scene, "wb") as f:
        f.write(b"TRGSCN01")
        f.write(struct.pack("<4i", W, H, BPP, 3))
        f.write(np.asarray(view, np.float64).tobytes()); f.write(np.asarray(proj, np.float64).tobytes())
        for k in ("key", "fill", "rim"):
            f.write(np.asarray(hd["world_lights"][k], np.float64).tobytes())
        for v, i, m in models:
            f.write(struct.pack("<ii", v.shape[0], i.shape[0])); f.write(m.tobytes()); f.write(v.tobytes())
            b = i.tobytes(); f.write(b + b"\0" * ((8 - len(b) % 8) % 8))
    r = subprocess.run([DEMO, str(scene), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    npx = W * H
    fb = np.frombuffer(raw, np.uint8, npx * BPP).reshape(H, W, BPP)
    z = np.frombuffer(raw, np.float64, npx, npx * BPP).reshape(H, W)
    off = npx * BPP + npx * 8
    zimg, ao, final = (np.frombuffer(raw, np.uint8, npx * 3, off + k * npx * 3).reshape(H, W, 3) for k in range(3))
    text = raw[off + 3 * npx * 3:].decode()

    visible, stats = scene_model.cull_scene(vp, [(v, i.shape[0], m) for v, i, m in models])
    assert visible == [sponza_at == "straddling", True, True]
    assert text.split("\n", 1)[1] == scene_model.format_culling_stats(stats)
    assert r.stdout == scene_model.format_culling_stats(stats)

    o = orc.Oracle(W, H, BPP)
    z_before_eyes = None
    for n, ((v, i, m), vis) in enumerate(zip(models, visible)):
        if not vis:
            continue
        mv = _matmul(view, m)
        clip, vary = orc.vertex_stage(mv, proj, v, i)
        lt = _eye_lights(mv, hd["world_lights"])
        if n == 2:
            z_before_eyes = o.z.copy()                                        # main.cpp:700
            o.draw(orc.EYE, clip, vary, uniforms=orc.make_uniforms(mv, lt["key"], lt["fill"], lt["rim"], 1.0, -1, -1, -1))
        else:
            o.draw(orc.PHONG, clip, vary, uniforms=orc.make_uniforms(mv, lt["key"], lt["fill"], lt["rim"], 0.5 if n == 0 else 1.0, -1, -1, -1))
    assert not np.array_equal(o.z.view(np.uint64), z_before_eyes.view(np.uint64)), "the eyes must change the depths for the restore to show"
    o.z[...] = z_before_eyes                                                  # main.cpp:730
    assert np.array_equal(z.view(np.uint64), o.z.view(np.uint64))
    d8 = np.abs(fb.astype(np.int16) - o.fb.astype(np.int16))
    assert d8.max() <= 1 and (d8.max(axis=-1) > 0).mean() <= 1e-3              # EYE pass: pow tolerance (see test_gpu_parity)
    line = text.split("\n", 1)[0]
    assert line == orc.format_stats_line(o.stats)
    assert r.stderr.strip().endswith(line)
    # main.cpp:751-785 on the restored depths
    want_ao = orc.ssao(o.z)
    assert np.array_equal(zimg, orc.zbuffer_image(o.z)) and np.array_equal(ao, want_ao)
    assert np.array_equal(final, orc.composite(fb, want_ao))
    if sponza_at == "straddling":
        assert o.stats[0] == si.shape[0] + hi.shape[0] + ei.shape[0]          # every face of the straddling model went to rasterize()
