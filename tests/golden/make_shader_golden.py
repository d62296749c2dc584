"""Generate the fixtures that pin the PHONG / EYE shading, the vertex stage and the post-process rows to the REFERENCE's own
main.cpp and model.cpp, through oracle/_ref/ref_shaders (the reference's PhongShader, EyeShader, save_zbuffer_image,
compute_ssao_at and Model, compiled in place against declaration-only Assimp stand-ins, see oracle/Makefile):

  shader_golden.npz       bgra[4] + bytespp of ~20 k single fragment() calls (tests/cases.py shader_fragment_inputs) and the
                          digest of their inputs
  lights_golden.bin       PhongShader / EyeShader ::initLightDirections on seeded ModelViews and world directions: int32 count,
                          int32 0, then per item 25 input doubles (ModelView[16], key, fill, rim) and 15 output doubles (Phong
                          key, fill, rim, Eye key, rim in eye space)
  next_rows_golden.json   N1: the fixture mesh (cases.fixture_mesh) through Model::load + shader.vertex + rasterize() (digests of
                          clip, varyings, frame and its stats line, for PHONG and EYE); N4: digests of save_zbuffer_image and the
                          SSAO bytes over cases.fixture_zbuffers

Only runs where the reference tree is; the committed outputs are data.

    python tests/golden/make_shader_golden.py
"""
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
from oracle import orc  # noqa: E402
from tinyrenderder_amd import scenes  # noqa: E402

N_LIGHTS = 128


def fragment_input_digest(textures, kinds, uniforms, vary, bary):
    parts = [textures[k].ravel() for k in sorted(textures)] + [kinds, np.frombuffer(b"".join(bytes(u) for u in uniforms), np.uint8),
                                                              vary, bary]
    return scenes.digest(np.concatenate([np.ascontiguousarray(p).view(np.uint8).ravel() for p in parts]))


def light_inputs(n=N_LIGHTS, seed=0x119):
    """[n, 25]: ModelView[16] (lookat frames, scaled and sheared ones, identity), key, fill, rim world directions (unit,
    unnormalized, zero)."""
    r = scenes.SplitMix64(seed)
    rows = np.zeros((n, 25))
    for i in range(n):
        eye = r.uniform(3, -3.0, 3.0)
        mv = scenes.lookat(eye, r.uniform(3, -0.5, 0.5), [0, 1, 0])
        if i % 4 == 1:
            mv[:3, :3] = mv[:3, :3] * r.uniform(9, 0.5, 2.0).reshape(3, 3)
        elif i % 4 == 2:
            mv = np.eye(4)
        rows[i, :16] = mv.reshape(16)
        d = r.uniform(9, -2.0, 2.0).reshape(3, 3)
        if i % 5 == 3:
            d[i % 3] = 0.0
        rows[i, 16:] = d.reshape(9)
    return rows


def main():
    assert orc.ref_available(), "oracle/_ref/ref_shaders missing: run `make -C oracle` where the reference tree exists"
    tex, kinds, uni, vary, bary = cases.shader_fragment_inputs()
    out = orc.run_reference_fragments(tex, kinds, uni, vary, bary)
    np.savez_compressed(os.path.join(HERE, "shader_golden.npz"), out=out,
                        inputs=np.array(fragment_input_digest(tex, kinds, uni, vary, bary)))
    print(len(kinds), "fragments")

    li = light_inputs()
    lo = orc.run_reference_lights(li[:, :16], li[:, 16:19], li[:, 19:22], li[:, 22:25])
    with open(os.path.join(HERE, "lights_golden.bin"), "wb") as f:
        f.write(struct.pack("<2i", N_LIGHTS, 0))
        f.write(np.ascontiguousarray(np.concatenate([li, lo], 1)).tobytes())
    print(N_LIGHTS, "light sets")

    verts, idx, u, proj, w, h = cases.fixture_mesh()
    tx = cases.edge_textures()
    n1 = dict(inputs=scenes.digest(verts) + scenes.digest(idx) + scenes.digest(np.frombuffer(bytes(u), np.uint8)) + scenes.digest(proj))
    for name, kind in (("phong", orc.PHONG), ("eye", orc.EYE)):
        clip, vr, fb, z, line = orc.run_reference_mesh(w, h, 3, kind, scenes.init_viewport(0, 0, w, h), proj, u, verts, idx, tx)
        n1[name] = dict(clip=scenes.digest(clip), varyings=scenes.digest(vr), fb=scenes.digest(fb), z=scenes.digest(z), stats=line)
        print("mesh", name, line)
    n4 = {}
    for name, z in cases.fixture_zbuffers().items():
        n4[name] = dict(inputs=scenes.digest(z), zimage=scenes.digest(orc.run_reference_zbuffer_image(z)),
                        ao=scenes.digest(orc.run_reference_ssao(z)))
    with open(os.path.join(HERE, "next_rows_golden.json"), "w") as f:
        json.dump(dict(mesh=n1, zbuffers=n4), f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
