"""The GPU's PHONG / EYE shading, vertex stage (N1) and post-process (N4) against fixtures taken from the reference's OWN
main.cpp and model.cpp (tests/golden/make_golden.py, make_shader_golden.py, through oracle/_ref/ref_shaders).  Only committed
fixtures are read.  PHONG frames match exactly; frames with EYE draws keep the suite's bar for pow(x, 8.0) (cases.assert_same_frame
eye=True: z exact, a colour byte at most 1 LSB off on at most 0.1 % of the pixels)."""
import json
import os

import numpy as np
import pytest

import cases
from tinyrenderder_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
NEXT_ROWS = json.load(open(os.path.join(HERE, "golden", "next_rows_golden.json")))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def whole_frames():
    """name -> the GPU's whole frame of each shading-edge case, checked against the reference's golden and the oracle."""
    out = {}
    for name in cases.SHADING_EDGE_CASES:
        case = cases.CASES[name]()
        got = cases.run_gpu(case)
        eye = cases.has_eye(case)
        cases.assert_golden(got, GOLDEN[name], eye=eye)
        cases.assert_same_frame(got, cases.run_oracle(case), eye=eye, what=f"{name} whole frame")
        out[name] = got
    return out


@pytest.mark.parametrize("name", cases.SHADING_EDGE_CASES)
def test_gpu_shading_edge_case_whole_frame(name, whole_frames):
    got = whole_frames[name]
    assert got[3] == GOLDEN[name]["stats"]


@pytest.mark.parametrize("name", cases.SHADING_EDGE_CASES)
def test_gpu_shading_edge_case_two_flushes(name):
    case = cases.CASES[name]()
    got = cases.run_gpu(case, split=2)
    cases.assert_golden(got, GOLDEN[name], eye=cases.has_eye(case))


@pytest.mark.parametrize("name", cases.SHADING_EDGE_CASES)
def test_gpu_shading_edge_case_strips_and_bands(name, whole_frames):
    """A strip context and the ranks of a banded split give the whole frame's rows, bit for bit (same device, same pow)."""
    case = cases.CASES[name]()
    full = whole_frames[name]
    h = case["height"]
    strip = (h // 3, h - 5)
    cases.assert_same_frame(cases.run_gpu(case, strip=strip), full, rows=strip, stats=False, what=f"{name} strip")
    world = 2 if h % 64 == 0 else 3                      # every rank gets whole 32-row bands
    for rank in range(world):
        inter = (32, rank, world)
        cases.assert_same_frame(cases.run_gpu(case, interleave=inter), full, rows=cases.band_rows(h, inter), stats=False,
                                what=f"{name} bands rank {rank}")


@pytest.mark.parametrize("kind_name", ["phong", "eye"])
def test_gpu_draw_indexed_equals_reference_vertex_stage_frame(kind_name):
    """draw_indexed of the fixture mesh (vertex stage on the device) gives the frame the reference's Model::load +
    shader.vertex(f, v) + rasterize() gave."""
    from tinyrenderder_amd.api import Context, PHONG, EYE
    verts, idx, u, proj, w, h = cases.fixture_mesh()
    kind = PHONG if kind_name == "phong" else EYE
    g = NEXT_ROWS["mesh"][kind_name]
    with Context(w, h, 3) as ctx:
        for slot, t in cases.edge_textures().items():
            ctx.upload_texture(slot, t)
        ctx.draw_indexed(kind, u, proj, verts, idx)
        got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line())
    cases.assert_golden(got, g, eye=kind == EYE)


@pytest.mark.parametrize("name", sorted(cases.fixture_zbuffers()))
def test_gpu_postprocess_equals_reference_zimage_and_ao(name):
    """postprocess() over the fixture z-buffers (NaN, +-inf, constant, empty, threshold steps) gives save_zbuffer_image's and
    compute_ssao_at's bytes."""
    from tinyrenderder_amd.api import Context
    z = cases.fixture_zbuffers()[name]
    g = NEXT_ROWS["zbuffers"][name]
    assert scenes.digest(z) == g["inputs"]
    h, w = z.shape
    with Context(w, h, 3) as ctx:
        ctx.write_zbuffer(z)
        out = ctx.postprocess(final=False)
    assert scenes.digest(out["zbuffer_image"]) == g["zimage"], "z-buffer image differs from save_zbuffer_image"
    assert scenes.digest(out["ao"]) == g["ao"], "AO bytes differ from compute_ssao_at"
