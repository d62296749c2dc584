"""CPU tests of the oracle (oracle/trgl_oracle.c) against the golden vectors in tests/golden/, which were
produced by the reference's own rasterize() (tests/golden/make_golden.py).  No GPU, no reference tree needed."""
import json
import os

import numpy as np
import pytest

import cases
from oracle import orc
from tinyrenderder_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))


def _input_digest(case):
    parts = [np.asarray(case["viewport"], np.float64)]
    for kind, u, clip, vary, col in case["draws"]:
        parts.append(np.frombuffer(bytes(u), np.uint8) if u is not None else np.zeros(1, np.uint8))
        parts += [clip] + ([vary] if vary is not None else []) + ([col] if col is not None else [])
    for slot in sorted(case["textures"]):
        parts.append(case["textures"][slot])
    return scenes.digest(np.concatenate([np.ascontiguousarray(p).view(np.uint8).ravel() for p in parts]))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_oracle_matches_reference_golden(name):
    case = cases.CASES[name]()
    g = GOLDEN[name]
    assert _input_digest(case) == g["inputs"], "scene generator drifted: inputs differ from the ones the reference saw"
    fb, z, st = cases.run_oracle(case)
    assert orc.format_stats_line(st) == g["stats"]
    assert scenes.digest(z) == g["z"], "z-buffer bits differ from the reference"
    assert scenes.digest(fb) == g["fb"], "framebuffer bytes differ from the reference"


@pytest.mark.parametrize("name", cases.FULL_BUFFER_CASES)
def test_oracle_full_buffers(name):
    ref = np.load(os.path.join(HERE, "golden", name + ".npz"))
    fb, z, _ = cases.run_oracle(cases.CASES[name]())
    assert np.array_equal(fb, ref["fb"])
    assert np.array_equal(z.view(np.uint64), ref["z"].view(np.uint64))


def test_oracle_strips_compose():
    """Rows are independent: rendering two strips separately equals the whole (basis of the multi-GPU shard)."""
    case = cases.CASES["flat_persp_512"]()
    fb, z, st = cases.run_oracle(case)
    h = case["height"]
    cut = 200                                  # not a multiple of the tile size on purpose
    fb0, z0, s0 = cases.run_oracle(case, strip=(0, cut))
    fb1, z1, s1 = cases.run_oracle(case, strip=(cut, h))
    assert np.array_equal(np.concatenate([fb0[:cut], fb1[cut:]]), fb)
    assert np.array_equal(np.concatenate([z0[:cut], z1[cut:]]).view(np.uint64), z.view(np.uint64))
    assert s0[1] + s1[1] == st[1]                                  # fragments_drawn adds up
    assert min(s0[6], s1[6]) == st[6] and max(s0[7], s1[7]) == st[7]
    assert s0[2:6] == st[2:6] and s1[2:6] == st[2:6]               # bbox stats come from triangles, not pixels


def test_x86_cast_edge_cases_are_in_the_golden_scene():
    """edge_256 holds a vertex whose screen coordinate overflows int: the reference (cvttsd2si) drops it."""
    clip, _ = scenes.edge_case_triangles(256, 256)
    assert abs(clip[25, 0] / clip[25, 3]) * 128 > 2 ** 31


def test_value_ops_match_reference_geometry_h():
    """normalized(), mat*vec4, varying interpolation and TGAColor*float of the restatement vs the real
    geometry.h / tgaimage.h (fixtures tests/golden/make_vecops_golden.py took through oracle/_ref/ref_harness vecops)."""
    import ctypes as C
    data, packed = cases.vecops_inputs()
    n = data.shape[0]
    g = np.load(os.path.join(HERE, "golden", "vecops_golden.npz"))
    assert str(g["inputs"]) == scenes.digest(data) + scenes.digest(packed), "inputs differ from the ones the reference saw"
    ref_d = g["d"].view(np.float64)
    ref_c = g["c"]
    L = orc.lib()
    for i in range(n):
        v, nn, M = data[i, 0:3].copy(), data[i, 3:6].copy(), data[i, 6:22].copy()
        v0, v1, v2, b = (data[i, 22 + 3 * k: 25 + 3 * k].copy() for k in range(4))
        o = np.empty(9)
        L.orc_normalized3(v.ctypes.data, o[0:3].ctypes.data)
        tmp = np.empty(3); L.orc_mat4_mul_dir(M.ctypes.data, nn.ctypes.data, tmp.ctypes.data); o[3:6] = tmp
        tmp2 = np.empty(3); L.orc_interp(v0.ctypes.data, v1.ctypes.data, v2.ctypes.data, b.ctypes.data, 3, tmp2.ctypes.data); o[6:9] = tmp2
        assert np.array_equal(o.view(np.uint64), ref_d[i].view(np.uint64)), i
        out = (C.c_uint8 * 4)()
        inten = np.array([data[i, 34]] * 3)
        bary = (C.c_double * 3)(1.0, 0.0, 0.0)
        L.orc_fragment(orc.GOURAUD, None, None, inten.ctypes.data, int(packed[i]), bary, out)
        assert bytes(out) == bytes(ref_c[i]), i


# ---- samplers: index math pinned by the reference's compiled IShader::sample2D (our_gl.h:38-44) ----------------------------------
SAMPLER_GOLDEN = np.load(os.path.join(HERE, "golden", "sampler_golden.npz"))


@pytest.mark.parametrize("i", range(5))
def test_sampler_restatement_equals_reference_sample2d(i):
    """orc tex_fetch (model.cpp:415-425 restated) vs the fixtures tests/golden/make_sampler_golden.py took from the compiled
    reference: NaN, +-inf, negatives, exactly 1.0, 1e300, values beyond INT_MAX after scaling, every texel boundary +- 1 ulp,
    textures of 1 / 3 / 4 bytes per pixel, 1x1 and odd sizes."""
    tex, uv, want = SAMPLER_GOLDEN[f"tex{i}"], SAMPLER_GOLDEN[f"uv{i}"].view(np.float64), SAMPLER_GOLDEN[f"out{i}"]
    got = orc.tex_fetch(tex, uv)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, f"{len(bad)} samples differ, first uv {uv[bad[0, 0]]}"
