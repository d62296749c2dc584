"""What the stage entry points (csrc/trgl_stage_*.cpp) answer to bad calls, and which of two faults wins: every call of
tests/stage_call_cases.py must return the code and leave the trgl_last_error text that tests/golden/stage_call_errors.json records
(make_stage_call_errors.py, from the commit before the entry points were split by family), and every valid baseline at the smallest
shape must compute what the host models compute.

The first part runs with c = NULL and needs no GPU; the gpu part covers what needs a context: every trgl_draw_* entry point, the
stage calls that work through device buffers, and device memory kinds in calls that a check refuses before anything is allocated or
launched (their device pointers are real small allocations, offset where the case is about alignment)."""
import json
import os

import numpy as np
import pytest

import clip_model
import instance_model
import order_model
import skin_model
import sprite_model
import stage_call_cases as SC
import triangle_order_model
from tinyrenderder_amd import api

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_call_errors.json")))
E_INVALID = -1


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{what}: {got} != {want}"


def _params(P):
    return {name: (list(getattr(P, name)) if hasattr(getattr(P, name), "__len__") else getattr(P, name)) for name, _ in P._fields_}


def _check_answers(part, results):
    assert set(results) == set(GOLDEN[part]), "the table and the recorded file name different cases: record the new ones from the parent commit"
    wrong = {k: (v, GOLDEN[part][k]) for k, v in results.items() if v != GOLDEN[part][k]}
    assert not wrong, "\n".join(f"{k}: got {v}, recorded {g}" for k, (v, g) in wrong.items())


@pytest.fixture(scope="module")
def host_part():
    return SC.run_host_part(api.load_library())


def test_every_host_call_answers_as_recorded(host_part):
    _check_answers("host", host_part[0])
    # the table holds what it claims: faults are refused, baselines run, and the order-pinning cases say what they pin
    g = GOLDEN["host"]
    assert all((rc == 0) == (text == "") for rc, text in g.values() if text is not None)
    assert all(g[SC.case_id(e, None)][0] == (E_INVALID if needs_ctx else 0) for e, (needs_ctx, _) in SC.BASELINES.items())
    assert g["trgl_sprite_stage:n0_and_bad_mode"][0] == E_INVALID and g["trgl_sprite_stage:n0"][0] == 0
    assert g["trgl_order_stage:bad_mem_and_negative_K"][1].endswith("bad mem_kind")
    assert g["trgl_clip_stage:device_without_context_and_null_plane"][1].endswith("needs a context")


def test_host_baselines_compute_what_the_models_compute(host_part):
    b = host_part[1]
    a = b["trgl_sprite_stage"]
    want = sprite_model.sprites(_params(a["P"]), a["points"], a["colors"])
    _same(a["clip_out"], want[0], "sprite clip"); _same(a["vary_out"], want[1], "sprite varyings")
    assert np.array_equal(a["colors_out"], want[2])
    a = b["trgl_line_stage"]
    want = sprite_model.lines(_params(a["P"]), a["points"], a["indices"], a["colors"])
    _same(a["clip_out"], want[0], "line clip"); _same(a["vary_out"], want[1], "line varyings")
    assert np.array_equal(a["colors_out"], want[2]) and np.any(want[0])
    a = b["trgl_skin_stage"]
    _same(a["out"], skin_model.skin(a["vertices"], a["joints"], a["weights"], a["palette"].reshape(1, 1, 16))[0], "skinned")
    assert a["out"].tolist() == [[-0.25, 0.0, 0.0]]
    a = b["trgl_pose_palette"]
    _same(a["palette"].reshape(1, 1, 16), skin_model.pose_palette(a["parents"], a["local"].reshape(1, 1, 16), a["inverse_bind"].reshape(1, 16)), "palette")
    a = b["trgl_triangle_depths"]
    _same(a["depths_out"], triangle_order_model.depths(a["clip"], 1, triangle_order_model.CENTROID), "triangle depths")
    a = b["trgl_order_stage"]
    want = triangle_order_model.gather(a["clip"], a["vary"], a["colors"], a["order"], 1)
    _same(a["clip_out"], want[0], "ordered clip"); _same(a["vary_out"], want[1], "ordered varyings")
    assert np.array_equal(a["colors_out"], want[2])
    a = b["trgl_clip_stage"]
    want = clip_model.clip_model(a["plane"], a["clip"], None, a["colors"])
    m = a["n_out"].value
    assert m == len(want[0]) == 2, "the plane cuts one corner off: two triangles"
    _same(a["clip_out"][:m], want[0], "clipped"); assert np.array_equal(a["colors_out"][:m], want[2])
    a = b["trgl_instance_depths"]
    _same(a["depths_out"], order_model.depths(a["model_view"], a["point"], a["instances"]), "instance depths")
    assert a["depths_out"][0] == -2.0
    a = b["trgl_depth_order"]
    assert np.array_equal(a["order_out"], order_model.order(a["depths"]))


@pytest.mark.gpu
def test_every_call_on_a_context_answers_as_recorded():
    results, b, frames = SC.run_context_part(api.load_library())
    _check_answers("context", results)
    g = GOLDEN["context"]
    assert all((rc == 0) == (text == "") for rc, text in g.values())
    assert all(g[SC.case_id(e, None)][0] == 0 for e, (needs_ctx, _) in SC.BASELINES.items() if needs_ctx)
    assert all(g[SC.case_id(e, f)][0] != 0 for e, f in SC.cases(True) if SC.uses_device(SC.arguments(e, f))), "a call with device pointers ran"
    assert g["trgl_draw_clipped:n0_and_bad_mem"][0] == 0 and g["trgl_draw_clipped:bad_mem"][1].endswith("bad mem_kind")
    assert g["trgl_draw_ordered:null_list_group_0"][0] == 0, "a null list falls through to trgl_draw"
    assert g["trgl_draw_skinned:two_poses_and_colors_without_shader"][1].endswith("n_poses must be 1")
    assert g["trgl_draw_indexed:no_faces_and_index_out_of_range"][0] == 0
    assert g["trgl_instance_stage:nothing_to_run_and_null_n_out"][1].endswith("n_out is null")
    # every draw's baseline left fragments behind, and the stages that work through device buffers equal the models
    assert sorted(frames) == sorted(e for e in SC.BASELINES if "_draw_" in e)
    assert all(np.isfinite(z).any() for z in frames.values()), [e for e, z in frames.items() if not np.isfinite(z).any()]
    v, idx = SC.mesh()
    want = instance_model.builtin_rows(SC.EYE4, SC.EYE4, v, idx, SC.move(0.0))
    for entry in ("trgl_vertex_stage", "trgl_instance_stage", "trgl_instance_stage_ordered"):
        _same(b[entry]["clip_out"], want[0], entry + " clip"); _same(b[entry]["vary_out"], want[1], entry + " varyings")
        assert entry == "trgl_vertex_stage" or b[entry]["n_out"].value == 1
