"""Call sequences on the GPU against the immediate-mode model (tests/call_programs.py): one program per (family, seed), one context
each.  Every observation a program asks for - z bits, framebuffer bytes, the stats tuple and line, post-process images, mesh bounds -
equals the model's; in family E, after the first EYE draw, framebuffer bytes by the EYE rule of cases.assert_same_frame.
Families T, P and I add the observations of registers (occlusion codes, shadow masks, instance boxes, depths, orders) and of stage
rows with their counts, all bit for bit.
tests/test_call_programs.py shows on the model alone which host rules of csrc/trgl_api.cpp these programs put to work."""
import pytest

import call_programs as cp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family,seed", [(f, s) for f in cp.FAMILIES for s in cp.SEEDS[f]])
def test_program(family, seed):
    program = cp.generate(family, seed)
    cp.assert_same(program, cp.run_gpu(program), cp.run_model(program))
