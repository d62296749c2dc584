"""The shim's deferred rasterize() on the GPU against the immediate-mode model (tests/shim_programs.py): one process of the driver
(tests/host/shim_program.cpp, built by examples/Makefile) per program, through the shim's public names alone.  Every observation a
program asks for - the bytes of a TGAImage behind gl_flush() and as the caller holds it, the depths the `zbuffer` proxy hands out
element by element, as a copy and in a range-for, its size, the line print_render_stats() prints, the kind a registered user shader
gets, gl_last_error() and its message at the end - equals the model's, bit for bit.
tests/test_shim_programs.py shows on the model alone which rules of tinyrenderder_amd/shim/trgl_gl.h these programs put to work.
The programs of shim_programs.B64 run a second time in the driver built with TRGL_SHIM_BATCH_TRIS=64, where rasterize() cuts its
batch by size inside their runs."""
import os
import subprocess

import pytest

import call_programs as cp
import shim_programs as sp

pytestmark = pytest.mark.gpu

DRIVERS = {"": os.path.join(cp.ROOT, "examples", "shim_program"), "b64": os.path.join(cp.ROOT, "examples", "shim_program_b64")}


@pytest.mark.parametrize("name,driver", [(n, "") for n in sp.PROGRAMS] + [(n, "b64") for n in sp.B64])
def test_program(name, driver, tmp_path):
    program = sp.PROGRAMS[name]
    want = sp.run_model(program)
    src, out = tmp_path / "program.bin", tmp_path / "observations.bin"
    src.write_bytes(sp.encode(program))
    run = subprocess.run([DRIVERS[driver], str(src), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    sp.assert_same(program, sp.decode(program, out.read_bytes(), run.stderr), want)
