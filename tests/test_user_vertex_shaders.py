"""User vertex shaders without a GPU (include/trgl.h, "User vertex shaders"): the exported symbols, run-time compilation and its
errors, the code cache (a vertex program and a fragment program with the same text are two entries), the binding's device-pointer
guard, and the shim's C++ surface."""
import ctypes
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

import user_shader_sources as S
import vertex_shader_sources as V
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tinyrenderder_amd", "csrc")
E_INVALID = -1
NEW_SYMBOLS = ("trgl_vertex_shader_compile", "trgl_register_vertex_shader", "trgl_draw_indexed_vs", "trgl_vertex_stage")


def _compile(src, k):
    L = api.load_library()
    log = ctypes.create_string_buffer(16384)
    return L.trgl_vertex_shader_compile(src.encode(), k, log, len(log)), log.value.decode()


def test_library_exports_the_four_entry_points():
    lib = ctypes.CDLL(api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.SYMBOLS
    assert api.MAX_USER_VERTEX_SHADERS == 32


@pytest.mark.parametrize("name,src,k", [("restated", V.RESTATED, 24), ("gouraud", V.GOURAUD, 3), ("gouraud5", V.GOURAUD_PADDED, 5),
                                        ("transform", V.TRANSFORM, 0), ("wide", V.WIDE, 64), ("arguments", V.ARGUMENTS, 6)])
def test_valid_sources_compile(name, src, k):
    rc, log = _compile(src, k)
    assert rc == 0, log
    assert api.vertex_shader_compile(src, k) == (True, log)


def test_second_compile_comes_from_the_cache():
    """A text no earlier test compiled: the first call runs the compiler, the second finds the code object (and hands back the
    log of the compilation, its warning included)."""
    src = f"#warning trgl-vertex-cached-warning\n// {time.time_ns()}\n" + V.GOURAUD
    t0 = time.perf_counter(); first = api.vertex_shader_compile(src, 3)
    t1 = time.perf_counter(); second = api.vertex_shader_compile(src, 3)
    t2 = time.perf_counter()
    assert first[0] and "trgl-vertex-cached-warning" in first[1]
    assert second == first
    assert t2 - t1 < (t1 - t0) / 4, (t1 - t0, t2 - t1)


def test_source_without_trgl_vertex_is_refused():
    rc, log = _compile("__device__ void my_vertex(const trgl_vert_in& in, trgl_vert_out& out) { out.clip[0] = in.vertex[0]; }\n", 0)
    assert rc == E_INVALID
    assert "trgl_vertex" in log and "error" in log
    assert "trgl_vertex_shader_compile" in api.load_library().trgl_last_error(None).decode()


def test_wrong_signature_is_refused():
    rc, log = _compile("__device__ int trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) { return in.nth; }\n", 0)
    assert rc == E_INVALID
    assert "trgl_vertex must be declared as" in log


def test_syntax_error_names_the_line():
    src = "__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {\n    out.clip[0] = in.vertex[0]\n}\n"
    rc, log = _compile(src, 0)
    assert rc == E_INVALID
    assert re.search(r"user_shader:2:\d+: error", log), log


@pytest.mark.parametrize("k", [-1, api.MAX_USER_VARY + 1])
def test_varyings_out_of_range_are_refused(k):
    rc, log = _compile(V.TRANSFORM, k)
    assert rc == E_INVALID
    assert "n_varyings" in log


def test_vertex_and_fragment_programs_with_the_same_text_do_not_collide():
    """One text, compiled for both stages: each stage compiles it behind its own kernel, so a text that only defines the other
    stage's function is a compile error - it would be `ok` if the cache handed back the other stage's code object."""
    assert api.shader_compile(S.FLAT, 0)[0]                      # a fragment program, now cached
    rc, log = _compile(S.FLAT, 0)                                # the same text as a vertex program
    assert rc == E_INVALID and "trgl_vertex" in log
    assert api.vertex_shader_compile(V.TRANSFORM, 0)[0]          # a vertex program, now cached
    ok, log = api.shader_compile(V.TRANSFORM, 0)                 # the same text as a fragment program
    assert not ok and "trgl_fragment" in log
    both = S.FLAT + V.TRANSFORM                                  # valid for both: two entries, both still fine afterwards
    assert api.shader_compile(both, 0)[0] and api.vertex_shader_compile(both, 0)[0]
    assert api.shader_compile(both, 0)[0] and api.vertex_shader_compile(both, 0)[0]


def test_template_compiles_on_its_own(tmp_path):
    """vertex_user.h behind a source in an ordinary hipcc build with the library's flags and -Wall -Werror, at K = 0, 3 and 64; the
    kernel keeps to LDS and 16-byte global stores and needs no scratch memory."""
    for k, body in ((0, V.TRANSFORM), (3, V.GOURAUD), (64, V.WIDE)):
        src = tmp_path / f"vs{k}.hip"
        src.write_text(f'#include <hip/hip_runtime.h>\n#include "user_prelude.h"\n#define TRGL_USER_VARY {k}\n{body}\n#include "vertex_user.h"\n')
        asm = tmp_path / f"vs{k}.s"
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                            "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Werror", "-Wno-unused-command-line-argument", "-I", CSRC,
                            "--cuda-device-only", "-S", "-o", str(asm), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        text = asm.read_text()
        assert "global_store_dwordx4" in text and "ds_write_b128" in text and "ds_read_b128" in text
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", text), "the kernel spills"
        assert not re.search(r"^\s+(flat_|scratch_)", text, flags=re.M), "LDS rows are reached through flat or scratch accesses"


class _FakeCuda:
    """What the guard looks at in a torch CUDA tensor."""
    is_cuda = True
    shape = (6, 8)

    def data_ptr(self):
        return 0x7F0000001000


class _Recorder:
    """Stands in for the loaded library: any call is recorded (and would 'succeed')."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


def _context(lib):
    ctx = object.__new__(api.Context)
    ctx.L, ctx.h, ctx._keep, ctx._user_vary, ctx._vertex_vary = lib, None, [], {}, {0: 3}
    return ctx


@pytest.mark.parametrize("which", ["vertices", "indices", "colors"])
def test_draw_indexed_with_a_vertex_shader_refuses_host_arrays_before_the_library_is_called(which):
    lib = _Recorder()
    ctx = _context(lib)
    args = dict(vertices=_FakeCuda(), indices=_FakeCuda(), colors=_FakeCuda())
    for bad in (np.zeros((6, 8)), torch.zeros(6, 8, dtype=torch.float64)):
        with pytest.raises(TypeError, match=which):
            ctx.draw_indexed(api.GOURAUD, None, np.eye(4), device=True, vertex_shader=0, **dict(args, **{which: bad}))
    assert lib.calls == [] and ctx._keep == []
    ctx.draw_indexed(api.GOURAUD, None, np.eye(4), device=True, vertex_shader=0, **args)
    assert lib.calls == ["trgl_draw_indexed_vs"] and len(ctx._keep) == 1


@pytest.mark.parametrize("which", ["vertices", "indices", "clip", "varyings"])
def test_vertex_stage_refuses_host_arrays_before_the_library_is_called(which):
    lib = _Recorder()
    ctx = _context(lib)
    args = dict(vertices=_FakeCuda(), indices=_FakeCuda(), clip=_FakeCuda(), varyings=_FakeCuda())
    for bad in (np.zeros((6, 8)), torch.zeros(6, 8, dtype=torch.float64)):
        a = dict(args, **{which: bad})
        with pytest.raises(TypeError, match=which):
            ctx.vertex_stage(0, None, np.eye(4), a["vertices"], a["indices"], device=True, out=(a["clip"], a["varyings"]))
    assert lib.calls == [] and ctx._keep == []
    ctx.vertex_stage(0, None, np.eye(4), args["vertices"], args["indices"], device=True, out=(args["clip"], args["varyings"]))
    assert lib.calls == ["trgl_vertex_stage"]


def test_default_draw_indexed_still_calls_trgl_draw_indexed():
    lib = _Recorder()
    ctx = _context(lib)
    ctx.draw_indexed(api.PHONG, api.make_uniforms(), np.eye(4), np.zeros((3, 8)), np.arange(3, dtype=np.uint32).reshape(1, 3))
    assert lib.calls == ["trgl_draw_indexed"]


def test_shim_vertex_shader_compiles(tmp_path):
    """A translation unit that uses gl_register_vertex_shader and UserShader::vertex_kind with a built-in kind (g++, compile only)."""
    src = tmp_path / "user.cpp"
    src.write_text('#include "trgl_shaders.h"\n'
                   "struct Vtx { double p[3], n[3], uv[2]; };\n"
                   "struct Model { std::vector<Vtx> vertices; std::vector<unsigned int> indices; };\n"
                   "int main() {\n"
                   "    const int vs = gl_register_vertex_shader(\"__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) { out.vary[in.nth] = 1.0; }\", 3);\n"
                   "    UserShader s(TRGL_SHADER_GOURAUD); s.vertex_kind = vs; s.color = TGAColor(1, 2, 3);\n"
                   "    trgl_shader_desc d; if (!s.describe(d) || d.vertex_kind != vs) return 2;\n"
                   "    TGAImage fb(16, 16, TGAImage::RGB); Model m;\n"
                   "    const bool ok = vs >= 0 && gl_draw_model(m, s, fb);\n"
                   "    return gl_flush(fb) && ok ? 0 : 1;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tinyrenderder_amd", "shim"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_keeps_the_vertex_interface_in_comments():
    text = open(os.path.join(ROOT, "include", "trgl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("trgl_vert_in", "trgl_vert_out", "TRGL_USER_VARY"):
        assert word in text and word not in code
    assert re.search(r"\btrgl_vertex\(", text) and not re.search(r"\btrgl_vertex\(", code)
    for name in NEW_SYMBOLS:                       # each entry point cites the interface it replaces
        at = text.index(f"int {name}(")
        comment = text[text.rindex("/*", 0, at):at]
        assert "our_gl.h:36-52" in comment and "main.cpp:660-666" in comment, name
    assert "#define TRGL_MAX_USER_VERTEX_SHADERS 32" in code
