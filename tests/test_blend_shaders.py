"""User shaders that blend, without a GPU (include/trgl.h, TRGL_SHADER_READS_DEST and TRGL_SHADER_NO_DEPTH_WRITE): which flag words
compile, the defines ahead of the source, the cache, the prelude's blend function and the shim's C++ surface."""
import ctypes
import os
import subprocess

import pytest

import blend_model as B
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tinyrenderder_amd", "csrc")
E_INVALID = -1
SOURCES = [B.OVER_SRC, B.ALPHA_TEST_SRC, B.ADD_SRC, B.ODD_DISCARD_SRC, B.PROBE_BPP3_SRC, B.PROBE_BPP1_SRC]


def _compile(src, k, flags):
    L = api.load_library()
    log = ctypes.create_string_buffer(16384)
    return L.trgl_shader_compile_ex(src.encode(), k, flags, log, len(log)), log.value.decode()


def test_flag_values():
    assert (api.SHADER_MAY_DISCARD, api.SHADER_READS_DEST, api.SHADER_NO_DEPTH_WRITE) == (1, 4, 8)
    header = open(os.path.join(ROOT, "include", "trgl.h")).read()
    assert "#define TRGL_SHADER_READS_DEST     4u" in header and "#define TRGL_SHADER_NO_DEPTH_WRITE 8u" in header


@pytest.mark.parametrize("flags", [5, 9, 13])
@pytest.mark.parametrize("src", SOURCES)
def test_blending_flag_words_compile(src, flags):
    rc, log = _compile(src, 0, flags)
    assert rc == 0, log
    assert api.shader_compile(src, 0, True, reads_dest=bool(flags & 4), depth_write=not flags & 8) == (True, log)


@pytest.mark.parametrize("flags", [4, 8, 12])
def test_blending_flags_without_may_discard_are_refused(flags):
    rc, log = _compile(B.OVER_SRC, 0, flags)
    assert rc == E_INVALID
    assert "flag" in log
    assert "trgl_shader_compile" in api.load_library().trgl_last_error(None).decode()
    rc, log = _compile(B.PORTABLE_SRC, 0, flags)             # (a source that would compile under the plain contract as well)
    assert rc == E_INVALID and "flag" in log
    assert api.shader_compile(B.PORTABLE_SRC, 0, False, reads_dest=bool(flags & 4), depth_write=not flags & 8)[0] is False


@pytest.mark.parametrize("flags", [0, 1, 5, 9, 13])
def test_a_source_that_reads_dst_compiles_under_every_contract(flags):
    """in.dst is a member of trgl_frag_in with and without TRGL_SHADER_READS_DEST, under both signatures."""
    rc, log = _compile(B.PORTABLE_SRC, 0, flags)
    assert rc == 0, log


def test_positional_calls_keep_their_meaning():
    assert api.shader_flags() == 0 and api.shader_flags(True) == 1
    assert api.shader_flags(True, reads_dest=True) == 5 and api.shader_flags(True, depth_write=False) == 9
    assert api.shader_flags(True, True, False) == 13
    assert api.shader_compile(B.PORTABLE_SRC, 0)[0] and api.shader_compile(B.PORTABLE_SRC, 0, True)[0]
    with pytest.raises(TypeError):
        api.shader_compile(B.OVER_SRC, 0, True, True)       # reads_dest and depth_write are keyword-only


DEFINES_SRC = r"""
#if TRGL_USER_READS_DEST
#warning trgl-test-reads-dest-1
#else
#warning trgl-test-reads-dest-0
#endif
#if TRGL_USER_DEPTH_WRITE
#warning trgl-test-depth-write-1
#else
#warning trgl-test-depth-write-0
#endif
#if TRGL_USER_MAY_DISCARD
__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in) { return trgl_frag_out{ false, in.color }; }
#else
__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color; }
#endif
"""


def test_each_flag_word_is_its_own_program_with_its_own_defines():
    """TRGL_USER_READS_DEST and TRGL_USER_DEPTH_WRITE are defined to 0 or 1 ahead of every fragment source, and the cache keeps the
    five valid flag words apart: each request gets the log of its own compilation, the second time round as well."""
    words = {0: (0, 1), 1: (0, 1), 5: (1, 1), 9: (0, 0), 13: (1, 0)}
    first = {f: _compile(DEFINES_SRC, 0, f) for f in words}
    for f, (rd, dw) in words.items():
        rc, log = first[f]
        assert rc == 0, log
        assert f"trgl-test-reads-dest-{rd}" in log and f"trgl-test-reads-dest-{1 - rd}" not in log, (f, log)
        assert f"trgl-test-depth-write-{dw}" in log and f"trgl-test-depth-write-{1 - dw}" not in log, (f, log)
    for f in reversed(list(words)):
        assert _compile(DEFINES_SRC, 0, f) == first[f]


def test_prelude_blend_over_compiles_on_its_own(tmp_path):
    """user_prelude.h in an ordinary hipcc build with the library's flags: trgl_blend_over over in.dst."""
    src = tmp_path / "prelude.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "user_prelude.h"\n'
                   "__global__ void k(trgl_frag_in in, uint32_t* out) { out[0] = trgl_blend_over(in.color, in.dst); }\n")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-I", CSRC, "-c", "-o", str(tmp_path / "p.o"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_register_shader_flags_compiles(tmp_path):
    """A translation unit that registers a blending kind through the shim and draws it with UserShader (g++, compile only)."""
    src = tmp_path / "user.cpp"
    src.write_text('#include "trgl_shaders.h"\n'
                   "int main() {\n"
                   "    const int kind = gl_register_shader_flags(\"__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in)"
                   " { return trgl_frag_out{ false, trgl_blend_over(in.color, in.dst) }; }\", 0,"
                   " TRGL_SHADER_MAY_DISCARD | TRGL_SHADER_READS_DEST | TRGL_SHADER_NO_DEPTH_WRITE);\n"
                   "    const int plain = gl_register_shader(\"__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color; }\", 0);\n"
                   "    UserShader s(kind), p(plain); s.color = TGAColor(1, 2, 3, 128);\n"
                   "    TGAImage fb(16, 16, TGAImage::RGB); Triangle t{};\n"
                   "    if (kind >= TRGL_SHADER_USER_FIRST) { rasterize(t, p, fb); rasterize(t, s, fb); }\n"
                   "    return gl_flush(fb) ? 0 : 1;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tinyrenderder_amd", "shim"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
