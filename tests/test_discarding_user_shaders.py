"""User shaders that may discard, without a GPU (include/trgl.h, TRGL_SHADER_MAY_DISCARD): run-time compilation under the flag,
sources of the wrong contract, unknown flags, the cache, the prelude and the shim's C++ surface."""
import ctypes
import os
import subprocess

import pytest

import discard_shader_sources as D
import user_shader_sources as S
from tinyrenderder_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tinyrenderder_amd", "csrc")
E_INVALID = -1


def _compile(src, k, flags):
    L = api.load_library()
    log = ctypes.create_string_buffer(16384)
    return L.trgl_shader_compile_ex(src.encode(), k, flags, log, len(log)), log.value.decode()


@pytest.mark.parametrize("name,src,k", [("checker", D.CHECKER, 0), ("checker_b", D.CHECKER_B, 0), ("discard_all", D.DISCARD_ALL, 0),
                                        ("flat", D.FLAT, 0), ("gouraud", D.GOURAUD, 3), ("phong", D.PHONG, 24)])
def test_discarding_sources_compile(name, src, k):
    rc, log = _compile(src, k, api.SHADER_MAY_DISCARD)
    assert rc == 0, log
    assert api.shader_compile(src, k, may_discard=True) == (True, log)


@pytest.mark.parametrize("src,flags", [(S.FLAT, api.SHADER_MAY_DISCARD), (S.PHONG, api.SHADER_MAY_DISCARD), (D.CHECKER, 0),
                                       (D.FLAT, 0)])
def test_source_of_the_other_contract_is_refused(src, flags):
    rc, log = _compile(src, 24 if "in.vary + 6" in src else 0, flags)
    assert rc == E_INVALID
    assert "trgl_fragment" in log and "error" in log
    assert api.shader_compile(src, 24 if "in.vary + 6" in src else 0, may_discard=bool(flags))[0] is False


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xffffffff])
def test_unknown_flag_bits_are_refused(flags):
    rc, log = _compile(D.CHECKER, 0, flags)
    assert rc == E_INVALID
    assert "flag" in log
    assert "trgl_shader_compile" in api.load_library().trgl_last_error(None).decode()


def test_plain_calls_are_the_calls_without_flags():
    L = api.load_library()
    log = ctypes.create_string_buffer(16384)
    assert L.trgl_shader_compile(D.CHECKER.encode(), 0, log, len(log)) == E_INVALID
    assert "trgl_fragment" in log.value.decode()
    assert L.trgl_shader_compile(S.FLAT.encode(), 0, log, len(log)) == 0


def test_same_source_with_and_without_the_flag_is_two_cache_entries():
    """One source that serves both contracts compiles to two programs; each compilation keeps its own log in the cache (a key
    without the flags would hand the second request the first one's code object and warning)."""
    first = _compile(D.BOTH_CONTRACTS, 0, api.SHADER_MAY_DISCARD)
    plain = _compile(D.BOTH_CONTRACTS, 0, 0)
    again = _compile(D.BOTH_CONTRACTS, 0, api.SHADER_MAY_DISCARD)
    assert first[0] == 0 and plain[0] == 0
    assert "trgl-test-discarding-contract" in first[1] and "trgl-test-plain-contract" not in first[1]
    assert "trgl-test-plain-contract" in plain[1] and "trgl-test-discarding-contract" not in plain[1]
    assert again == first


def test_prelude_with_frag_out_compiles_on_its_own(tmp_path):
    """user_prelude.h in an ordinary hipcc build with the library's flags: trgl_frag_out next to trgl_frag_in and trgl_sample2D."""
    src = tmp_path / "prelude.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "user_prelude.h"\n'
                   "__global__ void k(trgl_frag_in in, uint32_t* out) { double uv[2] = { in.bar[0], in.bar[1] };"
                   " trgl_frag_out o{ in.bar[2] < 0.5, trgl_sample2D(in, in.u->tex_diffuse, uv).bgra };"
                   " if (!o.discard) out[0] = o.bgra; }\n")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-I", CSRC, "-c", "-o", str(tmp_path / "p.o"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_discarding_user_shader_compiles(tmp_path):
    """A translation unit that registers a shader that may discard through the shim and draws it with UserShader (g++, compile only)."""
    src = tmp_path / "user.cpp"
    src.write_text('#include "trgl_shaders.h"\n'
                   "int main() {\n"
                   "    const int kind = gl_register_shader(\"__device__ trgl_frag_out trgl_fragment(const trgl_frag_in& in)"
                   " { return trgl_frag_out{ in.bar[0] < 0.5, in.color }; }\", 0, true);\n"
                   "    const int plain = gl_register_shader(\"__device__ uint32_t trgl_fragment(const trgl_frag_in& in) { return in.color; }\", 0);\n"
                   "    UserShader s(kind), p(plain); s.color = TGAColor(1, 2, 3);\n"
                   "    TGAImage fb(16, 16, TGAImage::RGB); Triangle t{};\n"
                   "    if (kind >= TRGL_SHADER_USER_FIRST) { rasterize(t, s, fb); rasterize(t, p, fb); }\n"
                   "    return gl_flush(fb) ? 0 : 1;\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "tinyrenderder_amd", "shim"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
