"""User shaders that may discard, on the GPU (include/trgl.h, TRGL_SHADER_MAY_DISCARD): their own raster kernel calls trgl_fragment for
every fragment that passes the z-test, in submission order per pixel.  A restatement of CHECKER must give the built-in kind's frame,
z bits and print_render_stats() line, and the reference binary's goldens; never-discarding restatements of FLAT, GOURAUD and PHONG
run every exactness path of the kernel against the built-in kinds; flush cuts between kinds, strips, bands, the device vertex stage
and the C++ shim are covered as well."""
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import discard_shader_sources as D
from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import Context, FLAT, GOURAUD, PHONG, CHECKER, make_uniforms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
same = cases.assert_same_frame

# built-in kind -> the (source, K, may_discard) that restates it
RESTATED = {CHECKER: (D.CHECKER, 0, True), FLAT: (D.FLAT, 0, True), GOURAUD: (D.GOURAUD, 3, True), PHONG: (D.PHONG, 24, True)}


def _user(case, kinds=(CHECKER,), **kw):
    """run_gpu with every draw of a kind in `kinds` drawn by the discarding user kind that restates it."""
    return cases.run_gpu(case, shaders=[RESTATED[d[0]] if d[0] in kinds else None for d in case["draws"]], **kw)


MODES = {"one": {}, "halves": dict(halves=True), "flush_after": dict(flush_after=0)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["checker_256", "zero_checker_discarded_first_96x64"])
def test_checker_source_equals_checker_and_golden(name):
    case = cases.CASES[name]()
    got = _user(case)
    same(got, cases.run_gpu(case), what=name)
    cases.assert_golden(got, GOLDEN[name])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_checker_source_in_mixed_scene(mode):
    """FLAT, then the user kind, then GOURAUD: flush cuts on both sides of the discarding draw, in every submission mode."""
    case = cases.checker_mixed_200x120()
    got = _user(case, **MODES[mode])
    same(got, cases.run_gpu(case, **MODES[mode]), what=mode)
    cases.assert_golden(got, GOLDEN["checker_mixed_200x120"])


FLAT_ONLY = sorted(n for n, f in cases.CASES.items() if f()["draws"] and all(d[0] == FLAT for d in f()["draws"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLAT_ONLY)
def test_never_discarding_flat_equals_flat_and_golden(name):
    """Literal path (edge_256, huge_depths_128), bpp 1, odd dimensions, a viewport offset, a finite z clear, the zero signs."""
    case = cases.CASES[name]()
    got = _user(case, kinds=(FLAT,))
    same(got, cases.run_gpu(case), what=name)
    cases.assert_golden(got, GOLDEN[name])


@pytest.mark.gpu
def test_never_discarding_gouraud_equals_gouraud_and_golden():
    case = cases.gouraud_256_rgba()
    got = _user(case, kinds=(GOURAUD,))
    same(got, cases.run_gpu(case), what="gouraud_256_rgba")
    cases.assert_golden(got, GOLDEN["gouraud_256_rgba"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["phong_512", "phong_nomaps_256"])
def test_never_discarding_phong_equals_phong(name):
    """Textures through trgl_sample2D; every z-pass is shaded, in order, and the last one stays."""
    case = cases.CASES[name]()
    same(_user(case, kinds=(PHONG,)), cases.run_gpu(case), what=name)


@pytest.mark.gpu
def test_discard_everything_leaves_the_clear():
    case = cases.checker_256()
    (_, _, clip, _, col), = case["draws"]
    case = dict(case, clear=(9, 8, 7, 255), zclear=0.75)
    fb, z, st, _ = cases.run_gpu(case, shaders=[(D.DISCARD_ALL, 0, True)])
    ref = cases.run_gpu(dict(case, draws=[(FLAT, None, clip, None, col)]))[2]
    assert (fb.reshape(-1, 3) == np.array([9, 8, 7], np.uint8)).all()
    assert (z == 0.75).all()
    assert st[1] == 0, st
    assert st[0] == ref[0] and st[2:6] == ref[2:6], (st, ref)


def _mixed(w, h, bpp, seed):
    """FLAT below, CHECKER in the middle (perspective w), GOURAUD on top, overlapping."""
    c0, k0 = scenes.random_triangles(600, w, h, seed=seed, rmin=3, rmax=40)
    c1, k1 = scenes.random_triangles(1200, w, h, seed=seed + 1, rmin=3, rmax=40, perspective_w=True)
    c2, k2 = scenes.random_triangles(400, w, h, seed=seed + 2, rmin=2, rmax=24, perspective_w=True)
    v2 = scenes.SplitMix64(seed + 3).uniform(400 * 3, 0.1, 1.2).reshape(400, 3)
    return cases.make_case(w, h, [(FLAT, None, c0, None, k0), (CHECKER, make_uniforms(cells=4), c1, None, k1),
                                  (GOURAUD, None, c2, v2, k2)], bpp=bpp, clear=(20, 30, 40, 255))


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", [3, 4])
def test_strips_and_bands_equal_whole_frame(bpp):
    w, h = 200, 192             # (the bands' period divides the height)
    case = _mixed(w, h, bpp, seed=51)
    whole = _user(case)
    same(whole, cases.run_gpu(case), what=f"bpp {bpp} whole frame")
    for strip, il in [((37, 131), None), (None, (32, 0, 2)), (None, (32, 1, 2)), (None, (64, 2, 3))]:
        got = _user(case, strip=strip, interleave=il)
        rows = strip if strip else cases.band_rows(h, il)
        same(got, whole, rows=rows, stats=False, what=f"bpp {bpp} strip {strip} bands {il}")
        same(got, cases.run_gpu(case, strip=strip, interleave=il), what=f"bpp {bpp} strip {strip} bands {il} against CHECKER")


def _five_draws(w, h):
    hd = scenes.head_standin(3, w, h, seed=7)
    d, n, s = scenes.procedural_textures(128)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.7, 0, 1, 2)
    draws = [(PHONG, u, hd["clip"], hd["varyings"], None)]
    for i, cells in enumerate((3, 5, 7)):
        c, k = scenes.random_triangles(700, w, h, seed=60 + i, rmin=3, rmax=50, perspective_w=True)
        draws.append((CHECKER, make_uniforms(cells=cells), c, None, k))
    fc, fk = scenes.random_triangles(500, w, h, seed=64, rmin=2, rmax=30)
    draws.append((FLAT, None, fc, None, fk))
    return cases.make_case(w, h, draws, textures={0: d, 1: n, 2: s})


@pytest.mark.gpu
def test_one_context_phong_user_checker_user_flat():
    """PHONG (visibility buffer + k_shade), user kind A, built-in CHECKER, user kind B, FLAT on one context: equal to the built-in
    CHECKER in both user positions.  Then A and B back to back (two discarding kinds meeting)."""
    case = _five_draws(256, 192)
    a, b = RESTATED[CHECKER], (D.CHECKER_B, 0, True)
    want = cases.run_gpu(case)
    same(cases.run_gpu(case, shaders=[None, a, None, b, None]), want, what="P A C B F")
    same(cases.run_gpu(case, shaders=[None, a, b, b, None]), want, what="P A B B F")
    same(cases.run_gpu(case, shaders=[None, a, b, a, None], halves=True), want, what="P A B A F, halves")


@pytest.mark.gpu
def test_draw_indexed_with_discarding_kind_equals_phong():
    W, H = 640, 480
    hd = scenes.head_standin(5, W, H)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    verts = np.ascontiguousarray(np.concatenate([pos, nrm, uv, np.zeros((pos.shape[0], 6))], 1))
    idx = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
    d, n, s = scenes.procedural_textures(256)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.8, 0, 1, 2)
    res = []
    for user in (False, True):
        with Context(W, H, 3) as ctx:
            kind = ctx.register_shader(*RESTATED[PHONG]) if user else PHONG
            for k, t in enumerate((d, n, s)):
                ctx.upload_texture(k, t)
            ctx.draw_indexed(kind, u, hd["projection"], verts, idx)
            res.append((ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()))
    same(res[1], res[0], what="draw_indexed")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_fuzz_discarding_user_scenes(seed):
    """Seeded scenes in the manner of test_gpu_parity's discarding fuzz: dense overdraw, perspective w, 1 - 40 cells, large and
    small triangles, a flat draw underneath (odd seeds: the same flush for CHECKER, a flush cut for the user kind) or two flushes.
    The user kind equals the built-in CHECKER, and both equal the oracle."""
    rng = scenes.SplitMix64(9500 + seed)
    u = rng.uniform(8)
    W = int(80 + u[0] * 240); H = int(80 + u[1] * 200)
    n = int(3000 + u[2] * 12000)
    cells = int(1 + u[3] * 40)
    clip, col = scenes.random_triangles(n, W, H, seed=9600 + seed, rmin=1 + 4 * u[4], rmax=10 + 150 * u[5], perspective_w=True)
    base, bcol = scenes.random_triangles(n // 3, W, H, seed=9700 + seed, rmin=3, rmax=60)
    checker = (CHECKER, make_uniforms(cells=cells), clip, None, col)
    case = cases.make_case(W, H, [(FLAT, None, base, None, bcol), checker] if seed & 1 else [checker])
    split = None if seed & 1 else 2
    got = _user(case, split=split)
    same(got, cases.run_gpu(case, split=split), what=f"seed {seed} against CHECKER")
    same(got, cases.run_oracle(case), what=f"seed {seed} against the oracle")


SHIM_CHECKER_PROGRAM = r"""
// checker_256 through the shim: rasterize() with CheckerShader, or with a UserShader registered with may_discard = true
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "trgl_shaders.h"
int main(int argc, char** argv) {     // <in.bin> <out.bin> [user_source_file]
    std::ifstream in(argv[1], std::ios::binary);
    int hd[4]; in.read(reinterpret_cast<char*>(hd), sizeof hd);
    const int W = hd[0], H = hd[1], n = hd[2], cells = hd[3];
    std::vector<double> clip(12 * size_t(n));
    std::vector<unsigned char> col(4 * size_t(n));
    in.read(reinterpret_cast<char*>(clip.data()), std::streamsize(clip.size() * 8));
    in.read(reinterpret_cast<char*>(col.data()), std::streamsize(col.size()));
    init_viewport(0, 0, W, H);
    TGAImage fb(W, H, TGAImage::RGB);
    init_zbuffer(W, H);
    int kind = -1;
    if (argc > 3) {
        std::ifstream sf(argv[3]);
        const std::string src((std::istreambuf_iterator<char>(sf)), std::istreambuf_iterator<char>());
        kind = gl_register_shader(src.c_str(), 0, true);
        if (kind < 0) { std::fprintf(stderr, "gl_register_shader: %s\n", gl_last_error_message()); return 2; }
    }
    for (int i = 0; i < n; ++i) {
        Triangle t;
        std::memcpy(&t, &clip[12 * size_t(i)], sizeof t);
        const TGAColor c(&col[4 * size_t(i)], 4);
        if (kind >= 0) {
            UserShader s(kind); s.color = c; s.uniforms.reserved = cells;
            rasterize(t, s, fb);
        } else {
            CheckerShader s; s.color = c; s.cells = cells;
            rasterize(t, s, fb);
        }
    }
    if (!gl_flush(fb)) { std::fprintf(stderr, "flush: %s\n", gl_last_error_message()); return 3; }
    print_render_stats();
    const std::vector<double>& z = zbuffer;
    std::ofstream out(argv[2], std::ios::binary);
    out.write(reinterpret_cast<const char*>(fb.buffer()), std::streamsize(size_t(W) * H * 3));
    out.write(reinterpret_cast<const char*>(z.data()), std::streamsize(z.size() * 8));
    gl_shutdown();
    return out ? 0 : 4;
}
"""


@pytest.mark.gpu
def test_shim_user_shader_equals_checker_shader(tmp_path):
    src = tmp_path / "checker.cpp"
    src.write_text(SHIM_CHECKER_PROGRAM)
    exe = str(tmp_path / "checker")
    lib = os.path.join(ROOT, "tinyrenderder_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, str(src), "-I", os.path.join(lib, "shim"),
                        "-L", lib, "-ltrgl", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    case = cases.checker_256()
    (_, u, clip, _, col), = case["draws"]
    W, H = case["width"], case["height"]
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, clip.shape[0], u.reserved], np.int32).tobytes())
        f.write(np.ascontiguousarray(clip, np.float64).tobytes() + np.ascontiguousarray(col, np.uint32).tobytes())
    (tmp_path / "checker.hip").write_text(D.CHECKER)
    res = {}
    for mode, extra in (("builtin", []), ("user", [str(tmp_path / "checker.hip")])):
        out = tmp_path / f"{mode}.bin"
        p = subprocess.run([exe, str(inp), str(out)] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        res[mode] = (out.read_bytes(), [ln for ln in p.stderr.splitlines() if ln.startswith("DEBUG:")])
    assert len(res["builtin"][0]) == W * H * 11
    assert res["user"][0] == res["builtin"][0], "framebuffer or z-buffer differs"
    assert res["user"][1] == res["builtin"][1] == [GOLDEN["checker_256"]["stats"]]
