"""Child process of test_stage_outputs_gpu.py::test_no_list_entry_is_a_foreign_word_in_the_diagnostic_build: the scenario of
test_raster_paths.py::test_short_tile_lists_after_a_large_frame against the diagnostic library (TRGL_LIB names it), whose k_raster
counts the list entries that are no triangle of the flush.  Exit status 0 = counters 9 and 10 stayed 0 and every frame equals the oracle."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import cases  # noqa: E402
from test_raster_paths import _tile_lists_scene  # noqa: E402
from tinyrenderder_amd import scenes  # noqa: E402
from tinyrenderder_amd.api import Context, FLAT  # noqa: E402


def main():
    assert "dbg" in os.path.basename(os.environ["TRGL_LIB"])
    W = H = 256
    big, bcol = scenes.random_triangles(400, W, H, seed=3800, rmin=80, rmax=300)
    out = (C.c_ulonglong * 16)()
    with Context(W, H, 3) as ctx:
        ctx.L.trgl_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
        ctx.draw(FLAT, big, colors=bcol)
        ctx.flush()
        assert ctx.last_flush_info()["pairs"] > 10_000
        for seed in (3801, 3802):
            clip, col = _tile_lists_scene(W, H, seed)
            ctx.clear()
            ctx.reset_stats()
            ctx.draw(FLAT, clip, colors=col)
            got = (ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats())
            assert ctx.L.trgl_debug_counters(ctx.h, out) == 0
            print(f"seed {seed}: candidates {out[0]} visits {out[2]} fragments {out[8]} dbg[9] {out[9]} dbg[10] {out[10]}", flush=True)
            assert out[0] > 0 and out[8] > 0, "the diagnostic build counted nothing: not the diagnostic library?"
            assert out[9] == 0, f"{out[9]} list entries that are no triangle of the flush"
            assert out[10] == 0, f"first foreign entry: list position {out[11] >> 32}, word {out[11] & 0xffffffff:#x}, tile {out[13] >> 32}"
            cases.assert_same_frame(got, cases.run_oracle(cases.make_case(W, H, [(FLAT, None, clip, None, col)])), what=f"seed {seed}")
    print("ok")


if __name__ == "__main__":
    main()
