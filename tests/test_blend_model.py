"""The blending model (blend_model.py) against the oracle it is built on, and the scenes of the GPU tests against what they are meant
to reach: no GPU and nothing of the library but its scene generator."""
import numpy as np
import pytest

import blend_model as B
from oracle import orc
from tinyrenderder_amd.api import FLAT


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_source_colour_with_depth_writes_is_the_oracle(bpp):
    """"return src, never discard, write depth" is FLAT: the frame, the z bits and the stats of one Oracle.draw of the whole scene."""
    name = f"96x64_bpp{bpp}"
    cfg, clip, col = B.frame(name)
    o = orc.Oracle(cfg["w"], cfg["h"], bpp, viewport=cfg["viewport"], clear_bgra=cfg["clear"], z_clear=cfg["zclear"])
    o.draw(FLAT, clip, None, col)
    fb, z, st, line = B.model_frame(name, B.f_source)
    assert (fb == o.fb).all()
    assert (z.view(np.uint64) == o.z.view(np.uint64)).all()
    assert st == o.stats and st[1] > 0
    assert line == orc.format_stats_line(o.stats)


def test_source_colour_from_loaded_buffers_and_seeded_stats():
    """start= and stats0=: a second model continued from the first one's frame ends where one model of the whole scene ends."""
    cfg, clip, col = B.frame("101x67_viewport_zclear")
    a = B.Model(**cfg)
    a.draw(clip[:100], col[:100], B.f_over)
    b = B.Model(**cfg, start=(a.fb, a.z), stats0=a.stats)
    b.draw(clip[100:], col[100:], B.f_over)
    want = B.model_frame("101x67_viewport_zclear", B.f_over)
    assert (b.fb == want[0]).all() and (b.z.view(np.uint64) == want[1].view(np.uint64)).all() and b.stats == want[2]


@pytest.mark.parametrize("name", sorted(B.FRAMES))
@pytest.mark.parametrize("depth_write", [True, False])
def test_scenes_are_order_sensitive(name, depth_write):
    fwd = B.model_frame(name, B.f_over, depth_write)
    rev = B.model_frame(name, B.f_over, depth_write, reverse=True)
    assert (fwd[0] != rev[0]).any()


@pytest.mark.parametrize("name", sorted(B.FRAMES))
def test_no_depth_write_keeps_the_clear_depth_and_passes_more(name):
    cfg, _, _ = B.frame(name)
    with_z, without = B.model_frame(name, B.f_over), B.model_frame(name, B.f_over, False)
    assert (without[1] == cfg["zclear"]).all()
    assert without[2][1] > with_z[2][1] > 0            # every layer in front of the clear depth passes
    assert without[2][0] == with_z[2][0] and without[2][2:6] == with_z[2][2:6]


def test_alpha_test_scene_discards_and_draws():
    over, cut = B.model_frame("96x64_bpp3", B.f_over), B.model_frame("96x64_bpp3", B.f_alpha_test)
    assert 0 < cut[2][1] < over[2][1]
    assert (cut[0] != over[0]).any()


@pytest.mark.parametrize("name, fn", [("96x64_bpp3", B.f_probe_bpp3), ("96x64_bpp1", B.f_probe_bpp1)])
def test_probe_scene_reaches_the_unmasked_case(name, fn):
    """The probe shader writes 0xAA above the frame's bytes and shows in blue what dst has there.  A model that formed dst from the
    last colour's 32 bits would differ from the one that masks: the scene has pixels drawn more than once."""
    masked, unmasked = B.model_frame(name, fn), B.model_frame(name, fn, mask_dst=False)
    assert (masked[0][..., 0] == 0).all()
    assert (unmasked[0][..., 0] != 0).any()


def test_blend_over_against_its_formula():
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    got = B.blend_over(src, dst)
    for s, d, g in zip(src[:500].tolist(), dst[:500].tolist(), got[:500].tolist()):
        a = s >> 24
        want = [(((s >> i) & 255) * a + ((d >> i) & 255) * (255 - a) + 127) // 255 for i in (0, 8, 16)] + [(255 * a + (d >> 24) * (255 - a) + 127) // 255]
        assert [(g >> i) & 255 for i in (0, 8, 16, 24)] == want
    assert B.blend_over(np.uint32([0xff123456]), np.uint32([0x0badcafe]))[0] == 0xff123456       # opaque: the source
    assert B.blend_over(np.uint32([0x00123456]), np.uint32([0x7badcafe]))[0] == 0x7badcafe       # transparent: the destination
