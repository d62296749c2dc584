"""CPU tests of tests/binning_model.py, the host model that tests/test_stage_outputs_gpu.py holds the GPU's setup records and pair
lists against: the model itself is checked against the CPU oracle (the restatement of our_gl.cpp)."""
import numpy as np
import pytest

import binning_model as bm
import cases
from oracle import orc

# every case of cases.CASES whose triangles the oracle can draw one by one in a few seconds
SMALL_CASES = [n for n in cases.CASES if n not in ("flat_800", "flat_persp_512", "phong_512")]


def _flat_case(case, keep=None):
    """the case with every draw as FLAT (coverage and depth do not depend on the kind), optionally only the triangles `keep`"""
    clip = bm.flush_clip(case)
    col = np.arange(len(clip), dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0xff000000)
    if keep is not None:
        clip, col = clip[keep], col[keep]
    return dict(case, draws=[(orc.FLAT, None, clip, None, col)], textures={})


@pytest.mark.parametrize("name", SMALL_CASES)
def test_accepted_triangles_alone_give_the_full_frame(name):
    """Nothing the model rejects contributes to the oracle's frame: drawing only the accepted triangles gives the same z bits,
    bytes, fragment count, bbox and z range (the triangle counter counts submissions, our_gl.cpp:90, and is left out)."""
    case = cases.CASES[name]()
    m = bm.model(case)
    full, part = cases.run_oracle(_flat_case(case)), cases.run_oracle(_flat_case(case, m.accepted))
    assert np.array_equal(full[1].view(np.uint64), part[1].view(np.uint64)), "z differs"
    assert np.array_equal(full[0], part[0]), "framebuffer differs"
    assert full[2][1:] == part[2][1:], (full[2], part[2])


@pytest.mark.parametrize("name", SMALL_CASES)
def test_block_masks_contain_every_pixel_a_triangle_writes(name):
    """Each triangle drawn alone on a cleared frame: every pixel the oracle writes lies in a block that the model's pair masks
    name, and a triangle the model gives no pairs writes nothing."""
    case = cases.CASES[name]()
    m = bm.model(case)
    assert m.N == sum(len(d[2]) for d in case["draws"])
    wrote = 0
    for i, ys, xs, z in bm.single_triangle_depths(case, m, which=range(m.N)):
        if not len(ys):
            continue
        wrote += 1
        assert m.has_pairs[i], f"triangle {i} writes {len(ys)} pixels but the model gives it no pairs"
        px = bm.mask_pixels(m, i)
        assert px[ys, xs].all(), f"triangle {i}: pixel {(int(xs[~px[ys, xs]][0]), int(ys[~px[ys, xs]][0]))} outside its block masks"
        assert (xs >= m.bx0[i]).all() and (xs <= m.bx1[i]).all() and (ys >= m.by0[i]).all() and (ys <= m.by1[i]).all()
    assert wrote or name == "empty_scene_64"


def test_pair_count_and_masks_agree():
    """cnt is the number of tiles triangle_tiles lists, every mask is non-empty, and strips / bands partition the pairs of the frame."""
    case = cases.CASES["multi_draw_320x200"]()
    whole = bm.model(case)
    for i in range(whole.N):
        tl = bm.triangle_tiles(whole, i)
        assert len(tl) == whole.cnt[i] and all(mk for _, mk in tl)
    tiles_whole = {(t, i) for t, i, _ in bm.pairs(whole)}
    for world, band in ((2, 32), (4, 64)):
        got = [bm.pairs(bm.model(case, interleave=(band, r, world))) for r in range(world)]
        union = set().union(*got)
        assert sum(len(g) for g in got) == len(union) and union == bm.pairs(whole)
    strips = [(0, 37), (37, 150), (150, 200)]
    got = [{(t, i) for t, i, _ in bm.pairs(bm.model(case, strip=s))} for s in strips]
    assert set().union(*got) == tiles_whole
