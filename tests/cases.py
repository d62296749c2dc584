"""Named parity scenes shared by the golden-fixture generator, the oracle tests and the GPU tests, and the one harness that
renders a scene and checks it (run_oracle, run_gpu, assert_same_frame and friends, below).

Each builder returns a dict (make_case): width, height, bpp, viewport (4x4), draws = [(kind, uniforms|None, clip,
varyings|None, colors|None)], textures = {slot: array}, clear (4 bytes), zclear.
Inputs come from tinyrenderder_amd.scenes (bit-reproducible everywhere).
"""
import numpy as np

from tinyrenderder_amd import scenes
from tinyrenderder_amd.api import FLAT, GOURAUD, PHONG, EYE, CHECKER, make_uniforms

DEFAULT_CLEAR = (0, 0, 0, 255)


def make_case(w, h, draws, bpp=3, viewport=None, textures=None, clear=DEFAULT_CLEAR, zclear=np.inf):
    return dict(width=w, height=h, bpp=bpp, viewport=scenes.init_viewport(0, 0, w, h) if viewport is None else viewport,
                draws=draws, textures=textures or {}, clear=tuple(clear), zclear=zclear)


def flat_small_64():
    clip, col = scenes.random_triangles(300, 64, 64, seed=11, rmin=2, rmax=32)
    return make_case(64, 64, [(FLAT, None, clip, None, col)])


def flat_800():          # BASELINE config 0 shape: 800x800, flat, CPU-runnable
    clip, col = scenes.random_triangles(100_000, 800, 800, seed=12, rmin=1, rmax=16)
    return make_case(800, 800, [(FLAT, None, clip, None, col)])


def flat_persp_512():
    clip, col = scenes.random_triangles(20_000, 512, 512, seed=13, rmin=2, rmax=64, perspective_w=True)
    return make_case(512, 512, [(FLAT, None, clip, None, col)])


def flat_big_tris_512():
    clip, col = scenes.random_triangles(400, 512, 512, seed=14, rmin=64, rmax=512)
    return make_case(512, 512, [(FLAT, None, clip, None, col)])


def edge_256():
    clip, col = scenes.edge_case_triangles(256, 256)
    return make_case(256, 256, [(FLAT, None, clip, None, col)])


def grid_256():
    clip, col = scenes.shared_edge_grid(8, 8, 256, 256)
    return make_case(256, 256, [(FLAT, None, clip, None, col)])


def grid_fine_128():
    clip, col = scenes.shared_edge_grid(32, 32, 128, 128, z_slope=0.0)   # all z equal: every shared pixel is a tie
    return make_case(128, 128, [(FLAT, None, clip, None, col)])


def gouraud_256_rgba():
    clip, col = scenes.random_triangles(5000, 256, 256, seed=15, rmin=2, rmax=64, perspective_w=True)
    inten = scenes.SplitMix64(5).uniform(5000 * 3, -0.2, 1.3).reshape(5000, 3)
    return make_case(256, 256, [(GOURAUD, None, clip, inten, col)], bpp=4)


def _head(level, w, h, tex):
    hd = scenes.head_standin(level, w, h)
    d, n, s = scenes.procedural_textures(tex)
    return hd, {0: d, 1: n, 2: s}


def phong_512():
    hd, tx = _head(4, 512, 512, 256)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
    return make_case(512, 512, [(PHONG, u, hd["clip"], hd["varyings"], None)], textures=tx)


def phong_nomaps_256():
    hd, _ = _head(3, 256, 256, 64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.5, -1, -1, -1)
    return make_case(256, 256, [(PHONG, u, hd["clip"], hd["varyings"], None)])


def eye_256():
    hd, tx = _head(3, 256, 256, 128)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, -1, 2)
    return make_case(256, 256, [(EYE, u, hd["clip"], hd["varyings"], None)], textures=tx)


def multi_draw_320x200():
    """main.cpp's frame shape: background PHONG (strength 0.5), PHONG head, EYE on top, flat overlay."""
    w, h = 320, 200
    hd, tx = _head(3, w, h, 128)
    big = scenes.head_standin(2, w, h, seed=99, distance=1.6)
    u_bg = make_uniforms(big["model_view"], big["key"], big["fill"], big["rim"], 0.5, 0, 1, -1)
    u_hd = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, 1, 2)
    u_ey = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 1.0, 0, -1, -1)
    small = scenes.head_standin(2, w, h, seed=5, distance=4.0)
    fclip, fcol = scenes.random_triangles(500, w, h, seed=17, rmin=2, rmax=24)
    return make_case(w, h, [(PHONG, u_bg, big["clip"], big["varyings"], None),
                            (PHONG, u_hd, hd["clip"], hd["varyings"], None),
                            (EYE, u_ey, small["clip"], small["varyings"], None),
                            (FLAT, None, fclip, None, fcol)], textures=tx, clear=(30, 20, 10, 255))


def odd_dims_101x67():
    clip, col = scenes.random_triangles(2000, 101, 67, seed=18, rmin=1, rmax=24)
    return make_case(101, 67, [(FLAT, None, clip, None, col)])


def gray_bpp1_96x64():
    clip, col = scenes.random_triangles(1500, 96, 64, seed=19, rmin=1, rmax=24)
    return make_case(96, 64, [(FLAT, None, clip, None, col)], bpp=1)


def viewport_offset_256x160():
    clip, col = scenes.random_triangles(3000, 200, 120, seed=20, rmin=1, rmax=32)
    return make_case(256, 160, [(FLAT, None, clip, None, col)], viewport=scenes.init_viewport(16, 8, 200, 120))


def zclear_finite_128():
    clip, col = scenes.random_triangles(3000, 128, 128, seed=21, rmin=2, rmax=32)
    return make_case(128, 128, [(FLAT, None, clip, None, col)], bpp=4, clear=(7, 8, 9, 10), zclear=0.25)


def huge_depths_128():
    """NDC depths up to 1.7e308 on vertices 1 and 2 (vertex 0 stays inside [-1, 1], so our_gl.cpp:103-106 keeps the
    triangle): the interpolated depth (our_gl.cpp:156-158) lands on huge finite values of either sign.  (It does not
    overflow: the computed barycentrics of a covered pixel sum to 1 within a few ulp, and 1.7e308 leaves 5 % of headroom below
    the largest double, so our_gl.cpp:160 drops nothing here.  At the largest double itself it does: see overflowing_depths_scene
    in test_user_kind_raster_paths_gpu.py.)  The screen coordinates stay ordinary ('well scaled')."""
    clip, col = scenes.random_triangles(600, 128, 128, seed=23, rmin=4, rmax=48)
    clip = clip.copy()
    clip[0::5, 6] = 1.7e308;   clip[0::5, 10] = 1.7e308       # sums up to 1.7e308
    clip[1::5, 6] = -1.7e308;  clip[1::5, 10] = -1.7e308      # ... down to -1.7e308 (wins every z-test where covered)
    clip[2::5, 6] = 1.7e308;   clip[2::5, 10] = -1.7e308      # huge cancelling terms
    clip[3::5, 6] = -1e300                                     # huge but finite: wins where covered
    return make_case(128, 128, [(FLAT, None, clip, None, col)])


def checker_256():
    """The kind that discards (our_gl.cpp:187-188): fragments whose perspective-correct barycentrics fall on odd checker cells
    write nothing - no depth, no colour, no counter - so what lies behind them shows through and later fragments are tested against
    the depth they left alone.  Perspective w makes the perspective-correct barycentrics differ from the screen-space ones."""
    clip, col = scenes.random_triangles(4000, 256, 256, seed=31, rmin=4, rmax=48, perspective_w=True)
    return make_case(256, 256, [(CHECKER, make_uniforms(cells=6), clip, None, col)])


def checker_mixed_200x120():
    """Discarding and ordinary draws in one flush (per-fragment kinds): flat below, checker in the middle, Gouraud on top."""
    w, h = 200, 120
    c0, k0 = scenes.random_triangles(800, w, h, seed=32, rmin=4, rmax=40)
    c1, k1 = scenes.random_triangles(1500, w, h, seed=33, rmin=4, rmax=40, perspective_w=True)
    c2, k2 = scenes.random_triangles(600, w, h, seed=34, rmin=2, rmax=24, perspective_w=True)
    v2 = scenes.SplitMix64(35).uniform(600 * 3, 0.1, 1.2).reshape(600, 3)
    return make_case(w, h, [(FLAT, None, c0, None, k0), (CHECKER, make_uniforms(cells=3), c1, None, k1), (GOURAUD, None, c2, v2, k2)], bpp=4)


def empty_scene_64():
    return make_case(64, 64, [])


# ---- z ranges that end in a signed zero.  std::min / std::max (our_gl.cpp:197-198) keep the first of two equal values and
# +0.0 == -0.0, so the printed end is "-0.000000" or "0.000000" after the first zero fragment WRITTEN in the reference's order
# (triangle, then x, then y: our_gl.cpp:147-148).  Ordinary depths are folded to one side of zero, so that the range ends there.
UNIT_VIEWPORT = np.eye(4)          # screen = NDC: vertices can sit exactly on pixel centres (and edge deltas can be tiny)


def fold_depths(clip, sign):
    """Vertex depths folded to sign * |z| (the clip z is ndc z * w)."""
    c = clip.copy()
    for v in range(3):
        c[:, 4 * v + 2] = sign * np.abs(c[:, 4 * v + 2])
    return c


def set_zero_depths(clip, rows, signs):
    """Vertex depths of the triangles `rows` become zeros of the given signs (one +-1 per vertex, or one for all three)."""
    for i in rows:
        for v in range(3):
            s = signs[v] if hasattr(signs, "__len__") else signs
            clip[i, 4 * v + 2] = np.copysign(0.0, s)


def to_screen_space(clip, w, h):
    """Triangles made for the default viewport of a w x h frame, restated for UNIT_VIEWPORT (same pixels)."""
    c = clip.copy()
    for v in range(3):
        cw = c[:, 4 * v + 3]
        c[:, 4 * v + 0] = ((c[:, 4 * v + 0] / cw) * (w / 2.0) + w / 2.0) * cw
        c[:, 4 * v + 1] = ((c[:, 4 * v + 1] / cw) * (h / 2.0) + h / 2.0) * cw
    return c


def screen_triangle(p0, p1, p2, z=(0.0, 0.0, 0.0)):
    """One clip row for UNIT_VIEWPORT from pixel-space vertices (w = 1)."""
    return np.array([p0[0], p0[1], z[0], 1.0, p1[0], p1[1], z[1], 1.0, p2[0], p2[1], z[2], 1.0])


def zero_min_neg_first_96x64():
    """min ends at -0: triangles 100-102 write -0 before triangles 250-252 write +0 (both stay in the z-buffer)."""
    clip, col = scenes.random_triangles(400, 96, 64, seed=41, rmin=3, rmax=24)
    clip = fold_depths(clip, 1.0)
    set_zero_depths(clip, range(100, 103), -1.0)
    set_zero_depths(clip, range(250, 253), 1.0)
    return make_case(96, 64, [(FLAT, None, clip, None, col)])


def zero_min_pos_first_96x64():
    """min ends at +0 although a later triangle writes -0; perspective w."""
    clip, col = scenes.random_triangles(400, 96, 64, seed=42, rmin=3, rmax=24, perspective_w=True)
    clip = fold_depths(clip, 1.0)
    set_zero_depths(clip, range(120, 123), 1.0)
    set_zero_depths(clip, range(200, 203), -1.0)
    return make_case(96, 64, [(FLAT, None, clip, None, col)])


def zero_signs_in_one_triangle_96x64():
    """One triangle with vertex depths (-0, -0, +0) writes both signs: z = b0 (-0) + b1 (-0) + b2 (+0) is -0 only where
    b2 = u.x / u.z is -0, on its edge v0 v1 - a column of pixel centres (x = 20.5).  In the reference's x-major order the
    first pixel visited is that column (-0); a y-major walk would meet an interior pixel (+0) of row 10 first."""
    clip, col = scenes.random_triangles(300, 96, 64, seed=43, rmin=3, rmax=24)
    clip = fold_depths(to_screen_space(clip, 96, 64), 1.0)
    tri = screen_triangle((20.5, 52.5), (20.5, 18.5), (60.5, 10.2), z=(-0.0, -0.0, 0.0))
    clip = np.concatenate([clip[:150], tri[None], clip[150:]])
    col = np.concatenate([col[:150], np.array([0xFF10E0F0], np.uint32), col[150:]])
    return make_case(96, 64, [(FLAT, None, clip, None, col)], viewport=UNIT_VIEWPORT)


def zero_max_neg_first_96x64():
    """Every depth <= 0: max ends at the first zero written (-0 by triangles 20-22, +0 by 23-25 after them), RGBA."""
    clip, col = scenes.random_triangles(200, 96, 64, seed=44, rmin=2, rmax=12)
    clip = fold_depths(clip, -1.0)
    set_zero_depths(clip, range(20, 23), -1.0)
    set_zero_depths(clip, range(23, 26), 1.0)
    return make_case(96, 64, [(FLAT, None, clip, None, col)], bpp=4)


def zero_checker_discarded_first_96x64():
    """CHECKER (cells = 2) triangle with vertex depths (-0, -0, +0): its first column x = 10 lies on the edge v0 v1 (-0 there) and
    is discarded all the way (exactly one of pc0, pc1 is >= 0.5 on it), so the first zero WRITTEN is +0 from column 11.  A later
    all -0 triangle leaves -0 in the z-buffer as well.  Discarded fragments count nowhere: the range ends at +0."""
    w, h = 96, 64
    base, bcol = scenes.random_triangles(200, w, h, seed=45, rmin=3, rmax=24)
    base = fold_depths(to_screen_space(base, w, h), 1.0)
    tris, tcol = scenes.random_triangles(200, w, h, seed=46, rmin=3, rmax=24)
    tris = fold_depths(to_screen_space(tris, w, h), 1.0)
    first = screen_triangle((10.5, 50.7), (10.5, 11.3), (40.5, 30.5), z=(-0.0, -0.0, 0.0))
    later = screen_triangle((60.5, 40.5), (85.5, 45.5), (70.5, 58.5), z=(-0.0, -0.0, -0.0))
    tris = np.concatenate([tris[:80], first[None], tris[80:140], later[None], tris[140:]])
    tcol = np.concatenate([tcol[:80], np.array([0xFF3060C0], np.uint32), tcol[80:140], np.array([0xFFC06030], np.uint32), tcol[140:]])
    return make_case(w, h, [(FLAT, None, base, None, bcol), (CHECKER, make_uniforms(cells=2), tris, None, tcol)],
                     viewport=UNIT_VIEWPORT)


def phong_soup_varyings(n, seed):
    """PHONG / EYE varyings [n, 24] of a triangle soup: uv outside [0, 1), unnormalised and zero normals, degenerate uv frames."""
    vr = scenes.SplitMix64(seed)
    uv = vr.uniform(n * 6, -0.5, 1.5).reshape(n, 6)
    pos = vr.uniform(n * 9, -2.0, 2.0).reshape(n, 9)
    nrm = vr.uniform(n * 9, -1.0, 1.0).reshape(n, 9)
    nrm[::17] = 0.0
    uv[::13, 2:4] = uv[::13, 0:2]
    return np.ascontiguousarray(np.concatenate([uv, pos, nrm], 1))


def zero_phong_128x96():
    """PHONG soup (visibility buffer + k_shade) whose range ends at +0: +0 triangles 90-92 come before -0 triangles 200-202."""
    w, h = 128, 96
    clip, _ = scenes.random_triangles(360, w, h, seed=47, rmin=3, rmax=30, perspective_w=True)
    clip = fold_depths(clip, 1.0)
    set_zero_depths(clip, range(90, 93), 1.0)
    set_zero_depths(clip, range(200, 203), -1.0)
    hd, tx = _head(1, w, h, 64)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.7, 0, 1, 2)
    return make_case(w, h, [(PHONG, u, clip, phong_soup_varyings(360, 48), None)], textures=tx)


# the sign each zero case's z range must end at: (min end, max end) as copysign(1, .) of the printed value, None = not zero
ZERO_CASES = {"zero_min_neg_first_96x64": (-1.0, None), "zero_min_pos_first_96x64": (1.0, None),
              "zero_signs_in_one_triangle_96x64": (-1.0, None), "zero_max_neg_first_96x64": (None, -1.0),
              "zero_checker_discarded_first_96x64": (1.0, None), "zero_phong_128x96": (1.0, None)}


# ---- shading edges: small PHONG / EYE frames whose varyings reach the places where a reading of main.cpp:92-170, 220-261 and
# model.cpp:428-459 can go wrong.  Their goldens come from the reference's own PhongShader / EyeShader (oracle/_ref/ref_shaders).
def _texels(rng, w, h, bpp):
    return (rng.u64(w * h * bpp) & np.uint64(0xFF)).astype(np.uint8).reshape(h, w, bpp)


def _threshold_texels(rng, w, h, bpp):
    """Diffuse texels around the eye-pixel threshold (main.cpp:110-112): channel sums 650 (brightness 0.8497) and 651 (0.8510),
    with a quarter left random."""
    t = _texels(rng, w, h, bpp)
    pick = (rng.u64(w * h) % np.uint64(4)).astype(np.int64).reshape(h, w)
    t[pick == 0, :3] = (217, 217, 216)
    t[pick == 1, :3] = (216, 217, 217)
    t[pick == 2, :3] = (217, 217, 217)
    return t


def edge_textures():
    """Non-power-of-two textures of 1, 3 and 4 bytes per pixel.  Slots: diffuse 0 (bpp 3, threshold texels), 3 (bpp 1), 4 (bpp 4,
    threshold texels); normal 1 (bpp 3), 5 (bpp 4), 6 (bpp 1); specular 2 (bpp 1), 7 (bpp 4), 8 (bpp 3)."""
    r = scenes.SplitMix64(0x5EAD)
    return {0: _threshold_texels(r, 37, 23, 3), 1: _texels(r, 31, 19, 3), 2: _texels(r, 11, 5, 1), 3: _texels(r, 13, 7, 1),
            4: _threshold_texels(r, 29, 17, 4), 5: _texels(r, 7, 9, 4), 6: _texels(r, 5, 3, 1), 7: _texels(r, 9, 6, 4),
            8: _texels(r, 3, 5, 3)}


EDGE_UV = np.array([-0.5, 1.5, 1e12, -1e12, np.nan, 0.0, 1.0])


def edge_varyings(n, seed, uv_edges=0.3, normal_edges=0.3, position_edges=0.2, nonfinite=0.04):
    """PHONG / EYE varyings [n, 24] (uv[6], position_eye[9], normal_eye[9]).  A fraction of the rows reach the edges:
    uv_edges - uv components from EDGE_UV (outside [0, 1], +-1e12, NaN); normal_edges - zero normals on every vertex, or
    n1 = -n0 with n2 = 0 (the interpolated normal cancels where b0 = b1), or one zero vertex normal; position_edges -
    position_eye through zero (p1 = -p0, p2 = 0) or zero at every vertex; nonfinite - one normal or position component NaN
    or +-inf (a NaN dot product: the operand order of std::max(0.0, d) and std::min(255.0, v) decides the colour)."""
    r = scenes.SplitMix64(seed)
    uv = r.uniform(n * 6, -0.1, 1.1).reshape(n, 6)
    pos = r.uniform(n * 9, -2.0, 2.0).reshape(n, 9)
    nrm = r.uniform(n * 9, -1.0, 1.0).reshape(n, 9)
    pick = r.uniform(n * 3).reshape(n, 3)
    sub = (r.u64(n * 3) % np.uint64(3)).astype(np.int64).reshape(n, 3)
    uvsel = (r.u64(n * 6) % np.uint64(len(EDGE_UV) + 2)).astype(np.int64).reshape(n, 6)
    rows = pick[:, 0] < uv_edges
    special = rows[:, None] & (uvsel < len(EDGE_UV))
    uv[special] = EDGE_UV[uvsel[special]]
    rows = pick[:, 1] < normal_edges
    nrm[rows & (sub[:, 1] == 0)] = 0.0
    m = rows & (sub[:, 1] == 1)
    nrm[m, 3:6] = -nrm[m, 0:3]; nrm[m, 6:9] = 0.0
    m = rows & (sub[:, 1] == 2)
    nrm[m, 0:3] = 0.0
    rows = pick[:, 2] < position_edges
    m = rows & (sub[:, 2] != 2)
    pos[m, 3:6] = -pos[m, 0:3]; pos[m, 6:9] = 0.0
    pos[rows & (sub[:, 2] == 2)] = 0.0
    out = np.concatenate([uv, pos, nrm], 1)
    bad = np.flatnonzero(r.uniform(n) < nonfinite)
    col = 6 + (r.u64(bad.size) % np.uint64(18)).astype(np.int64)
    out[bad, col] = np.array([np.nan, np.inf, -np.inf])[(r.u64(bad.size) % np.uint64(3)).astype(np.int64)]
    return np.ascontiguousarray(out)


def _edge_uniforms(seed, strength=1.0, slots=(0, 1, 2)):
    hd = scenes.head_standin(0, 16, 16, seed=seed)
    return make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], strength, *slots)


def _edge_draw(kind, n, w, h, seed, strength=1.0, slots=(0, 1, 2), **edges):
    clip, _ = scenes.random_triangles(n, w, h, seed=seed, rmin=3, rmax=28, perspective_w=True)
    return (kind, _edge_uniforms(seed, strength, slots), clip, edge_varyings(n, seed + 1, **edges), None)


def shade_zero_normals_96x64():
    """PHONG: zero and cancelling interpolated normals (normalized() leaves a zero vector as it is, geometry.h:136-140), on and off
    eye pixels, and position_eye through zero (view direction of a zero vector)."""
    return make_case(96, 64, [_edge_draw(PHONG, 260, 96, 64, 601, normal_edges=0.7, position_edges=0.5)], textures=edge_textures())


def shade_zero_normals_eye_96x64_rgba():
    """EYE on an RGBA frame with a 4-byte diffuse map: zero / cancelling normals and position_eye through zero."""
    return make_case(96, 64, [_edge_draw(EYE, 260, 96, 64, 611, slots=(4, -1, 7), normal_edges=0.7, position_edges=0.5)],
                     bpp=4, textures=edge_textures())


def shade_uv_extremes_128x64():
    """PHONG with uv of -0.5, 1.5, +-1e12 and NaN (x86's INT_MIN clamps to texel 0) on 1-, 3- and 4-byte maps of odd sizes."""
    return make_case(128, 64, [_edge_draw(PHONG, 300, 128, 64, 621, uv_edges=0.8),
                               _edge_draw(PHONG, 300, 128, 64, 623, slots=(3, 5, 8), uv_edges=0.8),
                               _edge_draw(PHONG, 200, 128, 64, 625, slots=(4, 6, 7), uv_edges=0.8)], textures=edge_textures())


def shade_strengths_128x96_rgba():
    """normal_map_strength 0, 0.5, 1 and 1.7: the blend geometry_normal * (1 - s) + normal_map_eye * s (main.cpp:122-125)."""
    draws = [_edge_draw(PHONG, 200, 128, 96, 631 + 2 * i, strength=s, slots=((0, 1, 2), (4, 5, 7), (3, 6, 8), (0, 5, -1))[i])
             for i, s in enumerate((0.0, 0.5, 1.0, 1.7))]
    return make_case(128, 96, draws, bpp=4, textures=edge_textures(), clear=(1, 2, 3, 4))


def shade_eye_threshold_96x64_gray():
    """Diffuse texels with channel sums 650 and 651 on either side of brightness >= 0.85 (main.cpp:110-112), into a 1-byte
    frame: on eye pixels the unnormalized geometry normal is used (main.cpp:122-123)."""
    return make_case(96, 64, [_edge_draw(PHONG, 300, 96, 64, 641, strength=0.5, uv_edges=0.0),
                              _edge_draw(PHONG, 200, 96, 64, 643, slots=(4, 1, -1), uv_edges=0.0)],
                     bpp=1, textures=edge_textures())


def shade_no_textures_64x64():
    """PHONG and EYE without maps: white diffuse, (0, 0, 1) normal map, specular 1.0f (model.cpp:415-459 fallbacks)."""
    return make_case(64, 64, [_edge_draw(PHONG, 150, 64, 64, 651, strength=0.5, slots=(-1, -1, -1)),
                              _edge_draw(EYE, 100, 64, 64, 653, slots=(-1, -1, -1))])


SHADING_EDGE_CASES = ("shade_zero_normals_96x64", "shade_zero_normals_eye_96x64_rgba", "shade_uv_extremes_128x64",
                      "shade_strengths_128x96_rgba", "shade_eye_threshold_96x64_gray", "shade_no_textures_64x64")


def shader_fragment_inputs(n=20000, seed=0x51AD):
    """Single fragment() calls for tests/golden/shader_golden.npz: (textures, kinds [n], uniforms [n], varyings [n, 24],
    bary [n, 3]).  Weighted towards the edges of edge_varyings; bary is a vertex, an edge midpoint (where n1 = -n0 cancels
    exactly) or random; lights are unit, unnormalized, zero or hold a NaN; strengths 0, 0.5, 1, 1.7 or random."""
    r = scenes.SplitMix64(seed)
    vary = edge_varyings(n, seed + 1, uv_edges=0.35, normal_edges=0.4, position_edges=0.3)
    kinds = np.where(r.uniform(n) < 0.6, PHONG, EYE).astype(np.int32)
    b = r.uniform(n * 3, 0.0, 1.0).reshape(n, 3)
    b /= b.sum(1, keepdims=True)
    form = (r.u64(n) % np.uint64(4)).astype(np.int64)
    b[form == 0] = (1.0, 0.0, 0.0)
    b[form == 1] = (0.5, 0.5, 0.0)
    b[form == 2] = (0.0, 0.5, 0.5)
    slot_sets = [(0, 1, 2), (3, 5, 8), (4, 6, 7), (-1, -1, -1), (0, -1, 2), (4, 1, -1), (-1, 5, 7)]
    sets = (r.u64(n) % np.uint64(len(slot_sets))).astype(np.int64)
    strengths = np.array([0.0, 0.5, 1.0, 1.7])
    ssel = (r.u64(n) % np.uint64(5)).astype(np.int64)
    srand = r.uniform(n, -0.5, 2.0)
    mvs = [scenes.head_standin(0, 16, 16, seed=s)["model_view"] for s in (1, 2, 3)] + [np.eye(4)]
    msel = (r.u64(n) % np.uint64(len(mvs))).astype(np.int64)
    lights = r.uniform(n * 9, -1.0, 1.0).reshape(n, 3, 3)
    lform = (r.u64(n) % np.uint64(5)).astype(np.int64)
    lights[lform <= 1] /= np.linalg.norm(lights[lform <= 1], axis=2, keepdims=True)
    lights[lform == 3, 0] = 0.0
    lights[lform == 4, 1, 2] = np.nan
    uniforms = [make_uniforms(mvs[msel[i]], lights[i, 0], lights[i, 1], lights[i, 2],
                              strengths[ssel[i]] if ssel[i] < 4 else srand[i], *slot_sets[sets[i]]) for i in range(n)]
    return edge_textures(), kinds, uniforms, vary, np.ascontiguousarray(b)


def fixture_mesh():
    """The mesh of the N1 fixtures (tests/golden/next_rows_golden.json): the head stand-in's vertices, float-representable (the
    reference reads them through Assimp's float aiVector3D), shared between faces through a shuffled index buffer.  Returns
    (vertices [nv, 8] f64: position, normal, uv; indices [nf, 3] u32, uniforms, projection, width, height)."""
    w, h = 160, 120
    hd = scenes.head_standin(2, w, h)
    pos, nrm, uv = hd["positions"].reshape(-1, 3), hd["normals"].reshape(-1, 3), hd["uvs"].reshape(-1, 2)
    verts = np.concatenate([pos, nrm, uv], 1).astype(np.float32).astype(np.float64)
    perm = np.argsort(scenes.SplitMix64(19).u64(pos.shape[0]), kind="stable")
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    u = make_uniforms(hd["model_view"], hd["key"], hd["fill"], hd["rim"], 0.8, 0, 1, 2)
    return np.ascontiguousarray(verts[perm]), inv.astype(np.uint32).reshape(-1, 3), u, hd["projection"], w, h


def fixture_zbuffers():
    """z-buffers of the N4 fixtures: name -> [h, w] f64.  Random depths with +-inf and NaN holes, a constant one (max - min
    below 1e-7), one with no finite depth, and depth steps that the SSAO threshold 1e-3 sees on one side only."""
    r = scenes.SplitMix64(0x2B0F)
    a = r.uniform(64 * 48, -1.0, 1.0).reshape(48, 64)
    a[r.uniform(64 * 48).reshape(48, 64) < 0.15] = np.inf
    a[5, 7] = -np.inf; a[9, 30] = np.nan
    steps = np.repeat(np.repeat(r.uniform(8 * 6, 0.0, 0.01).reshape(6, 8), 8, 0), 9, 1)[:, :70]
    steps[20:30, 30:40] = np.inf
    return {"random_holes_64x48": a, "constant_40x24": np.full((24, 40), 0.125), "all_inf_24x16": np.full((16, 24), np.inf),
            "steps_70x48": np.ascontiguousarray(steps)}


CASES = {f.__name__: f for f in (
    flat_small_64, flat_800, flat_persp_512, flat_big_tris_512, edge_256, grid_256, grid_fine_128, gouraud_256_rgba,
    phong_512, phong_nomaps_256, eye_256, multi_draw_320x200, odd_dims_101x67, gray_bpp1_96x64,
    viewport_offset_256x160, zclear_finite_128, huge_depths_128, empty_scene_64, checker_256, checker_mixed_200x120,
    zero_min_neg_first_96x64, zero_min_pos_first_96x64, zero_signs_in_one_triangle_96x64, zero_max_neg_first_96x64,
    zero_checker_discarded_first_96x64, zero_phong_128x96, shade_zero_normals_96x64, shade_zero_normals_eye_96x64_rgba,
    shade_uv_extremes_128x64, shade_strengths_128x96_rgba, shade_eye_threshold_96x64_gray, shade_no_textures_64x64)}

# cases whose full buffers are stored in tests/golden/ (small enough to commit)
FULL_BUFFER_CASES = ("flat_small_64", "odd_dims_101x67", "gray_bpp1_96x64")


def vecops_inputs(n=2000):
    """Inputs of the value-op comparison (tests/golden/make_vecops_golden.py, test_oracle.py): per row v[3], n[3], M[16],
    v0 v1 v2 b [3 each] and an intensity, plus a packed colour.  Returns (data [n,35] f64, packed [n] u32)."""
    rng = scenes.SplitMix64(77)
    data = rng.uniform(n * 35, -3.0, 3.0).reshape(n, 35)
    data[0, 0:3] = 0.0                                    # normalized(0) returns v
    data[:, 34] = rng.uniform(n, -0.5, 1.5)
    packed = (rng.u64(n) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return data, packed


def loaded_buffers(W, H, bpp):
    """A framebuffer and a z-buffer for a frame that starts from caller-written buffers (write_framebuffer / write_zbuffer): a colour
    pattern, and depth bands with NaN, -inf and +inf columns and a row band nothing passes."""
    y, x = np.mgrid[0:H, 0:W]
    fb = np.stack([(x * 7 + y * 13 + c * 31 + 5) & 0xFF for c in range(bpp)], -1).astype(np.uint8)
    z = np.where((y // 8) % 2 == 0, 0.6, -0.2) + 0.001 * x
    z[:, 5:9] = np.nan
    z[:, 20:23] = -np.inf
    z[:, 30:34] = np.inf
    z[40:44, :] = 0.95
    return fb, z


# ---- render a case and check it: the one harness of the GPU tests ---------------------------------------------------
def run_oracle(case, strip=None, start=None):
    """Render a case with the CPU oracle; returns (fb, z, stats tuple).  strip = (y0, y1): only those rows are drawn.
    start = (fb, z): the frame starts from these buffers instead of the clear (a None one is cleared)."""
    from oracle import orc
    o = orc.Oracle(case["width"], case["height"], case["bpp"], viewport=case["viewport"], clear_bgra=case["clear"],
                   z_clear=case["zclear"], strip=strip)
    fb0, z0 = start or (None, None)
    if fb0 is not None:
        o.fb[:] = fb0
    if z0 is not None:
        o.z[:] = z0
    for slot, t in case["textures"].items():
        o.upload_texture(slot, t)
    for kind, u, clip, vary, col in case["draws"]:
        o.draw(kind, clip, vary, col, None if u is None else orc.Uniforms.from_buffer_copy(bytes(u)))
    return o.fb, o.z, o.stats


def device_array(a, off=0):
    """A torch CUDA tensor holding the numpy array `a` (f64, or u32 carried as int32), its first element `off` bytes into a
    larger allocation (off: a multiple of the item size; torch's allocations themselves start on 512-byte boundaries)."""
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a
    assert off % a.itemsize == 0, (off, a.dtype)
    lead = off // a.itemsize
    buf = torch.empty(a.size + lead + (1 if lead else 0), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    t = buf[lead:lead + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_cuda and t.is_contiguous() and t.data_ptr() == buf.data_ptr() + off
    return t


def on_device(case, clip_off=0, vary_off=0, col_off=0, producer_sync=True):
    """The case with the clip, varyings and colour arrays of every draw in device memory (torch CUDA tensors: run_gpu draws
    them with device=True, slicing them for split=), each placed *_off bytes into a larger allocation (a multiple of 8 for
    the doubles, of 4 for the colours).  producer_sync: wait for the uploads, which run on torch's stream - a context's own
    stream is not ordered behind it."""
    import torch
    draws = [(kind, u, device_array(clip, clip_off), None if vary is None else device_array(vary, vary_off),
              None if col is None else device_array(col, col_off)) for kind, u, clip, vary, col in case["draws"]]
    if producer_sync:
        torch.cuda.synchronize()
    return dict(case, draws=draws)


def register_user_kind(ctx, sh):
    """The user kind of sh = (source, K[, flag word]) on a context: bit 0 of the word (True counts as 1) is TRGL_SHADER_MAY_DISCARD,
    bit 2 TRGL_SHADER_READS_DEST, bit 3 TRGL_SHADER_NO_DEPTH_WRITE (include/trgl.h)."""
    flags = int(sh[2]) if len(sh) > 2 else 0
    return ctx.register_shader(sh[0], sh[1], bool(flags & 1), reads_dest=bool(flags & 4), depth_write=not flags & 8)


def run_gpu(case, strip=None, interleave=None, split=None, flush_after=None, halves=False, start=None, shaders=None, inspect=None):
    """Render a case through the C ABI on the GPU; returns (fb, z, stats tuple, stats line).
    strip = (y0, y1): a strip context (set_strip); interleave = (band_rows, rank, world): one rank's bands (set_interleave).
    split = k: each draw in k flushes; flush_after = i: a flush after draw i; halves: the last flush as flush_begin / flush_end.
    start = (fb, z): as for run_oracle, through write_framebuffer / write_zbuffer.
    shaders: per draw, None or (source, K[, flag word]): the draw uses the user kind the context registers for it
    (register_user_kind).  inspect: f(ctx), called after the last flush has completed and before the read-backs; a run with
    it ends in an explicit flush() for that, where every other run leaves the last flush to the first read-back.
    A draw whose clip array is a torch CUDA tensor is drawn from device memory (on_device: all of its arrays are); the
    binding refuses a host array in such a draw."""
    from tinyrenderder_amd.api import Context
    shaders = shaders or [None] * len(case["draws"])
    with Context(case["width"], case["height"], case["bpp"]) as ctx:
        user = {sh: register_user_kind(ctx, sh) for sh in dict.fromkeys(sh for sh in shaders if sh)}
        ctx.set_viewport(case["viewport"])
        fb0, z0 = start or (None, None)
        if fb0 is None or z0 is None:
            ctx.clear(case["clear"], case["zclear"])
        if fb0 is not None:
            ctx.write_framebuffer(fb0)
        if z0 is not None:
            ctx.write_zbuffer(z0)
        if strip is not None:
            ctx.set_strip(*strip)
        if interleave is not None:
            ctx.set_interleave(*interleave)
        for slot, t in case["textures"].items():
            ctx.upload_texture(slot, t)
        for i, ((kind, u, clip, vary, col), sh) in enumerate(zip(case["draws"], shaders)):
            n = clip.shape[0]
            parts = split or 1
            edges = [n * k // parts for k in range(parts + 1)]
            for a, b in zip(edges[:-1], edges[1:]):
                if a == b:
                    continue
                ctx.draw(user[sh] if sh else kind, clip[a:b], None if vary is None else vary[a:b],
                         None if col is None else col[a:b], u, device=not isinstance(clip, np.ndarray))
                if split:
                    ctx.flush()
            if i == flush_after:
                ctx.flush()
        if halves:
            ctx.flush_begin()
            ctx.flush_end()
        if inspect is not None:
            ctx.flush()
            inspect(ctx)
        return ctx.read_framebuffer(), ctx.read_zbuffer(), ctx.stats(), ctx.stats_line()


def has_eye(case):
    """EYE draws shade with pow(x, 8), whose last ulp may differ from the oracle's (see assert_same_frame)."""
    return any(d[0] == EYE for d in case["draws"])


def band_rows(height, interleave):
    """Row ranges [y0, y1) that set_interleave(band_rows, rank, world) = interleave gives its rank (all rows for one rank)."""
    from tinyrenderder_amd import shard
    band, rank, world = interleave
    return shard.band_rows_of(height, world, rank, band) if world > 1 else [(0, height)]


def assert_same_frame(got, want, rows=None, eye=False, stats=True, what="frame"):
    """got, want: (fb, z, stats tuple[, stats line]) as run_gpu / run_oracle return them.  In `rows` (None: every row; one
    (y0, y1) or a list of them) the z bits and the framebuffer bytes are equal; so are the stats tuples unless stats=False (a
    strip or band against the whole frame), and then the stats lines when both sides have one.
    eye: a colour byte may be 1 LSB off, on at most 0.1 % of the pixels of each row range (EYE's pow(x, 8)); z stays exact."""
    ranges = [(0, got[0].shape[0])] if rows is None else [rows] if np.isscalar(rows[0]) else rows
    for y0, y1 in ranges:
        _assert_none(got[1][y0:y1].view(np.uint64) != want[1][y0:y1].view(np.uint64), y0, f"{what}: z values differ")
        fb, ref = got[0][y0:y1], want[0][y0:y1]
        if not eye:
            _assert_none(fb != ref, y0, f"{what}: framebuffer bytes differ")
            continue
        d = np.abs(fb.astype(np.int16) - ref.astype(np.int16))
        _assert_none(d > 1, y0, f"{what}: colour bytes differ by more than 1 LSB")
        px = d.max(axis=-1) > 0
        assert px.mean() <= 1e-3, f"{what}: {px.sum()} of {px.size} pixels differ, first at {_first(px, y0)}"
    if stats:
        assert got[2] == want[2], f"{what}: stats {got[2]} != {want[2]}"
        if len(got) > 3 and len(want) > 3:
            assert got[3] == want[3], f"{what}: stats line {got[3]!r} != {want[3]!r}"


def _first(bad, y0):
    at = np.argwhere(bad)[:5]
    at[:, 0] += y0
    return at.tolist()


def _assert_none(bad, y0, what):
    assert not bad.any(), f"{what}: {int(bad.sum())} of them, first at {_first(bad, y0)}"


def check_gpu(case, strip=None, split=None):
    """run_gpu against run_oracle with the same strip, on the strip's rows (EYE draws within their tolerance); returns run_gpu's."""
    got = run_gpu(case, strip=strip, split=split)
    assert_same_frame(got, run_oracle(case, strip=strip), rows=strip, eye=has_eye(case))
    return got


def assert_golden(got, g, eye=False):
    """got (run_gpu) against a golden entry (the reference's own frame): its stats line and the digests of its z bits and,
    unless eye (the oracle comparison bounds EYE colours), of its framebuffer bytes."""
    assert got[3] == g["stats"], (got[3], g["stats"])
    assert scenes.digest(got[1]) == g["z"], "z-buffer digest differs"
    if not eye:
        assert scenes.digest(got[0]) == g["fb"], "framebuffer digest differs"


# ---- BASELINE configs[3] / [4] at their stated sizes (C4 = 10 M random triangles at 4096^2,
# C5 = the C4-style scene at 8192^2, N = 10 M).  Too slow for the scalar oracle inside a test: the reference's own
# rasterize() rendered them once (tests/golden/make_golden_fullsize.py) and tests/golden/golden_fullsize.json holds the
# digests of its framebuffer bytes, z-buffer bits and its print_render_stats() line.
def c4_4096_10m():
    clip, col = scenes.random_triangles(10_000_000, 4096, 4096)          # = bench.py's default workload
    return make_case(4096, 4096, [(FLAT, None, clip, None, col)])


def c5_8192_10m():
    clip, col = scenes.random_triangles(10_000_000, 8192, 8192, seed=0x5EED0005, rmin=2, rmax=40)
    return make_case(8192, 8192, [(FLAT, None, clip, None, col)])


FULLSIZE_CASES = {f.__name__: f for f in (c4_4096_10m, c5_8192_10m)}
