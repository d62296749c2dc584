"""What the tests of trgl_instance_depths / trgl_depth_order / the ordered instanced calls share: the array of special depths, the order
lists, the stage cases (on top of tests/instanced_cases.py) and the two scenes whose result depends on the order of the instances."""
import collections

import numpy as np

import blend_model as B
import instanced_cases as IC
import vertex_shader_sources as V
from tinyrenderder_amd import scenes

# the sizes of the depth and order tests: 0, 1, around a wavefront and a block, past the one-block sort, and IC.BIG - more than one scan
# block and a second level of block sums
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097, IC.BIG)
assert IC.BIG == 66085


def special_depths():
    """A fixed array: both NaN signs (two payloads each), the infinities, the zeros, denormals, runs of 300 equal values, random doubles
    of every magnitude and ordinary ones."""
    rng = scenes.SplitMix64(0x0DE9)
    bits = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,      # NaNs: +quiet, -quiet, +signalling, -all ones
                     0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000000, 0x8000000000000000,      # +inf, -inf, +0, -0
                     0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,      # denormals
                     0x0010000000000000, 0x8010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64).view(np.float64)
    runs = np.concatenate([np.full(300, -2.5), np.full(300, 0.0), np.full(300, -0.0), np.full(300, np.nan)])
    anybits = rng.u64(400).view(np.float64)                           # every exponent, NaNs among them
    ordinary = rng.uniform(400, -8.0, 8.0)
    a = np.concatenate([bits, runs, anybits, ordinary, bits[::-1]])
    return np.ascontiguousarray(a[rng.u64(a.size).argsort(kind="stable")])     # shuffled, so that the runs are not contiguous


def depths_of(n):
    """The special array repeated (or cut) to length n."""
    s = special_depths()
    return np.ascontiguousarray(np.resize(s, n)) if n else np.zeros(0)


# ---- order lists ------------------------------------------------------------------------------------------------------------
ORDERS = ("identity", "reversed", "random", "repeats", "shorter", "out_of_range")


def order_list(kind, n, seed=13):
    """[m] uint32 for n instances.  out_of_range: a random permutation with the entries n and 0xFFFFFFFF mixed in (device lists only)."""
    rng = scenes.SplitMix64(seed + n)
    perm = rng.u64(n).argsort(kind="stable").astype(np.uint32)
    if kind == "identity":
        return np.arange(n, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    if kind == "random":
        return perm
    if kind == "repeats":
        return np.concatenate([perm, perm[:max(1, n // 3)], perm[:1]]) if n else perm
    if kind == "shorter":
        return perm[:max(1, (2 * n) // 3)] if n else perm
    assert kind == "out_of_range", kind
    o = np.concatenate([perm, np.array([n, 0xFFFFFFFF, n + 1, 0x80000000], np.uint32)])
    return np.ascontiguousarray(o[rng.u64(o.size).argsort(kind="stable")])


# ---- the stage cases: a shape of instanced_cases (stage, faces, instances, visibility, stride, memory, colours) under an order ------
Case = collections.namedtuple("Case", "stage nf n pattern stride inst_device colors order order_device")
CASES = {
    "builtin_box_257_random_dev_identity_dev": Case("builtin", 12, 257, "random", 16, True, "instance", "identity", True),
    "builtin_box_257_absent_dev_random_host": Case("builtin", 12, 257, "absent", 19, True, "instance", "random", False),
    "builtin_1f_big_alternating_dev_reversed_dev": Case("builtin", 1, IC.BIG, "alternating", 16, True, "instance", "reversed", True),
    "builtin_65f_3_all1_host_repeats_host": Case("builtin", 65, 3, "all1", 19, False, None, "repeats", False),
    "builtin_box_64_first_host_out_of_range_dev": Case("builtin", 12, 64, "first", 16, False, "face", "out_of_range", True),
    "builtin_box_257_last_host_shorter_host": Case("builtin", 12, 257, "last", 16, False, "instance", "shorter", False),
    "builtin_1f_257_all0_dev_random_dev": Case("builtin", 1, 257, "all0", 16, True, None, "random", True),
    "k0_1f_big_random_dev_out_of_range_dev": Case("k0", 1, IC.BIG, "random", 16, True, "instance", "out_of_range", True),
    "k0_box_64_absent_host_reversed_host": Case("k0", 12, 64, "absent", 19, False, "instance", "reversed", False),
    "k0_box_3_alternating_no_instances_repeats_dev": Case("k0", 12, 3, "alternating", 0, True, "instance", "repeats", True),
    "k5_box_257_alternating_dev_shorter_host": Case("k5", 12, 257, "alternating", 16, True, "face", "shorter", False),
    "k5_65f_3_absent_dev_repeats_dev": Case("k5", 65, 3, "absent", 19, True, None, "repeats", True),
    "k5_1f_257_random_host_random_dev": Case("k5", 1, 257, "random", 19, False, "instance", "random", True),
    "k5_box_64_last_host_identity_host": Case("k5", 12, 64, "last", 16, False, "instance", "identity", False),
    "k64_65f_3_all1_host_reversed_dev": Case("k64", 65, 3, "all1", 16, False, "face", "reversed", True),
    "k64_1f_257_first_dev_random_host": Case("k64", 1, 257, "first", 16, True, None, "random", False),
    "k64_box_64_random_dev_out_of_range_dev": Case("k64", 12, 64, "random", 19, True, "instance", "out_of_range", True),
}


def case_inputs(c):
    """(vertices, indices, instances or None, visible or None, face_colors or None, instance_colors or None, order) of a Case."""
    return IC.shape_inputs(IC.Shape(*c[:7])) + (order_list(c.order, c.n),)


# ---- the two scenes whose result depends on the order ---------------------------------------------------------------------------
# a user vertex shader (K = 0) that moves the vertex by the translation of the instance's row-major matrix - the records are matrices,
# so that trgl_instance_depths reads the same array
QUAD_VS = V._DOT4 + r"""
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* p = in.vertex; const double* M = in.inst;
    double q[3], eye[4];
    for (int k = 0; k < 3; ++k) q[k] = p[k] + M[4 * k + 3];
    for (int r = 0; r < 4; ++r) eye[r] = vs_dot4(in.u->model_view + 4 * r, q[0], q[1], q[2], 1.0);
    for (int r = 0; r < 4; ++r) out.clip[r] = vs_dot4(in.projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
}
"""


def quad(half=0.5):
    """Two faces in the plane z = 0, facing +z: records of 8 doubles."""
    p = np.array([[-half, -half, 0.0], [half, -half, 0.0], [half, half, 0.0], [-half, half, 0.0]])
    verts = np.concatenate([p, np.tile([0.0, 0.0, 1.0], (4, 1)), (p[:, :2] + half) / (2 * half)], 1)
    return np.ascontiguousarray(verts), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def quad_scene(w, h, n=48, seed=0x51DE):
    """n quads of side 1.4 at scattered places and distinct depths in front of a camera at z = 5 that looks down -z, behind nothing; an
    opaque FLAT layer (two triangles at z = -4) lies behind them all.  Colours: random, with alphas between 64 and 192."""
    rng = scenes.SplitMix64(seed)
    mv = scenes.lookat([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    proj = scenes.perspective(scenes.TAN_35DEG, w / h, 1.0, 30.0)
    verts, idx = quad(0.7)
    inst = np.zeros((n, 16))
    inst[:, [0, 5, 10, 15]] = 1.0
    inst[:, 3] = rng.uniform(n, -1.6, 1.6)
    inst[:, 7] = rng.uniform(n, -1.0, 1.0)
    inst[:, 11] = (rng.u64(n).argsort(kind="stable").astype(np.float64) / n) * 5.0 - 3.0      # distinct depths in [-3, 2), shuffled
    col = (rng.u64(n) & np.uint64(0xFFFFFF)).astype(np.uint32) | (np.uint32(64) + (rng.u64(n) % np.uint64(129)).astype(np.uint32)) << np.uint32(24)
    wall_v = np.array([[-6.0, -4.0, -4.0], [6.0, -4.0, -4.0], [6.0, 4.0, -4.0], [-6.0, 4.0, -4.0]])
    wall, _ = V.expect_clip(mv, proj, np.concatenate([wall_v, np.zeros((4, 5))], 1), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    return dict(w=w, h=h, mv=mv, proj=proj, verts=verts, idx=idx, inst=np.ascontiguousarray(inst), col=col.astype(np.uint32), wall=wall,
                wall_col=np.array([0xFF506070, 0xFF506070], np.uint32), point=np.zeros(3))


def quad_rows(sc, drawn):
    """The clip rows QUAD_VS gives the instances `drawn`, in that order, and their colours (one per triangle)."""
    clip, _ = IC.expect_user("k0", sc["mv"], sc["proj"], np.zeros(3), sc["verts"], sc["idx"], sc["inst"][:, [3, 7, 11]], np.asarray(drawn, np.int64))
    return clip, np.repeat(sc["col"][np.asarray(drawn, np.int64)], sc["idx"].shape[0])


_cache = {}


def quad_model(w, h, fn, depth_write, drawn, key):
    """blend_model's result() of the scene: the wall FLAT, then the quads `drawn` one triangle at a time; shared, do not write to it."""
    k = (w, h, fn, depth_write, key)
    if k not in _cache:
        sc = quad_scene(w, h)
        m = B.Model(w, h, 3)
        m.draw(sc["wall"], sc["wall_col"], B.f_source)
        clip, col = quad_rows(sc, drawn)
        m.draw(clip, col, fn, depth_write)
        _cache[k] = m.result()
    return _cache[k]
