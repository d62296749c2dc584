"""What the tests of trgl_draw_instanced / trgl_instance_stage share: meshes, instance arrays, visibility patterns, the HIP sources of
user vertex shaders that read in.instance / in.inst / in.inst_stride with numpy evaluations in the same operation order, and the list
of stage shapes (the CPU tests check that the shapes reach the branches they are meant for; the GPU tests run them)."""
import collections

import numpy as np

import vertex_shader_sources as V
from tinyrenderder_amd import api, scenes

BLOCK_FACES = api.INST_VS_FACES                                   # output faces per block of the instanced vertex kernels
SCAN_BLOCK = api.INST_BLOCK                                       # instances per block of the compaction
TWO_LEVEL = api.INST_BLOCK * api.INST_SCAN_CHUNK                  # instances one block of block sums covers
BIG = TWO_LEVEL + 2 * SCAN_BLOCK + 37                             # a second chunk of block sums, with a partial last block

PATTERNS = ("absent", "all0", "all1", "first", "last", "alternating", "random")


def visible(pattern, n, seed=3):
    """None, or [n] uint8.  random: bytes over the whole 0..255 range (0xFE skips, 0xFF draws)."""
    if pattern == "absent":
        return None
    v = np.zeros(n, np.uint8)
    if pattern == "all1":
        v[:] = 1
    elif pattern == "first":
        v[:1] = 1
    elif pattern == "last":
        v[-1:] = 0xFF
    elif pattern == "alternating":
        v[::2] = 3
        v[1::2] = 2
    elif pattern == "random":
        v[:] = (scenes.SplitMix64(seed).u64(n) >> np.uint64(17)).astype(np.uint8)
        if n >= 2:
            v[0], v[1] = 0xFE, 0xFF
    else:
        assert pattern == "all0", pattern
    return v


def cube(stride=8, half=1.0):
    """A cube of side 2 * half: 8 shared vertices (position, outward normal, uv, then 0.25s) and 12 faces."""
    p = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
    n = p / np.sqrt(3.0)
    uv = (p[:, :2] + 1.0) * 0.5
    verts = np.concatenate([p * half, n, uv, np.full((8, stride - 8), 0.25)], 1)
    idx = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                   np.uint32)
    return np.ascontiguousarray(verts), idx


def mesh(nf, stride=9, seed=11):
    """nf faces over a few shared vertices: records of `stride` doubles starting with position, unit-ish normal and uv."""
    if nf == 12:
        return cube(stride, 0.5)
    rng = scenes.SplitMix64(seed + nf)
    nv = max(3, nf // 2 + 3)
    verts = np.concatenate([rng.uniform(nv * 3, -0.5, 0.5).reshape(nv, 3), rng.uniform(nv * 3, -1.0, 1.0).reshape(nv, 3),
                            rng.uniform(nv * 2, 0.0, 1.0).reshape(nv, 2), rng.uniform(nv * (stride - 8), -1.0, 1.0).reshape(nv, stride - 8)], 1)
    idx = (rng.u64(nf * 3) % np.uint64(nv)).astype(np.uint32).reshape(nf, 3)
    return np.ascontiguousarray(verts), idx


def instances(n, stride=16, seed=21, spread=0.8, scale=(0.08, 0.25)):
    """[n, stride]: a row-major model matrix (scale, a small shear, a translation), then random extras."""
    rng = scenes.SplitMix64(seed + n)
    m = np.zeros((n, stride))
    s = rng.uniform(n, *scale)
    m[:, :16] = rng.uniform(n * 16, -0.02, 0.02).reshape(n, 16)
    m[:, 0] += s; m[:, 5] += s; m[:, 10] += s
    m[:, [3, 7, 11]] = rng.uniform(n * 3, -spread, spread).reshape(n, 3)
    m[:, 12:15] = 0.0
    m[:, 15] = 1.0
    if stride > 16:
        m[:, 16:] = rng.uniform(n * (stride - 16), -2.0, 2.0).reshape(n, stride - 16)
    return np.ascontiguousarray(m)


def colors(n, seed=5, alpha=False):
    c = scenes.SplitMix64(seed + n).u64(n)
    if alpha:
        return (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return ((c & np.uint64(0xFFFFFF)) | np.uint64(0xFF000000)).astype(np.uint32)


# ---- user vertex shaders of instanced calls ---------------------------------------------------------------------------------
# every body moves the vertex by the instance's first three doubles (nothing when the call has no instances) before the transform
_INST = V._DOT4 + r"""
__device__ static void vi_clip(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* p = in.vertex;
    double q[3], eye[4];
    for (int k = 0; k < 3; ++k) q[k] = in.inst ? p[k] + in.inst[k] : p[k];
    for (int r = 0; r < 4; ++r) eye[r] = vs_dot4(in.u->model_view + 4 * r, q[0], q[1], q[2], 1.0);
    for (int r = 0; r < 4; ++r) out.clip[r] = vs_dot4(in.projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
}
// what only an instanced call can tell: its number and the last double of its record
__device__ static double vi_tail(const trgl_vert_in& in) { return in.inst ? in.inst[in.inst_stride - 1] : -1.0; }
"""
# K = 0
MOVE = _INST + r"""
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) { vi_clip(in, out); }
"""
# K = 3 + OFFSET: Gouraud intensities from OFFSET on; with OFFSET >= 2, slots 0 and 1 are per-triangle constants written by call 0 -
# the instance's ORIGINAL number and the last double of its record
GOURAUD_TEMPLATE = _INST + r"""
#define OFFSET %d
static_assert(TRGL_USER_VARY == 3 + OFFSET, "registered with another K");
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* n = in.vertex + 3; const double* l = in.u->key_light_dir_eye;
    vi_clip(in, out);
    double sum = 0;
    sum += n[0] * l[0]; sum += n[1] * l[1]; sum += n[2] * l[2];
    out.vary[OFFSET + in.nth] = sum;
#if OFFSET >= 2
    if (in.nth == 0) { out.vary[0] = (double)in.instance; out.vary[1] = vi_tail(in); }
#endif
}
"""
GOURAUD = GOURAUD_TEMPLATE % 0
GOURAUD_K5 = GOURAUD_TEMPLATE % 2
# K = 64: vertex_shader_sources.WIDE under the moved transform; slot 63 (call 0) = the record's last double + the instance's number
WIDE = _INST + r"""
static_assert(TRGL_USER_VARY == 64, "registered with another K");
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* n = in.vertex + 3; const double* l = in.u->key_light_dir_eye;
    vi_clip(in, out);
    for (int j = 0; j < 20; ++j) out.vary[3 * j + in.nth] = in.vertex[j % 8] * (double)(j + 1);
    double sum = 0;
    sum += n[0] * l[0]; sum += n[1] * l[1]; sum += n[2] * l[2];
    out.vary[60 + in.nth] = sum;
    if (in.nth == 0) out.vary[63] = vi_tail(in) + (double)in.instance;
}
"""
STAGES = {"k0": (MOVE, 0), "k5": (GOURAUD_K5, 5), "k64": (WIDE, 64), "k3": (GOURAUD, 3)}


def expect_user(stage, model_view, projection, key, vertices, indices, inst, drawn):
    """(clip [len(drawn) * nf, 12], varyings [.., K] or None) of STAGES[stage]; inst: [n, stride] or None; drawn: original numbers."""
    idx = np.asarray(indices).reshape(-1, 3)
    nf, nd = idx.shape[0], len(drawn)
    v = np.asarray(vertices, np.float64)[idx]                                   # [nf, 3, stride]
    q = np.broadcast_to(v[None, ..., :3], (nd, nf, 3, 3))
    if inst is not None:
        q = v[None, ..., :3] + np.asarray(inst, np.float64)[drawn][:, None, None, :3]
    eye = V._dot4(np.asarray(model_view, np.float64), q[..., 0], q[..., 1], q[..., 2], 1.0)
    clip = np.ascontiguousarray(np.stack(V._dot4(np.asarray(projection, np.float64), *eye), -1).reshape(nd * nf, 12))
    K = STAGES[stage][1]
    if K == 0:
        return clip, None
    vary = np.zeros((nd, nf, K))
    tail = np.full(nd, -1.0) if inst is None else np.asarray(inst, np.float64)[drawn, -1]
    number = np.asarray(drawn, np.float64)
    inten = V.expect_intensity(key, vertices, idx)                              # [nf, 3]
    if stage in ("k3", "k5"):
        vary[..., K - 3:] = inten[None]
        if stage == "k5":
            vary[..., 0] = number[:, None]
            vary[..., 1] = tail[:, None]
    else:
        for j in range(20):
            vary[..., 3 * j:3 * j + 3] = (v[..., j % 8] * float(j + 1))[None]
        vary[..., 60:63] = inten[None]
        vary[..., 63] = (tail + number)[:, None]
    return clip, np.ascontiguousarray(vary.reshape(nd * nf, K))


# ---- the stage shapes --------------------------------------------------------------------------------------------------------
# stage: "builtin" or a key of STAGES; colors: None, "face" or "instance"; stride: doubles per instance (0: the call has no instances)
Shape = collections.namedtuple("Shape", "stage nf n pattern stride inst_device colors")
SHAPES = {
    "builtin_box_257_random_host": Shape("builtin", 12, 257, "random", 16, False, "face"),
    "builtin_box_257_random_device_s19": Shape("builtin", 12, 257, "random", 19, True, "instance"),
    "builtin_37f_3_absent_device": Shape("builtin", 37, 3, "absent", 16, True, None),
    "builtin_1f_big_alternating_device": Shape("builtin", 1, BIG, "alternating", 16, True, "instance"),
    "builtin_65f_1_all1_host": Shape("builtin", 65, 1, "all1", 19, False, None),
    "builtin_64f_64_first_device": Shape("builtin", 64, 64, "first", 16, True, "face"),
    "builtin_box_0_host": Shape("builtin", 12, 0, "absent", 16, False, None),
    "builtin_box_0_device": Shape("builtin", 12, 0, "all1", 16, True, "instance"),
    "k5_37f_3_all1_device_s19": Shape("k5", 37, 3, "all1", 19, True, None),
    "k5_2f_257_random_host_s19": Shape("k5", 2, 257, "random", 19, False, "instance"),
    "k5_box_257_alternating_device": Shape("k5", 12, 257, "alternating", 16, True, "face"),
    "k0_2f_64_last_device": Shape("k0", 2, 64, "last", 16, True, "instance"),
    "k0_box_3_alternating_no_instances": Shape("k0", 12, 3, "alternating", 0, True, "instance"),
    "k0_37f_64_random_host_s19": Shape("k0", 37, 64, "random", 19, False, "face"),
    "k0_1f_big_random_device": Shape("k0", 1, BIG, "random", 16, True, None),
    "k64_65f_3_absent_host": Shape("k64", 65, 3, "absent", 16, False, "face"),
    "k64_1f_257_all0_device": Shape("k64", 1, 257, "all0", 16, True, None),
    "k64_2f_64_all1_host_s19": Shape("k64", 2, 64, "all1", 19, False, None),
}


def shape_inputs(s):
    """(vertices, indices, instances or None, visible or None, face_colors or None, instance_colors or None) of a Shape."""
    verts, idx = mesh(s.nf)
    inst = instances(s.n, s.stride) if s.stride else None
    vis = visible(s.pattern, s.n)
    fc = colors(s.nf, 7) if s.colors == "face" else None
    ic = colors(s.n, 9) if s.colors == "instance" else None
    return verts, idx, inst, vis, fc, ic
