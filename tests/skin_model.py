"""A numpy model of trgl_skin_stage and trgl_pose_palette, written from the definitions in include/trgl.h alone: the header's
operations in the header's order, one rounding each (numpy's float64 `*`, `+`, `/` and sqrt are IEEE operations and nothing is fused).
The tests' yardstick; pinned to the reference's geometry.h by tests/golden/instance_matmul_golden.npz and skin_golden.npz."""
import numpy as np

NORMAL, TANGENT, BITANGENT = 1, 2, 4
DIR_OFFSETS = ((NORMAL, 3), (TANGENT, 8), (BITANGENT, 11))      # model.h:14-20
CANON_NAN = np.uint64(0x7FF8000000000000)


def canon(x):
    """The STORED NaNs rule: a computed NaN is stored as 0x7FF8000000000000."""
    x = np.array(x, np.float64)
    x.view(np.uint64)[np.isnan(x)] = CANON_NAN
    return x


def mat_product(a, b):
    """operator* of mat<4,4> (geometry.h:196-205): result[i][j] = 0; for k: result[i][j] += A[i][k] * B[k][j].  a, b: [..., 4, 4]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape), np.float64)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                s = np.zeros(out.shape[:-2], np.float64)
                for k in range(4):
                    s = s + a[..., i, k] * b[..., k, j]
                out[..., i, j] = s
    return out


def dot4(rows, v):
    """dot<4> (geometry.h:123-127): rows [..., 4] with v = 4 arrays (or scalars), summed from 0.0 in order."""
    s = np.zeros(rows.shape[:-1], np.float64)
    with np.errstate(all="ignore"):
        for k in range(4):
            s = s + rows[..., k] * v[k]
    return s


def blend(joints, weights, palette, skip_out_of_range=False):
    """B [n, 3, 4] for one pose: from +0.0, w_k * M_{j_k}[r][c] added in ascending k.  palette: [n_joints, 16].  skip_out_of_range: the
    device's rule for a joint number >= n_joints (the term is left out); else such a number raises."""
    joints = np.asarray(joints, np.int64)
    palette = np.asarray(palette, np.float64).reshape(-1, 16)
    n, ni = joints.shape
    B = np.zeros((n, 12), np.float64)
    with np.errstate(all="ignore"):
        for k in range(ni):
            ok = joints[:, k] < palette.shape[0]
            if not skip_out_of_range and not ok.all():
                raise ValueError("joint number out of range")
            term = weights[:, k, None] * palette[np.where(ok, joints[:, k], 0), :12]
            B = np.where(ok[:, None], B + term, B)
    return B.reshape(n, 3, 4)


def direction(B, d):
    """normalized(B * (d, 0)) (geometry.h:136-140): d [n, 3]."""
    with np.errstate(all="ignore"):
        t = np.stack([dot4(B[:, r], (d[:, 0], d[:, 1], d[:, 2], 0.0)) for r in range(3)], axis=1)
        s = np.zeros(t.shape[0], np.float64)
        for k in range(3):
            s = s + t[:, k] * t[:, k]
        length = np.sqrt(s)
        return np.where((length == 0)[:, None], t, t / length[:, None])


def skin(vertices, joints, weights, palette, flags=0, skip_out_of_range=False):
    """trgl_skin_stage: vertices [n, stride], joints [n, k], weights [n, k], palette [n_poses, n_joints, 16] -> [n_poses, n, stride]."""
    vertices = np.asarray(vertices, np.float64)
    weights = np.asarray(weights, np.float64)
    palette = np.asarray(palette, np.float64)
    palette = palette.reshape((-1,) + palette.shape[-2:])
    out = np.empty((palette.shape[0],) + vertices.shape, np.float64)
    for q in range(palette.shape[0]):
        o = vertices.copy()                                     # every other double keeps its 64 bits
        if vertices.shape[0]:
            B = blend(joints, weights, palette[q], skip_out_of_range)
            for r in range(3):
                o[:, r] = canon(dot4(B[:, r], (vertices[:, 0], vertices[:, 1], vertices[:, 2], 1.0)))
            for flag, at in DIR_OFFSETS:
                if flags & flag:
                    o[:, at:at + 3] = canon(direction(B, vertices[:, at:at + 3]))
        out[q] = o
    return out


def pose_palette(parents, local, inverse_bind=None, bad_parent_is_root=False):
    """trgl_pose_palette: local [n_poses, n_joints, 16] -> palettes [n_poses, n_joints, 16].  bad_parent_is_root: the device's rule for
    a parent that is neither -1 nor below its joint; else it raises."""
    local = np.asarray(local, np.float64)
    poses, nj = local.shape[0], local.shape[1]
    loc = local.reshape(poses, nj, 4, 4)
    world = np.empty_like(loc)
    out = np.empty_like(loc)
    for j in range(nj):
        p = int(parents[j])
        if p != -1 and not 0 <= p < j:
            if not bad_parent_is_root:
                raise ValueError("a parent must be -1 or a joint below its child")
            p = -1
        world[:, j] = loc[:, j] if p < 0 else mat_product(world[:, p], loc[:, j])
        out[:, j] = world[:, j] if inverse_bind is None else mat_product(world[:, j], np.asarray(inverse_bind, np.float64)[j].reshape(4, 4))
    return canon(out.reshape(poses, nj, 16))
