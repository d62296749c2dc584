"""A numpy model of trgl_draw_instanced / trgl_instance_stage, written from the definition in include/trgl.h alone.

Instance i is drawn when visible is None or visible[i] & 1; the drawn ones keep their order.  Output triangle j * nf + f is face f under
the j-th drawn instance.  Built-in stage: MV_i = model_view * M_i (geometry.h:196-205: every element summed from 0.0, k ascending), rows
those of orc.vertex_stage under MV_i.  Colour: instance_colors[i], else face_colors[f], else none."""
import numpy as np

from oracle import orc


def mat_product(a, b):
    """geometry.h:196-205 in explicit loops: result[i][j] = 0; for k: result[i][j] += A[i][k] * B[k][j] - fp64, one rounding per
    product and per sum.  a: one matrix (16 doubles); b: one, or [n, 16] of them (the loops then run over all n at once)."""
    a = np.asarray(a, np.float64).reshape(4, 4)
    b = np.asarray(b, np.float64)
    b = b.reshape(b.shape[:-1] + (4, 4)) if b.shape[-1] == 16 else b
    out = np.zeros(b.shape, np.float64)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                s = np.zeros(b.shape[:-2], np.float64)
                for k in range(4):
                    s = s + a[i, k] * b[..., k, j]
                out[..., i, j] = s
    return out


def compact(visible, n):
    """The original numbers of the drawn instances, ascending."""
    if visible is None:
        return np.arange(n, dtype=np.int64)
    visible = np.asarray(visible, np.uint8)
    assert visible.shape == (n,)
    return np.flatnonzero(visible & 1)


def colors(drawn, nf, face_colors=None, instance_colors=None):
    """[len(drawn) * nf] uint32, or None when the call has no colours."""
    assert face_colors is None or instance_colors is None
    if instance_colors is not None:
        return np.repeat(np.asarray(instance_colors, np.uint32)[drawn], nf)
    if face_colors is not None:
        return np.tile(np.asarray(face_colors, np.uint32), len(drawn))
    return None


def builtin_rows(model_view, projection, vertices, indices, instances, visible=None):
    """(clip [n_vis * nf, 12], varyings [n_vis * nf, 24], drawn) of the built-in stage; instances [n, stride >= 16]."""
    instances = np.asarray(instances, np.float64)
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    nf = idx.shape[0]
    drawn = compact(visible, instances.shape[0])
    clip = np.zeros((len(drawn) * nf, 12))
    vary = np.zeros((len(drawn) * nf, 24))
    mvs = mat_product(model_view, instances[drawn, :16])
    for j in range(len(drawn)):
        clip[j * nf:(j + 1) * nf], vary[j * nf:(j + 1) * nf] = orc.vertex_stage(mvs[j], projection, vertices, idx)
    return clip, vary, drawn
