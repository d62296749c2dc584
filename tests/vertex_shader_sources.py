"""HIP C++ sources of user vertex shaders (include/trgl.h, "User vertex shaders"), for the tests, and numpy evaluations of the same
bodies in the same operation order: what trgl_vertex_stage leaves must equal them bit for bit.

Every source reads a vertex record that starts with position[3], normal[3], uv[2] (the reference's Vertex, model.h:14-20)."""
import numpy as np

_DOT4 = r"""
__device__ static double vs_dot4(const double* m, double x, double y, double z, double w) {
    double sum = 0;                                   // geometry.h:122-127: left to right, from 0
    sum += m[0] * x; sum += m[1] * y; sum += m[2] * z; sum += m[3] * w;
    return sum;
}
// clip = Perspective * (ModelView * (p, 1))
__device__ static void vs_clip(const trgl_vert_in& in, trgl_vert_out& out, double eye[4]) {
    const double* p = in.vertex;
    for (int r = 0; r < 4; ++r) eye[r] = vs_dot4(in.u->model_view + 4 * r, p[0], p[1], p[2], 1.0);
    for (int r = 0; r < 4; ++r) out.clip[r] = vs_dot4(in.projection + 4 * r, eye[0], eye[1], eye[2], eye[3]);
}
"""

# PhongShader::vertex = EyeShader::vertex (main.cpp:71-90, 199-218) - what the built-in stage of trgl_draw_indexed computes; K = 24,
# the layout uv[3] (6 doubles), position_eye[3] (9), normal_eye[3] (9)
RESTATED = _DOT4 + r"""
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* n = in.vertex + 3;
    double eye[4];
    vs_clip(in, out, eye);
    out.vary[2 * in.nth] = in.vertex[6]; out.vary[2 * in.nth + 1] = in.vertex[7];
    for (int k = 0; k < 3; ++k) {
        out.vary[6 + 3 * in.nth + k] = eye[k];
        out.vary[15 + 3 * in.nth + k] = vs_dot4(in.u->model_view + 4 * k, n[0], n[1], n[2], 0.0);
    }
}
"""

# a Gouraud vertex stage: varying_intensity[nth] = normal . key_light_dir_eye, starting at vary[OFFSET]; K = 3 + OFFSET and the
# slots ahead of OFFSET are never written
GOURAUD_TEMPLATE = _DOT4 + r"""
#define OFFSET %d
static_assert(TRGL_USER_VARY == 3 + OFFSET, "registered with another K");
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* n = in.vertex + 3; const double* l = in.u->key_light_dir_eye;
    double eye[4];
    vs_clip(in, out, eye);
    double sum = 0;
    sum += n[0] * l[0]; sum += n[1] * l[1]; sum += n[2] * l[2];
    out.vary[OFFSET + in.nth] = sum;
}
"""
GOURAUD = GOURAUD_TEMPLATE % 0
GOURAUD_PADDED = GOURAUD_TEMPLATE % 2      # K = 5, for the fragment source user_shader_sources.GOURAUD_PADDED

# K = 0: the transform alone (out.vary is null)
TRANSFORM = _DOT4 + r"""
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) { double eye[4]; vs_clip(in, out, eye); }
"""

# K = 64: slot 3 * j + nth = vertex[j % 8] * (j + 1) for j < 20, the Gouraud intensities in slots 60..62, slot 63 never written
WIDE = _DOT4 + r"""
static_assert(TRGL_USER_VARY == 64, "registered with another K");
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    const double* n = in.vertex + 3; const double* l = in.u->key_light_dir_eye;
    double eye[4];
    vs_clip(in, out, eye);
    for (int j = 0; j < 20; ++j) out.vary[3 * j + in.nth] = in.vertex[j % 8] * (double)(j + 1);
    double sum = 0;
    sum += n[0] * l[0]; sum += n[1] * l[1]; sum += n[2] * l[2];
    out.vary[60 + in.nth] = sum;
}
"""

# K = 6: what a call is told about itself (slot nth: face, slot 3 + nth: index * 4 + nth); clip = the position as it is, w = 1
ARGUMENTS = r"""
__device__ void trgl_vertex(const trgl_vert_in& in, trgl_vert_out& out) {
    for (int k = 0; k < 3; ++k) out.clip[k] = in.vertex[k];
    out.clip[3] = (double)in.stride;
    out.vary[in.nth] = (double)in.face;
    out.vary[3 + in.nth] = (double)in.index * 4.0 + (double)in.nth;
}
"""


def _dot4(m, x, y, z, w):
    """vs_dot4 for the rows of the 4x4 matrix m: a list of four arrays."""
    return [(((0.0 + m[r, 0] * x) + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] * w for r in range(4)]


def expect_clip(model_view, projection, vertices, indices):
    """vs_clip: (clip [nf, 12], eye: four [nf, 3] arrays)."""
    v = np.asarray(vertices, np.float64)[np.asarray(indices).reshape(-1, 3)]         # [nf, 3, stride]
    eye = _dot4(np.asarray(model_view, np.float64), v[..., 0], v[..., 1], v[..., 2], 1.0)
    clip = _dot4(np.asarray(projection, np.float64), *eye)
    return np.ascontiguousarray(np.stack(clip, -1).reshape(-1, 12)), eye


def expect_intensity(key, vertices, indices):
    """normal . key, left to right from 0: [nf, 3]."""
    n = np.asarray(vertices, np.float64)[np.asarray(indices).reshape(-1, 3)][..., 3:6]
    key = np.asarray(key, np.float64)
    return ((0.0 + n[..., 0] * key[0]) + n[..., 1] * key[1]) + n[..., 2] * key[2]


def expect_gouraud(model_view, projection, key, vertices, indices, offset=0):
    clip, _ = expect_clip(model_view, projection, vertices, indices)
    vary = np.zeros((clip.shape[0], 3 + offset))
    vary[:, offset:] = expect_intensity(key, vertices, indices)
    return clip, vary


def expect_wide(model_view, projection, key, vertices, indices):
    clip, _ = expect_clip(model_view, projection, vertices, indices)
    v = np.asarray(vertices, np.float64)[np.asarray(indices).reshape(-1, 3)]
    vary = np.zeros((clip.shape[0], 64))
    for j in range(20):
        vary[:, 3 * j:3 * j + 3] = v[..., j % 8] * float(j + 1)
    vary[:, 60:63] = expect_intensity(key, vertices, indices)
    return clip, vary


def expect_restated(model_view, projection, vertices, indices):
    clip, eye = expect_clip(model_view, projection, vertices, indices)
    v = np.asarray(vertices, np.float64)[np.asarray(indices).reshape(-1, 3)]
    nrm = _dot4(np.asarray(model_view, np.float64), v[..., 3], v[..., 4], v[..., 5], 0.0)
    nf = clip.shape[0]
    vary = np.concatenate([v[..., 6:8].reshape(nf, 6), np.stack(eye[:3], -1).reshape(nf, 9), np.stack(nrm[:3], -1).reshape(nf, 9)], 1)
    return clip, np.ascontiguousarray(vary)
