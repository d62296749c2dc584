"""A restatement in Python of the reference's scene logic around the draws, for the tests of the scene entry points:
Model::computeAABB (model.cpp:15-40), AABB::transform (geometry.h:297-327), Plane::distance (geometry.h:264-266),
Frustum::createFromMatrix and Frustum::intersects (our_gl.cpp:212-280), and the culling bookkeeping of main.cpp:623-736,794-799.

Python floats are IEEE doubles and every operation below is a single rounded one, in the reference's order, so the results are meant
to be bit-identical; tests/test_scene_cpu.py holds this file to goldens made by the reference's compiled code."""
import math

import numpy as np


def std_min(a, b):
    """std::min(a, b): b when b < a, else a (a is the running bound: a NaN b never replaces it, an equal b neither)."""
    return b if b < a else a


def std_max(a, b):
    """std::max(a, b): b when a < b, else a."""
    return b if a < b else a


def _dot(a, b):
    s = 0.0                                   # geometry.h:122-127: from 0, left to right
    for x, y in zip(a, b):
        s += x * y
    return s


def compute_aabb(vertices):
    """Model::computeAABB (model.cpp:15-40) of vertices [n, stride >= 3], position at +0: (min[3], max[3]) of localAABB."""
    v = np.asarray(vertices, np.float64)
    if v.shape[0] == 0:
        return np.zeros(3), np.zeros(3)       # :16-19
    lo, hi = [1e9] * 3, [-1e9] * 3            # :21-22
    for a in range(3):
        for p in v[:, a].tolist():
            lo[a] = std_min(lo[a], p)         # :25-27
            hi[a] = std_max(hi[a], p)         # :29-31
    out_lo, out_hi = np.empty(3), np.empty(3)
    for a in range(3):
        margin = (hi[a] - lo[a]) * 0.01       # :35
        out_lo[a] = lo[a] - margin            # :36
        out_hi[a] = hi[a] + margin
    return out_lo, out_hi


def aabb_transform(bmin, bmax, m):
    """AABB::transform (geometry.h:297-327)."""
    bmin, bmax = [float(x) for x in bmin], [float(x) for x in bmax]
    m = np.asarray(m, np.float64).reshape(4, 4).tolist()
    lo, hi = [1e9] * 3, [-1e9] * 3
    for i in range(8):                        # :300-307
        corner = [bmax[0] if i & 1 else bmin[0], bmax[1] if i & 2 else bmin[1], bmax[2] if i & 4 else bmin[2], 1.0]
        t = [_dot(m[r], corner) for r in range(4)]                     # :314
        with np.errstate(all="ignore"):
            pos = (np.array(t[:3], np.float64) / np.float64(t[3])).tolist()   # :315, IEEE division: x / 0 is inf or NaN, no exception
        for a in range(3):
            lo[a] = std_min(lo[a], pos[a])
            hi[a] = std_max(hi[a], pos[a])
    return np.array(lo), np.array(hi)


def frustum_from_matrix(m):
    """Frustum::createFromMatrix (our_gl.cpp:212-262): planes [6, 4] = nx, ny, nz, d; LEFT, RIGHT, BOTTOM, TOP, NEAR, FAR."""
    m = np.asarray(m, np.float64).reshape(4, 4).tolist()
    planes = []
    for k in range(3):
        planes.append([m[r][3] + m[r][k] for r in range(4)])           # :217-220 and the like: rows 0..2 the normal, row 3 d
        planes.append([m[r][3] - m[r][k] for r in range(4)])
    for pl in planes:                                                  # :253-259
        length = math.sqrt(_dot(pl[:3], pl[:3]))
        if length > 0.0:
            for j in range(4):
                pl[j] = pl[j] / length
    return np.array(planes, np.float64)


def frustum_intersects(planes, bmin, bmax):
    """Frustum::intersects (our_gl.cpp:264-280)."""
    planes = np.asarray(planes, np.float64).reshape(6, 4).tolist()
    bmin, bmax = [float(x) for x in bmin], [float(x) for x in bmax]
    for pl in planes:
        positive = [bmax[a] if pl[a] >= 0 else bmin[a] for a in range(3)]     # :269-272
        if _dot(pl[:3], positive) + pl[3] < 0:                                # :275
            return False
    return True


def cull_scene(view_projection, models):
    """main.cpp:623-736 for models = [(vertices, n_faces, model_matrix), ...], each tested on its own: the visible flags and the
    counters that main.cpp:794-799 prints."""
    planes = frustum_from_matrix(view_projection)
    stats = dict(models_rendered=0, models_culled=0, total_triangles=0, culled_triangles=0)
    visible = []
    for vertices, n_faces, model_matrix in models:
        world = aabb_transform(*compute_aabb(vertices), model_matrix)  # Model::getWorldAABB
        vis = frustum_intersects(planes, *world)
        visible.append(vis)
        if vis:
            stats["models_rendered"] += 1
            stats["total_triangles"] += n_faces
        else:
            stats["models_culled"] += 1
            stats["culled_triangles"] += n_faces
    return visible, stats


def format_culling_stats(stats):
    """The lines of main.cpp:794-799, without the efficiency line."""
    return ("\n=== Frustum Culling Statistics ===\n"
            f"  Total models: {stats['models_rendered'] + stats['models_culled']}\n"
            f"  Models rendered: {stats['models_rendered']}\n"
            f"  Models culled: {stats['models_culled']}\n"
            f"  Total triangles: {stats['total_triangles']}\n"
            f"  Culled triangles: {stats['culled_triangles']}\n")
