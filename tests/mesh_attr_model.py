"""TEST INFRASTRUCTURE.  Sequential restatements in Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) of
Model::generateNormalsIfNeeded (model.cpp:269-316) and Model::computeTangentsIfNeeded (model.cpp:318-388).  tests/test_mesh_attr_cpu.py
pins both to tests/golden/mesh_attr_golden.json - results of the reference's own compiled code - so that GPU tests can check meshes
that are generated where the reference does not exist.  Records are the reference's Vertex: position +0, normal +3, texcoord +6,
tangent +8, bitangent +11."""
import math

import numpy as np


def fan_indices(nfaces, rim, seed):
    """[nfaces, 3] faces (0, a, b) around vertex 0 with a != b among the rim vertices 1..rim, from a 64-bit linear congruential
    generator in plain integers: the golden file keeps (nfaces, rim, seed) in place of the 3 * nfaces numbers."""
    x, out = seed, []
    for _ in range(nfaces):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        a = 1 + (x >> 33) % rim
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out.append([0, a, (a + (x >> 33) % (rim - 1)) % rim + 1])
    return np.array(out, np.uint32)


def load_case(g):
    """A case of tests/golden/mesh_attr_golden.json as (vertices [nv, stride], indices [nf, 3], vertices after): `out` holds the columns
    the function may write (normal, or tangent and bitangent); every other column must come back as it went in."""
    v = np.array([float.fromhex(t) for t in g["v"]], np.float64).reshape(-1, g["stride"])
    i = fan_indices(*g["i"]["fan"]) if isinstance(g["i"], dict) else np.array(g["i"], np.uint32).reshape(-1, 3)
    lo, hi = (3, 6) if g["kind"] == "normals" else (8, 14)
    want = v.copy()
    want[:, lo:hi] = np.array([float.fromhex(t) for t in g["out"]], np.float64).reshape(-1, hi - lo)
    return v, i, want


def _norm(v):                                   # geometry.h:123-133: dot summed from 0 in component order, then sqrt
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s) if s >= 0.0 else math.nan       # (a NaN sum: math.sqrt raises only for negative numbers)


def _normalized(v):                             # geometry.h:136-140
    length = _norm(v)
    if length == 0:
        return list(v)
    return [x / length for x in v]


def _needs(rows, field):
    return any(_norm(r[field:field + 3]) < 0.001 for r in rows)


def generate_normals(vertices, indices):
    """Returns (vertices after, generated) for vertices [n, stride >= 6] and indices [n_faces, 3]; the input is not changed."""
    out = np.array(vertices, np.float64, order="C")
    rows = out.tolist()
    if not _needs(rows, 3):
        return out, False
    nrm = [[0.0, 0.0, 0.0] for _ in rows]
    for i0, i1, i2 in np.asarray(indices).reshape(-1, 3).tolist():
        v0, v1, v2 = rows[i0], rows[i1], rows[i2]
        e1 = [v1[a] - v0[a] for a in range(3)]
        e2 = [v2[a] - v0[a] for a in range(3)]
        fn = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        for i in (i0, i1, i2):
            nrm[i] = [nrm[i][a] + fn[a] for a in range(3)]
    for i, s in enumerate(nrm):
        length = _norm(s)
        out[i, 3:6] = [x / length for x in s] if length > 0.001 else [0.0, 0.0, 1.0]
    return out, True


def compute_tangents(vertices, indices):
    """Returns (vertices after, generated) for vertices [n, stride >= 14] and indices [n_faces, 3]; the input is not changed."""
    out = np.array(vertices, np.float64, order="C")
    rows = out.tolist()
    if not _needs(rows, 8):
        return out, False
    tan = [[0.0, 0.0, 0.0] for _ in rows]
    for i0, i1, i2 in np.asarray(indices).reshape(-1, 3).tolist():
        v0, v1, v2 = rows[i0], rows[i1], rows[i2]
        dp1 = [v1[a] - v0[a] for a in range(3)]
        dp2 = [v2[a] - v0[a] for a in range(3)]
        duv1 = [v1[6] - v0[6], v1[7] - v0[7]]
        duv2 = [v2[6] - v0[6], v2[7] - v0[7]]
        r = duv1[0] * duv2[1] - duv2[0] * duv1[1]
        if abs(r) < 1e-8:
            continue
        invr = 1.0 / r if r != 0 else math.copysign(math.inf, r)       # (unreachable: r == 0 is skipped above)
        t = [(dp1[a] * duv2[1] - dp2[a] * duv1[1]) * invr for a in range(3)]
        for i in (i0, i1, i2):
            tan[i] = [tan[i][a] + t[a] for a in range(3)]
    for i, s in enumerate(tan):
        normal = rows[i][3:6]
        if _norm(s) > 0.001 and _norm(normal) > 0.001:
            n, t = _normalized(normal), _normalized(s)
            d = 0.0
            for a in range(3):
                d += n[a] * t[a]
            t = _normalized([t[a] - n[a] * d for a in range(3)])
            b = [normal[1] * t[2] - normal[2] * t[1], normal[2] * t[0] - normal[0] * t[2], normal[0] * t[1] - normal[1] * t[0]]
        else:
            t, b = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
        out[i, 8:11] = t
        out[i, 11:14] = b
    return out, True
