"""Meshes for the subdivision tests (tests/test_subdiv.py, tests/test_subdiv_gpu.py): those of tests/edge_cases.py, cones - an interior
hub of any valence inside a boundary -, isolated vertices, a bow-tie corner and a regular grid with integer coordinates.  Every mesh is
(vertices [nv, stride] float64, indices [F, 3] uint32, nv)."""
import numpy as np

import edge_cases as EC

SENTINEL_U32 = EC.SENTINEL_U32
SENTINEL_F64_BITS = 0x7FF4A5A5A5A5A5A5          # a NaN with a payload: a copy keeps it, nothing computed makes it
CONE_SIZES = [3, 4, 6, 7, 64, 65, 1000]          # valence 3 and 4: either side of the switch of beta; 64, 65: a wave of ring entries
STRIDES = [(3, 3), (3, 0), (5, 3), (5, 0), (5, 5), (8, 0), (8, 8), (14, 3), (14, 14), (14, 0)]      # (vertex_stride, smooth): 24- to 112-byte records


def restride(mesh, stride, seed=5):
    """the mesh with records of `stride` doubles: its positions, then noise"""
    v, idx, nv = mesh
    pos = np.zeros((nv, 3)) if v is None else np.asarray(v)[:, :3]
    if stride < 3:
        return np.ascontiguousarray(pos[:, :stride]), idx, nv
    return EC._pad(pos, stride, seed), idx, nv


def cone(n, stride=3):
    """a hub (vertex 0) and n rim vertices, open at the rim: the hub is interior with valence n, the rim vertices lie on the boundary"""
    t = 2.0 * np.pi * np.arange(n) / n
    pos = np.concatenate([[[0.0, 0.0, 1.0]], np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3.0 * t)], 1)])
    idx = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)]
    return EC._pad(pos, stride), np.array(idx, np.uint32), n + 1


def isolated(stride=3):
    """a tetrahedron over the vertices 0, 2, 4, 6 of seven: 1, 3 and 5 belong to no face"""
    v, idx, _ = EC.tetrahedron()
    pos = np.zeros((7, 3))
    pos[::2] = v[:, :3]
    pos[1::2] = [[5, 5, 5], [-6, 7, 8], [9, -9, 9]]
    return EC._pad(pos, stride), (idx * 2).astype(np.uint32), 7


def bowtie(stride=3):
    """two triangles that share vertex 0 only: four boundary edges meet there, a corner"""
    pos = [[0, 0, 0], [1, 1, 0], [1, -1, 0.5], [-1, -1, 0], [-1, 1, -0.5]]
    return EC._pad(pos, stride), np.array([[0, 1, 2], [0, 3, 4]], np.uint32), 5


def integer_grid(m, n, stride=3):
    """EC.grid with every coordinate a multiple of 16 and a sheared height: each interior vertex has valence 6"""
    v, idx, nv = EC.grid(m, n, 3)
    pos = 16.0 * v[:, :3]
    pos[:, 2] = 16.0 * (v[:, 0] + 2.0 * v[:, 1])
    return EC._pad(pos, stride), idx, nv


def named():
    """the small meshes every test walks"""
    out = dict(EC.named())
    out.update({"cone3": cone(3), "cone4": cone(4, 5), "cone7": cone(7, 8), "isolated": isolated(4), "bowtie": bowtie(),
                "integer_grid": integer_grid(5, 4)})
    return out


CLOSED = ("tetrahedron", "cube", "icosphere")
