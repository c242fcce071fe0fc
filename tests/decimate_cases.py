"""Meshes of the decimation tests (no test in here; tests/test_decimate_cpu.py and tests/test_gpu_decimate.py import
it): small, built once, never changed.  Every builder returns (vertices (n,3) f64, faces (m,3) int64, local indices)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_ref  # noqa: E402

LATTICE = 16                    # the marching-cubes meshes live in the padded index space [0, LATTICE + 1]^3
CUBE_SIDE = LATTICE + 2.0       # lo = 0, h = CUBE_SIDE / cells covers it


@functools.lru_cache(maxsize=None)
def _implicit(radii, centre):
    g = np.stack(np.meshgrid(*[np.arange(LATTICE, dtype=np.float64)] * 3, indexing='ij'), -1)
    field = 1.0 - np.sqrt((((g - np.asarray(centre)) / np.asarray(radii)) ** 2).sum(-1))
    v, f = mc_ref.index_soup(mc_ref.marching_cubes_soup(field, 0.0))
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f.astype(np.int64)


def sphere():
    """a closed marching-cubes sphere on the 16^3 lattice (about 1 100 faces); many vertices on lattice planes"""
    return _implicit((5.5, 5.5, 5.5), (7.5, 7.5, 7.5))


def ellipsoid():
    return _implicit((6.3, 4.1, 3.2), (7.2, 7.9, 7.4))


def unit_cube():
    """the cube [0.2, 0.8]^3 inside the unit cube: vertex i at corner ((i & 1), (i >> 1) & 1, (i >> 2)), twelve triangles"""
    v = np.array([[0.2 + 0.6 * (i & 1), 0.2 + 0.6 * ((i >> 1) & 1), 0.2 + 0.6 * (i >> 2)] for i in range(8)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3],
                  [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]], np.int64)
    return v, f


def fan(n_faces, z=0.3, hub=(0., 0., 0.), phase=0.):
    """n_faces triangles around vertex 0 at `hub`, their outer vertices on the unit circle lifted by z sin(3 t): the
    hub has exactly n_faces corners"""
    t = phase + 2 * np.pi * np.arange(n_faces + 1) / (n_faces + 1.5)
    rim = np.stack([np.cos(t), np.sin(t), z * np.sin(3 * t)], 1)
    v = np.concatenate([np.asarray(hub, np.float64).reshape(1, 3), rim])
    f = np.stack([np.zeros(n_faces, np.int64), np.arange(1, n_faces + 1), np.arange(2, n_faces + 2)], 1)
    return v, f


def two_hubs(n_corners):
    """ONE mesh of two fans whose hubs share the cell around the origin of a grid with h = 0.5 centred there (and nothing
    else does): that cell visits exactly n_corners corners, of planes that do not meet in a point, so every corner's
    weight shows in its position"""
    first = (n_corners + 1) // 2
    a = fan(first, 0.3, (0.1, -0.07, 0.05))
    parts = [a] if n_corners == first else [a, fan(n_corners - first, -0.25, (-0.12, 0.08, -0.1), 0.4)]
    v = np.concatenate([p[0] for p in parts])
    f = np.concatenate([p[1] + off for p, off in zip(parts, [0, len(a[0])])])
    return v, f


def slab(n=6, thickness=0.02, thick_from=4, top=0.8):
    """a closed box, x and y in [0, n]: two n x n sheets of quads and the rim between them.  The sheets lie at
    z = +-thickness / 2, except that the upper one rises to z = top in the columns x >= thick_from: with unit cells from
    (-0.5, -0.5, -0.5) the thin part's two sides fall into the same cells, the thick part's do not"""
    idx = lambda i, j, s: (s * (n + 1) + j) * (n + 1) + i
    v = np.array([[i, j, top if s == 1 and i >= thick_from else (s - 0.5) * thickness]
                  for s in range(2) for j in range(n + 1) for i in range(n + 1)], np.float64)
    f = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j, 1), idx(i + 1, j, 1), idx(i + 1, j + 1, 1), idx(i, j + 1, 1)
            f += [[a, b, c], [a, c, d]]
            a, b, c, d = idx(i, j, 0), idx(i + 1, j, 0), idx(i + 1, j + 1, 0), idx(i, j + 1, 0)
            f += [[a, c, b], [a, d, c]]
    rim = [(i, 0) for i in range(n)] + [(n, j) for j in range(n)] + [(i, n) for i in range(n, 0, -1)] + \
          [(0, j) for j in range(n, 0, -1)]
    for (i0, j0), (i1, j1) in zip(rim, rim[1:] + rim[:1]):
        a, b, c, d = idx(i0, j0, 0), idx(i1, j1, 0), idx(i1, j1, 1), idx(i0, j0, 1)
        f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int64)


def batch(meshes):
    """[(v, f)] -> (v (V,3) f64, f (F,3) int64 local, vend, tend)"""
    vend = np.concatenate([[0], np.cumsum([np.asarray(m[0]).reshape(-1, 3).shape[0] for m in meshes])]).astype(int).tolist()
    tend = np.concatenate([[0], np.cumsum([np.asarray(m[1]).reshape(-1, 3).shape[0] for m in meshes])]).astype(int).tolist()
    v = np.concatenate([np.asarray(m[0], np.float64).reshape(-1, 3) for m in meshes])
    f = np.concatenate([np.asarray(m[1], np.int64).reshape(-1, 3) for m in meshes])
    return v, f, vend, tend
