"""Cases of the mesh-sampling tests (no test in here; tests/golden/make_sample_fixture.py, tests/test_mesh_sample_cpu.py
and tests/test_gpu_mesh_sample.py import it): how the fixture's meshes and query points are made, so that the fixture
stores the reference's answers and the shared random arrays only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F_SMP.npz")
MESHES = ("sphere", "ellipsoid", "unit_cube")
HASH_RESOLUTIONS = (512, 16, 2)
SURFACE_RESOLUTIONS = (7, 16, 33)
GRID = 16
BINVOX_TRANSLATE, BINVOX_SCALE = (0.1, -0.2, 0.3), 1.7


def normalised(name):
    """a mesh of decimate_cases moved into the cube: (V - centre of the bounding box) / largest extent * 0.9"""
    v, f = getattr(decimate_cases, name)()[:2]
    v = np.asarray(v, np.float64)
    lo, hi = v.min(0), v.max(0)
    return (v - (lo + hi) / 2) / (hi - lo).max() * 0.9, np.asarray(f, np.int64)


def grid_centres(resolution):
    c = (np.arange(resolution, dtype=np.float64) + 0.5) / resolution - 0.5
    return np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)


def jittered_centres(resolution, jitter):
    c = np.arange(resolution, dtype=np.float64) + 0.5
    return (np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3) + jitter) / resolution - 0.5


def query_points(v, f, jitter, uniform):
    """the points every containment case asks about: lattice centres (rays through vertices and along axis-aligned
    faces), jittered centres, vertices, face centroids, edge midpoints, uniform points, the bounding box's corners and
    centre, a NaN and a point far outside"""
    tri = v[f]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    return np.concatenate([
        grid_centres(GRID), jittered_centres(GRID, jitter), v[:200], ((tri[:, 0] + tri[:, 1]) + tri[:, 2])[:200] / 3,
        ((tri[:, 0] + tri[:, 1]) / 2)[:200], uniform, lo[None], hi[None], ((lo + hi) / 2)[None],
        np.full((1, 3), np.nan), np.full((1, 3), 10.)])


def cube():
    """the unit cube of decimate_cases as it is: [0.2, 0.8]^3"""
    v, f = decimate_cases.unit_cube()
    return np.asarray(v, np.float64), np.asarray(f, np.int64)
