"""The inputs of tests/test_knn_cpu.py and tests/test_gpu_knn.py (no test in here): small point sets, a lattice whose
queries meet exact ties, sets for every cell count, a ragged batch, bounds and masks.  Everything is float64 and seeded;
nothing here imports the package."""
import numpy as np

SMALL_SIZES = (1, 7, 33)
SMALL_K = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)           # both edges of every kernel instance (1, 4, 8, 16, 32 slots)
SMALL_QUERIES = (1, 63, 65, 255, 256, 257)
CELLS = (1, 2, 3, 5, 64)


def small_set(n):
    return np.random.default_rng(100 + n).uniform(-1., 1., (n, 3))


def small_queries(count=257):
    return np.random.default_rng(7).normal(0., 0.8, (count, 3))


# ties ------------------------------------------------------------------------------------------------------------------
LATTICE_N = 6


def lattice():
    """the 6 x 6 x 6 integer lattice, row (ix 6 + iy) 6 + iz"""
    g = np.arange(LATTICE_N, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def lattice_queries():
    """-> {name: (queries, the number of points tied for the nearest place)}: edge midpoints (2), face centres (4), body
    centres (8), and lattice points, whose second to seventh neighbours tie (6, asked for with k >= 2)"""
    inner = np.stack(np.meshgrid(*[np.arange(1., 4.)] * 3, indexing='ij'), -1).reshape(-1, 3)
    return {
        'edge': (inner + [0.5, 0., 0.], 2),
        'face': (inner + [0.5, 0.5, 0.], 4),
        'body': (inner + [0.5, 0.5, 0.5], 8),
        'point': (inner, 6),
    }


DUPLICATES = 40
DUPLICATE_AT = (2., 3., 1.)


def lattice_with_duplicates():
    """the lattice, then 40 more points at one lattice position: 41 rows at distance 0 of a query there"""
    return np.concatenate([lattice(), np.tile(np.array(DUPLICATE_AT), (DUPLICATES, 1))])


# every R ---------------------------------------------------------------------------------------------------------------
def frame_sets():
    """-> {name: points}: a filled box, a coplanar and a collinear set (zero-extent axes), one point, no point"""
    rng = np.random.default_rng(11)
    box = rng.uniform([-1., 0., 2.], [3., 1., 2.5], (150, 3))
    plane = box[:60].copy()
    plane[:, 2] = 2.25
    line = box[:40].copy()
    line[:, 1], line[:, 2] = 0.5, 2.25
    return {'box': box, 'plane': plane, 'line': line, 'single': np.array([[0.25, -0.5, 1.]]), 'empty': np.zeros((0, 3))}


def frame_queries(points):
    """queries inside the frame of `points`, on its faces, 10 extents outside it, and at 1e300"""
    rng = np.random.default_rng(12)
    lo = points.min(0) if len(points) else np.zeros(3)
    hi = points.max(0) if len(points) else np.zeros(3)
    ext = np.where(hi > lo, hi - lo, 1.)
    inside = lo + rng.uniform(0., 1., (24, 3)) * (hi - lo)
    faces = lo + rng.uniform(0., 1., (12, 3)) * (hi - lo)
    for i in range(12):
        faces[i, i % 3] = (lo, hi)[(i // 3) % 2][i % 3]
    outside = lo + (hi - lo) / 2 + rng.choice([-10., 0., 10.], (16, 3)) * ext + rng.uniform(-0.5, 0.5, (16, 3)) * ext
    far = np.array([[1e300, 0., 0.], [0., -1e300, 0.], [1e300, 1e300, 1e300], [-1e300, 0.5, 1e300]])
    return np.concatenate([inside, faces, outside, far])


# ragged ----------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = (0, 1, 40, 300, 2000)


def ragged_case(order=None):
    """K = 5 sets of 0, 1, 40, 300 and 2 000 points, each in a box of its own, and 700 queries of mixed sets -> a dict;
    `order`: the sets laid out in that order (the queries' objects are renamed with them)"""
    rng = np.random.default_rng(21)
    sets = [rng.uniform(-1., 1., (n, 3)) * rng.uniform(0.5, 2., 3) + rng.uniform(-3., 3., 3) for n in RAGGED_SIZES]
    obj = rng.integers(0, len(sets), 700)
    centre = np.array([s.mean(0) if len(s) else np.zeros(3) for s in sets])
    queries = centre[obj] + rng.normal(0., 1.2, (700, 3))
    order = list(range(len(sets))) if order is None else list(order)
    rename = np.argsort(order)                                  # set j of the canonical batch is set rename[j] of this one
    sizes = [len(sets[j]) for j in order]
    return {'sets': sets, 'points': np.concatenate([sets[j] for j in order]), 'pend': np.concatenate([[0], np.cumsum(sizes)]),
            'queries': queries, 'obj': rename[obj], 'canonical_obj': obj, 'order': order}


# bounds and masks ------------------------------------------------------------------------------------------------------
def axis_points():
    """points on the x axis at distances of a query at the origin that are exact in binary: 0.125, 0.25, 0.5, 0.5, 1, 2, 4"""
    x = np.array([0.125, -0.25, 0.5, -0.5, 1., -2., 4.])
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)


# metrics ---------------------------------------------------------------------------------------------------------------
def cube_samples(n, seed, shift=0.):
    """n points on the surface of the unit cube [0,1]^3 (+ shift along x) with their outward normals"""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, 6, n)
    p = rng.uniform(0., 1., (n, 3))
    normals = np.zeros((n, 3))
    axis, side = face % 3, face // 3
    p[np.arange(n), axis] = side
    normals[np.arange(n), axis] = 2. * side - 1.
    p[:, 0] += shift
    return p, normals


def sphere_samples(n, seed, radius=0.5, centre=(0.5, 0.5, 0.5)):
    rng = np.random.default_rng(seed)
    normals = rng.normal(size=(n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return np.asarray(centre) + radius * normals, normals


# the larger size -------------------------------------------------------------------------------------------------------
def large_case(dtype=np.float64):
    """default_rng(0): 20 000 uniform data points in [0,1)^3, 4 096 queries in [-0.2, 1.2)^3"""
    rng = np.random.default_rng(0)
    data = rng.uniform(0., 1., (20000, 3)).astype(dtype)
    queries = rng.uniform(-0.2, 1.2, (4096, 3)).astype(dtype)
    return data, queries
