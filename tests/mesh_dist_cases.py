"""The shapes and queries of the mesh-distance tests (no test in here), all seeded and small, and the restatement's
brute-force answer of every case, computed once per process and never changed (tests/mesh_dist_f64.py)."""
import numpy as np

import mesh_dist_f64 as D
import simplify_cases as C

NAN = np.nan

# ----------------------------------------------------------------------------------------------------- one triangle ----
TRIANGLE = (np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]]), np.array([[0, 1, 2]]))
# (query, closest point written down by hand, region); every number is exact in binary
REGIONS = [
    ((-1., -1., 0.5), (0., 0., 0.), 'vertex a'),
    ((2., -0.5, 0.), (1., 0., 0.), 'vertex b'),
    ((-0.5, 2., 1.), (0., 1., 0.), 'vertex c'),
    ((0.5, -1., 0.), (0.5, 0., 0.), 'edge ab'),
    ((-1., 0.5, 2.), (0., 0.5, 0.), 'edge ac'),
    ((1., 1., 0.), (0.5, 0.5, 0.), 'edge bc'),
    ((0.25, 0.25, 3.), (0.25, 0.25, 0.), 'interior'),
    ((0.5, 0., 0.), (0.5, 0., 0.), 'on edge ab'),
    ((0., 0.25, 0.), (0., 0.25, 0.), 'on edge ac'),
    ((0.5, 0.5, 0.), (0.5, 0.5, 0.), 'on edge bc'),
    ((0., 0., 0.), (0., 0., 0.), 'on vertex a'),
    ((1., 0., 0.), (1., 0., 0.), 'on vertex b'),
    ((0., 1., 0.), (0., 1., 0.), 'on vertex c'),
    ((0.25, 0.5, 0.), (0.25, 0.5, 0.), 'in the plane, inside'),
    ((2., 2., 0.), (0.5, 0.5, 0.), 'in the plane, outside'),
    ((0., -1., 0.), (0., 0., 0.), 'between vertex a and edge ab'),
    ((1., -1., 0.), (1., 0., 0.), 'between edge ab and vertex b'),
    ((0.5, 0., 1.), (0.5, 0., 0.), 'between edge ab and the interior'),
    ((-1., 0., 0.), (0., 0., 0.), 'between vertex a and edge ac'),
    ((2., 1., 0.), (1., 0., 0.), 'between vertex b and edge bc'),
]


def triangle_queries(n, seed=0):
    """n queries around TRIANGLE: the regions and boundaries first (as many as fit), seeded random points after"""
    q = np.array([r[0] for r in REGIONS])
    rng = np.random.default_rng(seed)
    more = rng.uniform(-1.5, 2.5, (max(n - len(q), 0), 3))
    return np.concatenate([q, more])[:n] if n >= len(q) else q[:n]


# -------------------------------------------------------------------------------------------------------------- ties ----
def cube():
    v = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
         [1, 5, 7], [1, 7, 3]]
    return v, np.array(f)


def duplicates():
    """two coplanar duplicate triangles behind a third face, the duplicates in rows 1 and 2"""
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., -1.]])
    return v, np.array([[0, 1, 3], [0, 1, 2], [0, 1, 2]])


# name -> (mesh, queries, the face row that must win)
TIES = {
    'duplicates': (duplicates(), np.array([[0.25, 0.25, 1.], [0.25, 0.5, 0.], [3., 3., 0.5]]), [1, 1, 1]),
    # (0.25, 0.25, 0.5) is 0.25 from the faces x = 0 (rows 0, 1) and y = 0 (rows 4, 5): row 0 or 1 must win over 4 and 5
    'bisector': (cube(), np.array([[0.25, 0.25, 0.5], [0.75, 0.5, 0.75]]), None),
    # nearest to the edge x = 0, y = 0 (shared by rows 0 / 1 and 4 / 5) and to the corner (1,1,1) shared by six rows
    'shared_edge': (cube(), np.array([[-0.5, -0.5, 0.5], [-0.25, -0.5, 0.25], [2., 2., 2.]]), None),
}


# ----------------------------------------------------------------------------------------------------- ragged batch ----
def square(z=0.):
    v = np.array([[0., 0., z], [1., 0., z], [1., 1., z], [0., 1., z]])
    return v, np.array([[0, 1, 2], [0, 2, 3]])


def one_face():
    return np.array([[0.5, 0., 0.], [0., 2., 0.25], [-1., 0., 3.]]), np.array([[0, 1, 2]])


def bad_mesh():
    """a tetrahedron's four faces among: an index out of range, a negative index, a NaN vertex, an a == b face and a
    collinear face"""
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.], [NAN, 0.5, 0.5], [2., 0., 0.], [4., 0., 0.]])
    f = [[0, 2, 1], [1, 2, 7], [0, 1, 3], [0, 3, 4], [1, 1, 2], [1, 2, 3], [0, 5, 6], [-1, 0, 1], [0, 3, 2]]
    return v, np.array(f)


ZERO_AREA = (np.array([[0., 0., 0.], [1., 0., 0.], [2., 0., 0.], [1., 0., 0.]]), np.array([[0, 1, 2], [1, 3, 0], [2, 2, 1]]))

OBJECTS = {
    'tetrahedron': C.tetrahedron(),
    'octahedron': C.octahedron(),
    'icosphere320': C.icosphere(2, seed=1),
    'icosphere1280': C.icosphere(3, seed=2),
    'square': square(),
    'empty': C.EMPTY,
    'one_face': one_face(),
    'bad_mesh': bad_mesh(),
}
NAMES = list(OBJECTS)
WALK_CELLS = (1, 2, 7, 64)                    # the CPU test's walks
DEVICE_CELLS = (1, 2, 7, None, 64)            # the GPU test's builds


def batch(names=NAMES):
    return C.batch([OBJECTS[n] for n in names])


def object_queries(name, seed):
    """the queries of one object: inside the frame, on the surface (its own vertices, rule-D7 samples), exactly on cell
    boundary planes lo + i h, on the frame's faces and corners, 10 x the frame away along an axis and along the
    diagonal, and one with a NaN"""
    v, f = OBJECTS[name]
    tri, valid, _ = D.triangles(v, f, [0, len(v)], [0, len(f)])
    fr = D.Frame(tri, valid)
    lo, hi = fr.lo, fr.hi
    ext = hi - lo
    mid = (lo + hi) / 2
    rng = np.random.default_rng(seed)
    q = [lo + ext * rng.uniform(0, 1, (12, 3))]
    own = np.asarray(v, np.float64).reshape(-1, 3)
    q.append(own[np.isfinite(own).all(1)][:20])
    if valid.any():
        cum = D.area_prefix(tri, valid, [0, len(tri)])
        q.append(D.sample(tri, [0, len(tri)], cum, rng.uniform(0, 1, (1, 12, 3)))[0][0])
    for R in (2, 7, fr.R):
        h = ext / R
        steps = np.arange(R + 1, dtype=np.float64)[:, None]
        q.append(lo + steps * h)                                                     # on three planes at once
        q.append(np.concatenate([lo[:1] + steps * h[:1], np.broadcast_to(mid[1:], (R + 1, 2))], 1))
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    q.append(corners)
    for a in range(3):
        for side in (lo, hi):
            p = mid.copy()
            p[a] = side[a]
            q.append(p[None])
    far = 10 * np.maximum(ext, 1.)
    q.append(np.array([mid + far * [1, 0, 0], mid - far * [0, 1, 0], mid + far * [0, 0, 1], mid + far, mid - far]))
    q.append(np.array([[mid[0], NAN, mid[2]]]))
    return np.concatenate(q)


_CACHE = {}


def ragged_case():
    """-> dict: the batch (v, f, vend, tend), the queries with their objects, and the brute-force answer"""
    if 'ragged' not in _CACHE:
        v, f, vend, tend = batch()
        qs = [object_queries(n, 10 + k) for k, n in enumerate(NAMES)]
        points = np.concatenate(qs)
        obj = np.concatenate([np.full(len(q), k) for k, q in enumerate(qs)])
        b = D.Batch(v, f, vend, tend, cells=1)
        _CACHE['ragged'] = dict(v=v, f=f, vend=vend, tend=tend, points=points, obj=obj, brute=b.query(points, obj, brute=True),
                                valid=b.valid, tri=b.tri)
    return _CACHE['ragged']


def restated_batch(cells):
    """the restatement's frames and lists of the ragged batch at `cells` per axis (None: the default)"""
    key = ('batch', cells)
    if key not in _CACHE:
        v, f, vend, tend = batch()
        _CACHE[key] = D.Batch(v, f, vend, tend, cells=cells)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- known answers ----
def squares():
    """two parallel unit squares at z = 0 and z = 0.25, two triangles each"""
    return square(0.), square(0.25)
