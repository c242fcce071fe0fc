"""The shapes of the simplification tests (no test in here), all seeded and small, the checks both test files share, and
the restatement's result of every case, computed once per process (tests/simplify_f64.py)."""
import numpy as np

import simplify_f64 as S


def tetrahedron():
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def octahedron():
    v = np.array([[1., 0., 0.], [-1., 0., 0.], [0., 1.25, 0.], [0., -1., 0.], [0., 0., 1.5], [0., 0., -0.75]])
    return v, np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def icosphere(level, noise=0.05, seed=0):
    """20 * 4^level faces, radius 0.4 (1 + noise * U(-1, 1)) per vertex"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(v)
                v.append((v[a] + v[b]) / 2)
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    v = np.array(v)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    return v * (0.4 * (1 + noise * rng.uniform(-1, 1, (len(v), 1)))), np.array(f)


def torus(nu=16, nv=8, R=0.35, r=0.12):
    """nu x nv quads, two faces each; genus 1"""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3)
    f = []
    for x in range(nu):
        for y in range(nv):
            p, q, s, t = x * nv + y, ((x + 1) % nu) * nv + y, ((x + 1) % nu) * nv + (y + 1) % nv, x * nv + (y + 1) % nv
            f += [(p, q, s), (p, s, t)]
    return v, np.array(f)


def grid(nx, ny):
    f = []
    for x in range(nx - 1):
        for y in range(ny - 1):
            p = x * ny + y
            f += [(p, p + ny, p + ny + 1), (p, p + ny + 1, p + 1)]
    i, j = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    return np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3), np.array(f)


def patch(seed=1):
    """9 x 9 vertices, open, noise in z"""
    v, f = grid(9, 9)
    v[:, 2] = np.random.default_rng(seed).uniform(-0.2, 0.2, len(v))
    return v * 0.1, f


def folded_strip(seed=0):
    """9 x 5 vertices folded along x = 4, jittered in the plane by up to 0.4 of a cell: many collapses would turn a face over"""
    v, f = grid(9, 5)
    rng = np.random.default_rng(seed)
    v[:, :2] += rng.uniform(-0.4, 0.4, (len(v), 2))
    v[:, 2] = 0.5 * np.abs(v[:, 0] - 4.0)
    return v * 0.1, f


def two_tetrahedra():
    """two tetrahedra that share the edge 0-1: a non-manifold edge of four faces"""
    v = np.array([[0., 0., 0.], [0., 0., 1.], [1., 0., 0.5], [0.5, 1., 0.5], [-1., 0., 0.5], [-0.5, -1., 0.5]])
    f = [[0, 1, 2], [1, 0, 3], [0, 2, 3], [2, 1, 3], [1, 0, 4], [0, 1, 5], [0, 4, 5], [4, 1, 5]]
    return v, np.array(f)


def bad_input():
    """an icosphere with a face that repeats an index, two with an index out of range and a NaN vertex"""
    v, f = icosphere(1, seed=5)
    v, f = v.copy(), f.copy()
    f[3, 1] = f[3, 0]
    f[10, 2] = len(v)
    f[40, 0] = -1
    v[20, 1] = np.nan
    return v, f


EMPTY = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))

# name -> (mesh, target)
CASES = {
    'tetrahedron': (tetrahedron(), 2),
    'octahedron': (octahedron(), 6),
    'icosphere320': (icosphere(2, seed=1), 100),
    'icosphere1280': (icosphere(3, seed=2), 400),
    'torus': (torus(), 64),
    'icosphere5120': (icosphere(4, seed=3), 500),
    'patch': (patch(), 40),
    'two_tetrahedra': (two_tetrahedra(), 4),
    'bad_input': (bad_input(), 30),
    'empty': (EMPTY, 10),
    'folded_strip': (folded_strip(), 24),
}
CLOSED = ('tetrahedron', 'octahedron', 'icosphere320', 'icosphere1280', 'torus', 'icosphere5120')

_RESULTS = {}


def restated(name):
    """the restatement's result of a case -> (dict, trace); computed once, never changed"""
    if name not in _RESULTS:
        (v, f), target = CASES[name]
        trace = []
        _RESULTS[name] = (S.simplify(v, f, target, trace=trace), trace)
    return _RESULTS[name]


def batch(meshes):
    """[(v, f), ...] -> (v, f, vend, tend) of the ragged batch"""
    vend, tend = [0], [0]
    for v, f in meshes:
        vend.append(vend[-1] + len(v))
        tend.append(tend[-1] + len(f))
    return (np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _ in meshes]),
            np.concatenate([np.asarray(f, np.int64).reshape(-1, 3) for _, f in meshes]), vend, tend)


# ------------------------------------------------------------------------------------------------------ the checks ----
def directed_edges(f):
    f = np.asarray(f).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist()


def border_vertices(f):
    """the vertices of every edge that does not have exactly two faces"""
    count = {}
    for a, b in directed_edges(f):
        count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    return sorted(set(i for e, n in count.items() if n != 2 for i in e))


def is_closed_oriented_manifold(f):
    """every directed edge once, its reverse present, and the faces around every vertex one single fan"""
    f = np.asarray(f).reshape(-1, 3)
    e = directed_edges(f)
    de = set(map(tuple, e))
    if len(de) != len(e) or not all((b, a) in de for a, b in de):
        return False
    nxt = {}
    for a, b, c in f.tolist():
        for u, w, x in ((a, b, c), (b, c, a), (c, a, b)):
            nxt[(u, w)] = x                                     # around u: after the neighbour w comes x
    faces_at = np.bincount(f.reshape(-1))
    first = {}
    for (u, w) in nxt:
        first.setdefault(u, w)
    for u, start in first.items():
        w, steps = nxt[(u, start)], 1
        while w != start and steps <= faces_at[u]:
            w, steps = nxt[(u, w)], steps + 1
        if steps != faces_at[u]:
            return False
    return True


def euler(f):
    f = np.asarray(f).reshape(-1, 3)
    edges = set((min(a, b), max(a, b)) for a, b in directed_edges(f))
    return len(set(f.reshape(-1).tolist())) - len(edges) + len(f)


def no_degenerate_or_duplicate_face(f):
    f = np.asarray(f).reshape(-1, 3)
    sets = [tuple(sorted(t)) for t in f.tolist()]
    return all(len(set(t)) == 3 for t in sets) and len(set(sets)) == len(sets)


def point_triangle_distance(p, tri):
    """exact distances of the points p (n,3) to the triangles tri (m,3,3) -> (n,) the least over the triangles; float64
    numpy, the region walk of Ericson, Real-Time Collision Detection 5.1.5, vectorised over the triangles"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    out = np.empty(len(p))
    for i, x in enumerate(p):
        ap = x - a
        d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
        bp = x - b
        d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
        cp = x - c
        d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(all='ignore'):
            denom = 1.0 / (va + vb + vc)
            q = a + ab * (vb * denom)[:, None] + ac * (vc * denom)[:, None]                       # inside
            t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + (c - b) * t[:, None], q)
            t = d2 / (d2 - d6)
            q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + ac * t[:, None], q)
            t = d1 / (d1 - d3)
            q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + ab * t[:, None], q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, q)
        out[i] = np.sqrt(((x - q) ** 2).sum(1).min())
    return out


def two_sided_rms(v1, f1, s1, v2, f2, s2):
    """RMS of the exact distances of the samples s1 (on mesh 1) to mesh 2 and of s2 (on mesh 2) to mesh 1"""
    d12 = point_triangle_distance(s1, np.asarray(v2, np.float64)[np.asarray(f2)])
    d21 = point_triangle_distance(s2, np.asarray(v1, np.float64)[np.asarray(f1)])
    return float(np.sqrt((np.concatenate([d12, d21]) ** 2).mean()))


def surface_samples(v, f, n, seed):
    """n seeded area-weighted points on the mesh, float64"""
    v, f = np.asarray(v, np.float64), np.asarray(f)
    rng = np.random.default_rng(seed)
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = rng.choice(len(f), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], -1)
    return (tri[pick] * w[:, :, None]).sum(1)
