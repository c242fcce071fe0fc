"""Rules D1 - D8 of include/rfd_mesh_dist.h restated in numpy float64 (no test in here): the valid faces, the frame, the
cell lists, the closest point of a triangle, the brute force over all valid faces, the shell walk with its pruning, the
ragged surface samples and the fixed-shape sums.  Every operation is written in the header's order, one rounding each;
numpy's element-wise loops fuse nothing.  Nothing here imports the package."""
import numpy as np

MAX_RES = 64
INF = np.inf


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(t):
    """the cross product of rules S1 / S4 of rfd_sample.h for triangles (m,3,3) -> (m,3)"""
    a, b = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def face_normals(t):
    """rule S4: (m,3), the zero vector for a face of area 0"""
    c = cross(t)
    length = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    with np.errstate(all='ignore'):
        return np.where((length == 0)[:, None], 0., c / length[:, None])


def triangles(v, f, vend, tend):
    """rule D1 -> tri (F,3,3) (zeros for a corner whose index is out of range), valid (F) bool, fobj (F) int"""
    v, f = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    F = len(f)
    fobj = np.searchsorted(np.asarray(tend, np.int64), np.arange(F), side='right') - 1
    v0 = np.asarray(vend, np.int64)[fobj]
    nv = np.asarray(vend, np.int64)[fobj + 1] - v0
    inside = (f >= 0) & (f < nv[:, None])
    tri = np.zeros((F, 3, 3))
    tri[inside] = v[(f + v0[:, None])[inside]]
    valid = inside.all(1) & np.isfinite(tri).all((1, 2))
    with np.errstate(all='ignore'):
        c = cross(tri)
        area = 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    valid &= np.isfinite(area) & (area != 0)
    return tri, valid, fobj


def default_cells(n_valid):
    return int(min(max(np.ceil(np.cbrt(n_valid / 8.)), 1), MAX_RES))


class Frame(object):
    """rule D2 for one object: lo, hi, R, inv_h, h, slack"""

    def __init__(self, tri, valid, cells=None):
        corners = tri[valid].reshape(-1, 3)
        self.lo = corners.min(0) if len(corners) else np.zeros(3)
        self.hi = corners.max(0) if len(corners) else np.zeros(3)
        self.R = R = default_cells(int(valid.sum())) if cells is None else int(cells)
        assert 1 <= R <= MAX_RES
        ext = self.hi - self.lo
        with np.errstate(all='ignore'):
            self.inv_h = np.where(ext > 0, R / ext, 0.)
            self.h = np.where(ext > 0, ext / R, 0.)
        self.slack = 2. ** -30 * max(ext.max(), np.abs(self.lo).max(), np.abs(self.hi).max())
        self.Ra = np.where(self.inv_h == 0, 1, R)

    def cell(self, x):
        """x (...,3) -> (...,3) int"""
        with np.errstate(all='ignore'):
            t = (x - self.lo) * self.inv_h
        out = np.zeros(t.shape, np.int64)
        ok = t >= 0
        out[ok] = np.minimum(np.floor(t[ok]), self.R - 1).astype(np.int64)
        return out


def cell_lists(tri, valid, frame):
    """rule D3 for one object -> {(ix, iy, iz): [face rows]} (rows local to `tri`)"""
    lists = {}
    for row in np.nonzero(valid)[0]:
        c = frame.cell(tri[row])
        c0, c1 = c.min(0), c.max(0)
        for x in range(c0[0], c1[0] + 1):
            for y in range(c0[1], c1[1] + 1):
                for z in range(c0[2], c1[2] + 1):
                    lists.setdefault((x, y, z), []).append(row)
    return lists


def closest_points(p, tri):
    """rule D4: one point p (3) against triangles (m,3,3) -> q (m,3), d2 (m)"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot3(ab, ap), dot3(ac, ap), dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all='ignore'):
        e = 1. / ((va + vb) + vc)
        q = (a + ab * (vb * e)[:, None]) + ac * (vc * e)[:, None]
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + (c - b) * t[:, None], q)
        t = d2 / (d2 - d6)
        q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + ac * t[:, None], q)
        t = d1 / (d1 - d3)
        q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + ab * t[:, None], q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, q)
        r = p - q
        return q, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]


NONE = (INF, -1, np.full(3, np.nan))


def best_of(p, tri, rows, best=NONE):
    """rule D5: the least key (d2, row) of best and the triangles tri[rows]; rows ascending or not"""
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return best
    q, d2 = closest_points(p, tri[rows])
    d2 = np.where(np.isfinite(d2), d2, INF)
    m = d2.min()
    if not m < INF:
        return best
    at = np.nonzero(d2 == m)[0]
    i = at[np.argmin(rows[at])]
    if m < best[0] or (m == best[0] and rows[i] < best[1]):
        return (m, int(rows[i]), q[i])
    return best


def brute_force(p, tri, valid):
    """rules D4 and D5 over all valid faces of one object -> (d2, row, q)"""
    if not np.isfinite(p).all():
        return (np.nan, -1, np.full(3, np.nan))
    return best_of(p, tri, np.nonzero(valid)[0])


def walk(p, tri, frame, lists):
    """rule D6 -> (d2, row, q), and the number of shells visited"""
    if not np.isfinite(p).all():
        return (np.nan, -1, np.full(3, np.nan)), 0
    pp = np.minimum(np.maximum(p, frame.lo), frame.hi)
    c = np.minimum(frame.cell(pp), frame.Ra - 1)
    o = np.maximum(np.abs(p - pp) - frame.slack, 0.)
    out2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    best, shells = NONE, 0
    for r in range(frame.R):
        shells += 1
        rows = []
        lo_c, hi_c = np.maximum(c - r, 0), np.minimum(c + r, frame.Ra - 1)
        for x in range(lo_c[0], hi_c[0] + 1):
            for y in range(lo_c[1], hi_c[1] + 1):
                if abs(x - c[0]) == r or abs(y - c[1]) == r:
                    zs = range(lo_c[2], hi_c[2] + 1)
                else:
                    zs = [z for z in sorted(set((c[2] - r, c[2] + r))) if 0 <= z <= frame.Ra[2] - 1]
                for z in zs:
                    rows += lists.get((x, y, z), [])
        best = best_of(p, tri, sorted(set(rows)), best)
        g = INF
        for a in range(3):
            if c[a] - r - 1 >= 0:
                g = min(g, pp[a] - (frame.lo[a] + float(c[a] - r) * frame.h[a]))
            if c[a] + r + 1 <= frame.Ra[a] - 1:
                g = min(g, (frame.lo[a] + float(c[a] + r + 1) * frame.h[a]) - pp[a])
        if g == INF:
            break
        g = max(g - frame.slack, 0.)
        if best[0] < (out2 + g * g) * (1. - 2. ** -40):
            break
    return best, shells


class Batch(object):
    """the ragged batch of the restatement: per-object frames and lists, rows of the flat face array throughout"""

    def __init__(self, v, f, vend, tend, cells=None):
        self.tri, self.valid, self.fobj = triangles(v, f, vend, tend)
        self.tend = np.asarray(tend, np.int64)
        self.K = len(self.tend) - 1
        self.frames, self.lists = [], []
        for k in range(self.K):
            rows = slice(self.tend[k], self.tend[k + 1])
            fr = Frame(self.tri[rows], self.valid[rows], cells)
            self.frames.append(fr)
            self.lists.append(cell_lists(self.tri[rows], self.valid[rows], fr))

    def query(self, points, obj, brute=False):
        """-> d2 (n), face (n) flat rows, closest (n,3)"""
        points = np.asarray(points, np.float64).reshape(-1, 3)
        n = len(points)
        d2, face, q = np.empty(n), np.empty(n, np.int64), np.empty((n, 3))
        for i in range(n):
            k = int(obj[i])
            rows = slice(self.tend[k], self.tend[k + 1])
            if brute:
                b = brute_force(points[i], self.tri[rows], self.valid[rows])
            else:
                b, _ = walk(points[i], self.tri[rows], self.frames[k], self.lists[k])
            d2[i], face[i], q[i] = b[0], (b[1] + self.tend[k] if b[1] >= 0 else -1), b[2]
        return d2, face, q


def face_areas(tri, valid):
    """rule S1, 0 for a face that is not valid (rule D7)"""
    with np.errstate(all='ignore'):
        c = cross(tri)
        return np.where(valid, 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]), 0.)


def area_prefix(tri, valid, tend):
    """every object's own inclusive prefix of the face areas (numpy's cumsum: rule D7 leaves the order open)"""
    cum = np.zeros(len(tri))
    for k in range(len(tend) - 1):
        rows = slice(int(tend[k]), int(tend[k + 1]))
        cum[rows] = np.cumsum(face_areas(tri[rows], valid[rows]))
    return cum


def sample(tri, tend, cum, u):
    """rule D7: u (K,count,3), cum (F) -> points (K,count,3), face (K,count) flat rows, normals (K,count,3)"""
    K, count = u.shape[:2]
    points, face, normals = np.full((K, count, 3), np.nan), np.full((K, count), -1, np.int64), np.zeros((K, count, 3))
    for k in range(K):
        f0, Fk = int(tend[k]), int(tend[k + 1] - tend[k])
        if Fk < 1:
            continue
        cm = cum[f0:f0 + Fk]
        nrm = face_normals(tri[f0:f0 + Fk])
        for i in range(count):
            target = u[k, i, 0] * cm[Fk - 1]
            lo, hi = 0, Fk - 1
            while lo < hi:
                mid = lo + (hi - lo) // 2
                if cm[mid] >= target:
                    hi = mid
                else:
                    lo = mid + 1
            t = tri[f0 + lo]
            a, b = u[k, i, 1], u[k, i, 2]
            if a + b > 1.:
                a, b = abs(a - 1.), abs(b - 1.)
            points[k, i] = t[0] + ((t[1] - t[0]) * a + (t[2] - t[0]) * b)
            face[k, i] = f0 + lo
            normals[k, i] = nrm[lo]
    return points, face, normals


def tree_sum(x, keep):
    """rule D8's fixed shape over the entries x (m) of which `keep` take part"""
    part = np.zeros(64)
    for j in range(64):
        s = 0.
        for e in range(j, len(x), 64):
            if keep[e]:
                s = s + x[e]
        part[j] = s
    w = 32
    while w >= 1:
        part[:w] = part[:w] + part[w:2 * w]
        w //= 2
    return part[0]


def sums(seg, d2, face, normals, tri, tau):
    """rule D8 -> sums (S,3), counts (S, 1 + T)"""
    S, T = len(seg) - 1, len(tau)
    out, counts = np.zeros((S, 3)), np.zeros((S, 1 + T), np.int64)
    with np.errstate(all='ignore'):
        d = np.sqrt(d2)
    keep = np.isfinite(d) & (face >= 0) & (face < len(tri))
    ndot = np.zeros(len(d2))
    if normals is not None and keep.any():
        ndot[keep] = np.abs(dot3(normals[keep], face_normals(tri[face[keep]])))
    for s in range(S):
        e = slice(int(seg[s]), int(seg[s + 1]))
        out[s] = [tree_sum(d[e], keep[e]), tree_sum(d2[e], keep[e]), tree_sum(ndot[e], keep[e])]
        counts[s, 0] = (~keep[e]).sum()
        for t in range(T):
            counts[s, 1 + t] = (keep[e] & (d[e] <= tau[t])).sum()
    return out, counts


def two_sided_rms(d2_ab, d2_ba):
    """the metric `rms` of mesh_metrics from the two directions' squared distances (tree sums, then f64 arithmetic)"""
    sa = tree_sum(d2_ab, np.isfinite(d2_ab))
    sb = tree_sum(d2_ba, np.isfinite(d2_ba))
    return float(np.sqrt((sa + sb) / (np.isfinite(d2_ab).sum() + np.isfinite(d2_ba).sum())))
