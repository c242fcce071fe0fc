"""Mesh simplification restated in IEEE doubles and integers (no test in here; tests/test_simplify_cpu.py and
tests/test_gpu_simplify.py import it).  It follows rules S0-S7 of include/rfd_simplify.h literally, one mesh, one edge,
one face at a time, and shares no code with the package.  The arithmetic is Python's own float: an IEEE double with one
rounding per written operation and a correctly rounded sqrt, every expression grouped as in the rules, so the device
(which evaluates them as written, no fused multiply-add) computes the same costs and positions bit for bit.

An edge's result (S2, S3) reads the faces of its two ends, their vertices' positions and the two quadrics only, so it is
kept from round to round until a collapse touches a vertex of one of those faces; the rules do not change by that, only
the time this file takes.  Two switches, flip_guard and link_condition, exist to show that the test cases bite."""
import math

import numpy as np

INF = float('inf')
INT32_MAX = 2 ** 31 - 1
MAX_ROUNDS = 1000


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _length(a):
    s = _dot(a, a)
    return math.sqrt(s) if s == s and s >= 0 else float('nan')      # sqrt(+inf) = +inf


def _usable(L):
    return L != 0 and math.isfinite(L)


def face_quadric(p0, p1, p2):
    """S1 for one face -> the ten numbers, or None"""
    n = _cross(_sub(p1, p0), _sub(p2, p0))
    L = _length(n)
    if not _usable(L):
        return None
    w = 0.5 * L
    m = (n[0] / L, n[1] / L, n[2] / L)
    d = -_dot(m, p0)
    gx, gy, gz, e = w * m[0], w * m[1], w * m[2], w * d
    return (gx * m[0], gx * m[1], gx * m[2], gy * m[1], gy * m[2], gz * m[2], e * m[0], e * m[1], e * m[2], e * d)


def quadric_cost(q, p):
    axx, axy, axz, ayy, ayz, azz, bx, by, bz, c = q
    hx = (axx * p[0] + axy * p[1]) + axz * p[2]
    hy = (axy * p[0] + ayy * p[1]) + ayz * p[2]
    hz = (axz * p[0] + ayz * p[1]) + azz * p[2]
    return (((p[0] * hx + p[1] * hy) + p[2] * hz) + 2.0 * ((bx * p[0] + by * p[1]) + bz * p[2])) + c


def placement(qa, qb, pa, pb):
    """S2 -> (cost, position), cost = +inf when no candidate costs less than that"""
    q = tuple(qa[t] + qb[t] for t in range(10))
    axx, axy, axz, ayy, ayz, azz, bx, by, bz, c = q
    mid = ((pa[0] + pb[0]) * 0.5, (pa[1] + pb[1]) * 0.5, (pa[2] + pb[2]) * 0.5)
    t = _sub(pb, pa)
    len2 = _dot(t, t)
    c00, c01, c02 = ayy * azz - ayz * ayz, axz * ayz - axy * azz, axy * ayz - axz * ayy
    c11, c12, c22 = axx * azz - axz * axz, axy * axz - axx * ayz, axx * ayy - axy * axy
    det = (axx * c00 + axy * c01) + axz * c02
    candidates = []
    if det != 0 and math.isfinite(det):
        rx, ry, rz = -bx, -by, -bz
        y = (((c00 * rx + c01 * ry) + c02 * rz) / det, ((c01 * rx + c11 * ry) + c12 * rz) / det,
             ((c02 * rx + c12 * ry) + c22 * rz) / det)
        if all(math.isfinite(a) for a in y):
            s = _sub(y, mid)
            if _dot(s, s) <= len2:
                candidates.append(y)
    candidates += [mid, tuple(pa), tuple(pb)]
    best, p = INF, (0.0, 0.0, 0.0)
    for cand in candidates:
        cc = quadric_cost(q, cand)
        if cc < best:
            best, p = cc, cand
    return best, p


class State(object):
    """the working state of one mesh: pos (list of 3-tuples), face (list of 3-lists, None = dead), Q"""

    def __init__(self, v, f):
        self.pos = [tuple(float(a) for a in row) for row in np.asarray(v, np.float64).reshape(-1, 3)]
        nv = len(self.pos)
        self.face = []
        for row in np.asarray(f).reshape(-1, 3).astype(np.int64).tolist():
            ok = all(0 <= i < nv for i in row) and len(set(row)) == 3
            self.face.append(list(row) if ok else None)
        self.nonfinite = [not all(math.isfinite(a) for a in p) for p in self.pos]
        self.rows()
        self.Q = []
        for vtx in range(nv):                                   # S1: the corners of vtx in ascending 3 face + c
            acc = [0.0] * 10
            for j in self.vfaces[vtx]:
                t = self.face[j]
                q = face_quadric(self.pos[t[0]], self.pos[t[1]], self.pos[t[2]])
                if q is not None:
                    acc = [acc[i] + q[i] for i in range(10)]
            self.Q.append(acc)

    def rows(self):
        self.vfaces = [[] for _ in self.pos]
        for j, t in enumerate(self.face):
            if t is not None:
                for i in t:
                    self.vfaces[i].append(j)                    # ascending face; a vertex is in a face once

    def alive(self):
        return sum(t is not None for t in self.face)

    def edges(self):
        """S0 -> {(a, b): [(face, runs a -> b), ...]} in ascending face order, and the frozen vertices"""
        table = {}
        for j, t in enumerate(self.face):
            if t is not None:
                for c in range(3):
                    u, w = t[c], t[(c + 1) % 3]
                    table.setdefault((min(u, w), max(u, w)), []).append((j, u < w))
        frozen_v = list(self.nonfinite)
        frozen_e = {}
        for (a, b), uses in table.items():
            fr = len(uses) != 2 or uses[0][1] == uses[1][1]
            frozen_e[(a, b)] = fr
            if fr:
                frozen_v[a] = frozen_v[b] = True
        return table, frozen_e, frozen_v

    def apex(self, j, a, b):
        return [i for i in self.face[j] if i != a and i != b][0]

    def link_ok(self, a, b, c0, c1):
        if c0 == c1:
            return False
        near_b = set(i for j in self.vfaces[b] for i in self.face[j])
        for j in self.vfaces[a]:
            t = self.face[j]
            if b in t:
                continue
            for w in t:
                if w != a and w != c0 and w != c1 and w in near_b:
                    return False

        def both(v, other):
            return any(other not in self.face[j] and c0 in self.face[j] and c1 in self.face[j] for j in self.vfaces[v])
        return not (both(a, b) and both(b, a))

    def flips(self, moved, other, p):
        o = self.pos[moved]
        for j in self.vfaces[moved]:
            t = self.face[j]
            if other in t:
                continue
            s = t.index(moved)
            q1, q2 = self.pos[t[(s + 1) % 3]], self.pos[t[(s + 2) % 3]]
            k = _cross(_sub(q1, o), _sub(q2, o))
            Lk = _length(k)
            d1, d2 = _sub(q1, p), _sub(q2, p)
            l1, l2 = _length(d1), _length(d2)
            if not _usable(l1) or not _usable(l2):
                return True
            u1 = (d1[0] / l1, d1[1] / l1, d1[2] / l1)
            u2 = (d2[0] / l2, d2[1] / l2, d2[2] / l2)
            if abs(_dot(u1, u2)) > 0.999:
                return True
            n = _cross(u1, u2)
            Ln = _length(n)
            if not _usable(Ln):
                return True
            if _usable(Lk) and _dot(n, k) < 0.2 * (Ln * Lk):
                return True
        return False

    def evaluate(self, a, b, c0, c1, flip_guard, link_condition):
        """S2, S3 -> (cost, position) of a legal edge, or None"""
        best, p = placement(self.Q[a], self.Q[b], self.pos[a], self.pos[b])
        if not best < INF:
            return None
        if link_condition and not self.link_ok(a, b, c0, c1):
            return None
        if flip_guard and (self.flips(a, b, p) or self.flips(b, a, p)):
            return None
        return best + 0.0, p


def simplify(v, f, n_faces, max_rounds=MAX_ROUNDS, flip_guard=True, link_condition=True, trace=None):
    """one mesh: v (V,3), f (F,3) with local indices, the target n_faces
    -> dict: 'v' (V2,3) f64, 'f' (F2,3) int64, 'reached' bool, 'rounds' int.  trace: a list that receives, per round, the
    kept collapses as (a, b, the set of alive faces that held a or b)."""
    v = np.asarray(v).astype(np.float64).reshape(-1, 3)         # f32 -> f64 is exact
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    n_faces = int(n_faces)
    if len(f) <= n_faces:                                       # S0: takes no part
        return {'v': v.copy(), 'f': f.copy(), 'reached': True, 'rounds': 0}
    st = State(v, f)
    cache = {}
    rounds = 0
    while rounds < max_rounds:
        need = (st.alive() - n_faces + 1) // 2
        if need <= 0:
            break
        rounds += 1
        table, frozen_e, frozen_v = st.edges()
        legal = []
        for (a, b) in sorted(table):
            if frozen_e[(a, b)] or frozen_v[a] or frozen_v[b]:
                continue
            if (a, b) not in cache:
                (j0, _), (j1, _) = table[(a, b)]
                cache[(a, b)] = st.evaluate(a, b, st.apex(j0, a, b), st.apex(j1, a, b), flip_guard, link_condition)
            if cache[(a, b)] is not None:
                legal.append((cache[(a, b)][0], a, b))
        legal.sort()                                            # S4: (cost, a, b); -0 == 0 for Python as for the device
        rank = {(a, b): r for r, (_, a, b) in enumerate(legal)}
        m1 = [INT32_MAX] * len(st.pos)
        for (a, b), r in rank.items():
            m1[a], m1[b] = min(m1[a], r), min(m1[b], r)
        m2 = list(m1)
        for (a, b) in table:
            m2[a], m2[b] = min(m2[a], m1[b]), min(m2[b], m1[a])
        kept = [(a, b) for (_, a, b) in legal if rank[(a, b)] == m2[a] == m2[b]][:need]
        if not kept:
            break
        if trace is not None:
            trace.append([(a, b, set(st.vfaces[a]) | set(st.vfaces[b])) for a, b in kept])
        dirty = set()
        for a, b in kept:                                       # S5
            for j in st.vfaces[a] + st.vfaces[b]:
                dirty.update(st.face[j])
        for a, b in kept:
            p = cache[(a, b)][1]
            (j0, _), (j1, _) = table[(a, b)]
            st.pos[a] = p
            st.Q[a] = [st.Q[a][t] + st.Q[b][t] for t in range(10)]
            for j in st.vfaces[b]:
                st.face[j] = [a if i == b else i for i in st.face[j]]
            st.face[j0] = st.face[j1] = None
        st.rows()
        cache = {e: r for e, r in cache.items() if e[0] not in dirty and e[1] not in dirty}
    # S7
    faces = [t for t in st.face if t is not None]
    named = sorted(set(i for t in faces for i in t))
    renumber = {i: at for at, i in enumerate(named)}
    return {'v': np.array([st.pos[i] for i in named], np.float64).reshape(-1, 3),
            'f': np.array([[renumber[i] for i in t] for t in faces], np.int64).reshape(-1, 3),
            'reached': st.alive() <= n_faces, 'rounds': rounds}
