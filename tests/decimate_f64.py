"""Mesh decimation restated in numpy float64 / int64 (no test in here; tests/test_decimate_cpu.py and
tests/test_gpu_decimate.py import it).  It follows the five rules of include/rfd_decimate.h literally, one mesh, one
cell, one face at a time, and shares no code with the package.  Every floating-point expression is written with the
grouping of the rules, so an IEEE machine that evaluates them as written (no fused multiply-add) computes the same
cells bit for bit and the same positions up to the last place of a quotient or a square root."""
import numpy as np

PADDING = 0.1
LANES = 16


def default_cube(K, cells, padding=PADDING):
    box = 1.0 + padding
    return np.full((K, 3), -box / 2), np.full(K, box / cells)


def vertex_cells(x, lo, h, cells):
    """rule 1 for the vertices x (n,3) f64 of one mesh -> (ix, iy, iz) (n,3) int64, has_cell (n) bool"""
    inv_h = 1.0 / h
    finite = np.isfinite(x).all(1)
    with np.errstate(all='ignore'):
        t = np.floor((np.where(finite[:, None], x, 0.0) - lo) * inv_h)
    return np.clip(t, 0, cells - 1).astype(np.int64), finite


def corner_terms(p0, p1, p2, pc, g):
    """rule 3 for one corner (all (3,) f64) -> the 13 terms, or None for a skipped corner"""
    u, v = p1 - p0, p2 - p0
    with np.errstate(all='ignore'):
        n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        L = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if L == 0 or not np.isfinite(L):
            return None
        w = 0.5 * L
        m = n / L
        q = p0 - g
        d = -((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2])
        wm, wd, r = w * m, -(w * d), pc - g
        return np.array([wm[0] * m[0], wm[0] * m[1], wm[0] * m[2], wm[1] * m[1], wm[1] * m[2], wm[2] * m[2],
                         wd * m[0], wd * m[1], wd * m[2], w, w * r[0], w * r[1], w * r[2]])


def tree_sum(terms):
    """the fixed summation shape: 16 partial sums (partial j: terms j, j + 16, ... in order, from 0), then 8, 4, 2, 1"""
    part = np.zeros((LANES, 13))
    with np.errstate(all='ignore'):
        for i, t in enumerate(terms):
            part[i % LANES] = part[i % LANES] + t
        step = LANES // 2
        while step >= 1:
            part[:step] = part[:step] + part[step:2 * step]
            step //= 2
    return part[0]


def solve(sums, h, regularise):
    """rule 3's solve -> y (3,) f64, clamped into the cell"""
    axx, axy, axz, ayy, ayz, azz, bx, by, bz, W, sx, sy, sz = np.asarray(sums, np.float64)      # numpy scalars: x / 0 = inf
    y = np.zeros(3)
    with np.errstate(all='ignore'):
        if W != 0:
            l = np.float64(regularise) * W
            axx, ayy, azz = axx + l, ayy + l, azz + l
            bx, by, bz = bx + l * (sx / W), by + l * (sy / W), bz + l * (sz / W)
            c00, c01, c02 = ayy * azz - ayz * ayz, axz * ayz - axy * azz, axy * ayz - axz * ayy
            c11, c12, c22 = axx * azz - axz * axz, axy * axz - axx * ayz, axx * ayy - axy * axy
            det = (axx * c00 + axy * c01) + axz * c02
            y = np.array([((c00 * bx + c01 * by) + c02 * bz) / det, ((c01 * bx + c11 * by) + c12 * bz) / det,
                          ((c02 * bx + c12 * by) + c22 * bz) / det])
        y = np.where(np.isfinite(y), y, 0.0)
        half = 0.5 * np.float64(h)
        return np.minimum(np.maximum(y, -half), half)


def decimate(v, f, vend, tend, cells, lo=None, h=None, regularise=1e-3):
    """-> dict: 'v' (V2,3) f32, 'f' (F2,3) int64 (local indices), 'vend', 'tend' (lists), and for the tests 'key' (V2)
    int64 (the cell key of every output vertex), 'corners' (V2) int64 (how many corners its cell visited, skipped ones
    included), 'W' (V2) f64, 'h' (V2) f64 (its mesh's cell size), 'centre' (V2,3) f64"""
    vend, tend = [int(a) for a in vend], [int(a) for a in tend]
    K, cells = len(vend) - 1, int(cells)
    if cells < 1:
        raise ValueError("cells < 1")
    if K * cells ** 3 >= 2 ** 31:
        raise ValueError("K cells^3 >= 2^31")
    if lo is None or h is None:
        dlo, dh = default_cube(K, cells)
        lo, h = dlo if lo is None else lo, dh if h is None else h
    lo = np.broadcast_to(np.asarray(lo, np.float64), (K, 3))
    h = np.broadcast_to(np.asarray(h, np.float64), (K,))
    x = np.asarray(v).astype(np.float64).reshape(-1, 3)                  # f32 -> f64 is exact
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    out = {name: [] for name in ('v', 'f', 'key', 'corners', 'W', 'h', 'centre')}
    vend2, tend2 = [0], [0]
    for k in range(K):
        xk, fk = x[vend[k]:vend[k + 1]], f[tend[k]:tend[k + 1]]
        nv = xk.shape[0]
        ijk, has_cell = vertex_cells(xk, lo[k], h[k], cells)
        cell = np.where(has_cell, (ijk[:, 2] * cells + ijk[:, 1]) * cells + ijk[:, 0], -1)      # rule 1, without k cells^3
        cand = np.unique(cell[cell >= 0])                                                        # rule 2
        in_range = ((fk >= 0) & (fk < nv)).all(1) if len(fk) else np.zeros(0, bool)
        # rule 4: remap, drop, mod 2
        groups, mapped = {}, {}
        for j in range(len(fk)):
            if not in_range[j]:
                continue
            cs = cell[fk[j]]
            if (cs < 0).any() or len(set(cs.tolist())) < 3:
                continue
            mapped[j] = np.searchsorted(cand, cs)
            groups.setdefault(tuple(sorted(cs.tolist())), []).append(j)
        kept = sorted(js[0] for js in groups.values() if len(js) % 2 == 1)
        # rule 5
        named = np.zeros(len(cand), bool)
        for j in kept:
            named[mapped[j]] = True
        renumber = np.cumsum(named) - 1
        out['f'].append(np.array([renumber[mapped[j]] for j in kept], np.int64).reshape(-1, 3))
        # rule 3 for the cells that stay
        corners_of = {}
        for j in range(len(fk)):
            if in_range[j]:
                for c in range(3):
                    corners_of.setdefault(int(cell[fk[j, c]]), []).append((j, c))                # ascending 3 j + c
        for ci in np.nonzero(named)[0]:
            r = int(cand[ci])
            idx = np.array([r % cells, (r // cells) % cells, r // (cells * cells)], np.float64)
            g = lo[k] + (idx + 0.5) * h[k]
            terms = []
            for j, c in corners_of.get(r, []):
                t = corner_terms(xk[fk[j, 0]], xk[fk[j, 1]], xk[fk[j, 2]], xk[fk[j, c]], g)
                if t is not None:
                    terms.append(t)
            sums = tree_sum(terms)
            y = solve(sums, h[k], regularise)
            out['v'].append((g + y).astype(np.float32))
            out['key'].append(k * cells ** 3 + r)
            out['corners'].append(len(corners_of.get(r, [])))
            out['W'].append(sums[9])
            out['h'].append(h[k])
            out['centre'].append(g)
        vend2.append(vend2[-1] + int(named.sum()))
        tend2.append(tend2[-1] + len(kept))
    res = {'v': np.array(out['v'], np.float32).reshape(-1, 3),
           'f': np.concatenate(out['f']).reshape(-1, 3) if out['f'] else np.zeros((0, 3), np.int64),
           'vend': vend2, 'tend': tend2, 'key': np.array(out['key'], np.int64),
           'corners': np.array(out['corners'], np.int64), 'W': np.array(out['W'], np.float64),
           'h': np.array(out['h'], np.float64), 'centre': np.array(out['centre'], np.float64).reshape(-1, 3)}
    return res


def edge_counts(f):
    """faces (n,3) of ONE mesh -> {undirected edge: how many faces use it}"""
    counts = {}
    for a, b, c in np.asarray(f).reshape(-1, 3).tolist():
        for e in ((a, b), (b, c), (c, a)):
            e = (min(e), max(e))
            counts[e] = counts.get(e, 0) + 1
    return counts


def all_edges_even(f):
    return all(n % 2 == 0 for n in edge_counts(f).values())
