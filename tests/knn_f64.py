"""Rules N1 - N7 of include/rfd_knn.h restated in numpy float64 (no test in here): the valid points, the frame, the cell
of every point, the brute force as a stable sort by (d2, row), the shell walk with its pruning, and the fixed-shape sums.
Every operation is written in the header's order, one rounding each; numpy's element-wise loops fuse nothing.  The frame
(rule N2 is rule D2) and the tree of the sums (rule N7 has rule D8's shape) are those of tests/mesh_dist_f64.py.  Nothing
here imports the package."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_dist_f64 as D  # noqa: E402

INF = np.inf
MAX_K = 32


def valid_points(pts):
    """rule N1"""
    return np.isfinite(pts).all(1)


def frame_of(pts, cells=None):
    """rule N2 for one set: rule D2's frame over the valid points (a point is a triangle of one corner here)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    return D.Frame(pts[:, None, :], valid_points(pts), cells)


def dist2(q, pts):
    """rule N4: queries (n,3) against points (m,3) -> (n,m)"""
    with np.errstate(all='ignore'):
        r = q[:, None, :] - pts[None, :, :]
        return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def candidates(pts, mask):
    """the rows that may answer at all: valid and not masked (rule N5)"""
    keep = valid_points(pts)
    if mask is not None:
        keep &= np.asarray(mask).reshape(-1) == 0
    return keep


def k_least(d2, rows, k):
    """d2 (m) of the candidate rows (m), ascending -> the k least keys (d2, row): a stable sort, padded with (inf, -1)"""
    order = np.argsort(d2, kind='stable')[:k]
    out_d, out_i = np.full(k, INF), np.full(k, -1, np.int64)
    out_d[:len(order)], out_i[:len(order)] = d2[order], rows[order]
    return out_d, out_i


def brute_force(q, pts, k, limit2=INF, mask=None, chunk=256):
    """rules N4, N5 over one whole set -> d2 (n,k), idx (n,k); (NaN, -1) for a query that is not finite.  The stable sort
    of every row runs over the entries up to its k-th least value only (np.partition finds that value exactly)."""
    q, pts = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(q)
    out_d, out_i = np.full((n, k), INF), np.full((n, k), -1, np.int64)
    rows = np.nonzero(candidates(pts, mask))[0]
    finite = np.isfinite(q).all(1)
    out_d[~finite] = np.nan
    if len(rows):
        for a in range(0, n, chunk):
            d2 = dist2(q[a:a + chunk], pts[rows])
            d2 = np.where(d2 < limit2, d2, INF)                  # strict; +inf itself is never a candidate
            kk = min(k, len(rows))
            kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
            for i in range(len(d2)):
                if not finite[a + i]:
                    continue
                take = np.nonzero((d2[i] <= kth[i]) & (d2[i] < INF))[0]
                out_d[a + i], out_i[a + i] = k_least(d2[i][take], rows[take], k)
    return out_d, out_i


def walk(p, pts, frame, cell, k, limit2=INF, mask=None):
    """rule N6 for one query -> (d2 (k), idx (k)), and the number of shells visited.  cell (m,3): the cell of every row,
    -1 for a row that is not valid; a shell's rows are the valid rows whose cell is at Chebyshev distance r."""
    if not np.isfinite(p).all():
        return (np.full(k, np.nan), np.full(k, -1, np.int64)), 0
    keep = candidates(pts, mask)
    pp = np.minimum(np.maximum(p, frame.lo), frame.hi)
    c = np.minimum(frame.cell(pp), frame.Ra - 1)
    o = np.maximum(np.abs(p - pp) - frame.slack, 0.)
    with np.errstate(over='ignore'):                           # a query at 1e300: the bound is +inf, as on the device
        out2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    cheb = np.abs(cell - c).max(1) if len(cell) else np.zeros(0, np.int64)
    best_d, best_i = np.full(k, INF), np.full(k, -1, np.int64)
    shells = 0
    for r in range(frame.R):
        shells += 1
        rows = np.nonzero(keep & (cell[:, 0] >= 0) & (cheb == r))[0] if len(cell) else np.zeros(0, np.int64)
        if len(rows):
            d2 = dist2(p[None], pts[rows])[0]
            ok = d2 < limit2
            # what entered so far and the shell's candidates, merged: the k least keys of all of them
            d_all, i_all = np.concatenate([best_d[best_i >= 0], d2[ok]]), np.concatenate([best_i[best_i >= 0], rows[ok]])
            order = np.lexsort((i_all, d_all))
            best_d, best_i = k_least(d_all[order], i_all[order], k)
        g = INF
        for a in range(3):
            if c[a] - r - 1 >= 0:
                g = min(g, pp[a] - (frame.lo[a] + float(c[a] - r) * frame.h[a]))
            if c[a] + r + 1 <= frame.Ra[a] - 1:
                g = min(g, (frame.lo[a] + float(c[a] + r + 1) * frame.h[a]) - pp[a])
        if g == INF:
            break
        g = max(g - frame.slack, 0.)
        if min(best_d[k - 1], limit2) < (out2 + g * g) * (1. - 2. ** -40):
            break
    return (best_d, best_i), shells


class Batch(object):
    """the ragged batch of the restatement: per-set frames and cells; rows LOCAL to their set throughout"""

    def __init__(self, pts, pend=None, cells=None):
        self.pts = np.asarray(pts, np.float64).reshape(-1, 3)
        self.pend = np.asarray([0, len(self.pts)] if pend is None else pend, np.int64)
        self.K = len(self.pend) - 1
        self.frames, self.cell = [], []
        for k in range(self.K):
            mine = self.pts[self.pend[k]:self.pend[k + 1]]
            fr = frame_of(mine, cells)
            cell = np.full((len(mine), 3), -1, np.int64)
            ok = valid_points(mine)
            cell[ok] = fr.cell(mine[ok])
            self.frames.append(fr)
            self.cell.append(cell)

    def query(self, points, obj=None, k=1, limit2=INF, mask=None, brute=True):
        """-> d2 (n,k), idx (n,k); mask (N) over the batch's GLOBAL rows"""
        points = np.asarray(points, np.float64).reshape(-1, 3)
        n = len(points)
        obj = np.zeros(n, np.int64) if obj is None else np.asarray(obj, np.int64)
        d2, idx = np.full((n, k), np.nan), np.full((n, k), -1, np.int64)
        for s in range(self.K):
            mine = np.nonzero(obj == s)[0]
            if not len(mine):
                continue
            rows = slice(self.pend[s], self.pend[s + 1])
            m = None if mask is None else np.asarray(mask).reshape(-1)[rows]
            if brute:
                d2[mine], idx[mine] = brute_force(points[mine], self.pts[rows], k, limit2, m)
            else:
                for i in mine:
                    (d2[i], idx[i]), _ = walk(points[i], self.pts[rows], self.frames[s], self.cell[s], k, limit2, m)
        return d2, idx


def sums(seg, d2, row, qobj, pend, n_s, n_t, tau):
    """rule N7 over the slot-0 results d2 (n), row (n) of queries of the objects qobj (n) -> sums (S,3), counts (S, 1 + T)"""
    S, T = len(seg) - 1, len(tau)
    pend = np.asarray(pend, np.int64)
    K = len(pend) - 1
    out, counts = np.zeros((S, 3)), np.zeros((S, 1 + T), np.int64)
    with np.errstate(all='ignore'):
        d = np.sqrt(d2)
    row, qobj = np.asarray(row, np.int64), np.asarray(qobj, np.int64)
    ko = np.clip(qobj, 0, max(K - 1, 0))
    inside = (qobj >= 0) & (qobj < K) & (row >= 0)
    if K > 0:
        inside &= row < (pend[ko + 1] - pend[ko])
    else:
        inside &= False
    keep = np.isfinite(d) & inside
    ndot = np.zeros(len(d2))
    if n_s is not None and n_t is not None and keep.any():
        ndot[keep] = np.abs(D.dot3(n_s[keep], n_t[(pend[ko] + row)[keep]]))
    for s in range(S):
        e = slice(int(seg[s]), int(seg[s + 1]))
        out[s] = [D.tree_sum(d[e], keep[e]), D.tree_sum(d2[e], keep[e]), D.tree_sum(ndot[e], keep[e])]
        counts[s, 0] = (~keep[e]).sum()
        for t in range(T):
            counts[s, 1 + t] = (keep[e] & (d[e] <= tau[t])).sum()
    return out, counts
