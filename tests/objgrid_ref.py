"""Numpy restatement of the ragged batch of include/rfd_mesh_eval.h, rules B1 - B7 (no test in here;
tests/test_objgrid_cpu.py and tests/test_gpu_objgrid.py import it).  Unlike tests/mesh_iou_f64.voxelize -- the oracle,
which asks tests/mesh_sample_ref.contains about every lattice point against every triangle -- this walks the lattice as
the kernels do: per-axis candidates, the 32 x 32 bins of rule B6, per column the parity words P0 / P1 over z.  That it
gives the oracle's words proves the filter and the parities before any GPU run.  numpy evaluates every operation on its
own, in float64, left to right as the rules write them."""
import numpy as np

import mesh_iou_f64 as M
import mesh_sample_ref as R

RES, SHIFT = 512, 4
BINS = RES >> SHIFT


class Restated(object):
    """one object: D (0: no grid), lo, cell, the packed words S, P0, P1, I, U (uint64), cnt = (|U|, |S|), margin"""

    def __init__(self, D=0, lo=None, cell=None, S=None, P0=None, P1=None, margin=np.inf, pairs=0):
        self.D, self.lo, self.cell, self.S, self.P0, self.P1, self.margin, self.pairs = D, lo, cell, S, P0, P1, margin, pairs
        if D:
            self.I = P0 & P1
            self.U = S | self.I
            self.cnt = (popcount(self.U), popcount(S))
        else:
            self.I = self.U = np.zeros(0, np.uint64)
            self.cnt = (0, 0)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def constants(tri):
    """B3: tri (F,3,3) in the unit cube -> (scale, translate), or None where I = 0; ValueError as rescale_constants"""
    flat = tri.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    if not (hi - lo > 0).all():
        return None
    scale = (RES - 1) / (hi - lo)
    translate = 0.5 - scale * lo
    if not (np.isfinite(scale).all() and np.isfinite(translate).all()):
        raise ValueError("mesh: the triangles' bounding box is too thin to rescale (%s .. %s)" % (lo, hi))
    return scale, translate


def cell_of(x):
    """(int)x clamped to [0, RES - 1]"""
    return np.clip(np.trunc(x).astype(np.int64), 0, RES - 1)


def bin_lists(T):
    """B6: rescaled triangles (F,3,3) -> {(bx, by): [triangle, ...]}, the number of (bin, triangle) pairs"""
    x0, x1 = cell_of(T[:, :, 0].min(1)) >> SHIFT, cell_of(T[:, :, 0].max(1)) >> SHIFT
    y0, y1 = cell_of(T[:, :, 1].min(1)) >> SHIFT, cell_of(T[:, :, 1].max(1)) >> SHIFT
    lists, pairs = {}, 0
    for f in range(T.shape[0]):
        for bx in range(x0[f], x1[f] + 1):
            for by in range(y0[f], y1[f] + 1):
                lists.setdefault((bx, by), []).append(f)
                pairs += 1
    return lists, pairs


def parities(unit, faces, D):
    """B3 - B6 -> n0, n1 (D,D,D) i32: how often every lattice point was toggled in P0 / P1; the margin; the pairs"""
    n0, n1 = np.zeros((D, D, D), np.int32), np.zeros((D, D, D), np.int32)
    tri = np.asarray(unit, np.float64)[faces]
    st = constants(tri)
    if st is None:
        return n0, n1, np.inf, 0
    scale, translate = st
    T = scale * tri + translate                                                         # C2
    c = (np.arange(D) + 0.5) / D - 0.5                                                  # B4
    p = scale * c[:, None] + translate                                                  # (D,3): px', py', pz' by index
    margin = float(np.minimum(np.abs(p), np.abs(RES - p)).min() / RES)
    cand_x, cand_y = (0 <= p[:, 0]) & (p[:, 0] < RES), (0 <= p[:, 1]) & (p[:, 1] < RES)
    cand_z = (0 <= p[:, 2]) & (p[:, 2] <= RES)
    bin_x, bin_y = cell_of(p[:, 0]) >> SHIFT, cell_of(p[:, 1]) >> SHIFT
    lists, pairs = bin_lists(T)
    for (bx, by), members in sorted(lists.items()):
        I, J = np.nonzero(cand_x & (bin_x == bx))[0], np.nonzero(cand_y & (bin_y == by))[0]
        if len(I) == 0 or len(J) == 0:
            continue
        ii, jj = (a.reshape(-1) for a in np.meshgrid(I, J, indexing='ij'))
        px, py = p[ii, 0][:, None], p[jj, 1][:, None]
        t = T[np.array(members)]
        t1, t2, t3 = t[None, :, 0], t[None, :, 1], t[None, :, 2]
        A00, A10, A01, A11 = t1[..., 0] - t3[..., 0], t1[..., 1] - t3[..., 1], t2[..., 0] - t3[..., 0], t2[..., 1] - t3[..., 1]
        det = A00 * A11 - A01 * A10                                                    # C4
        s, ad = np.sign(det), np.abs(det)
        y0, y1 = px - t3[..., 0], py - t3[..., 1]
        u = (A11 * y0 - A01 * y1) * s
        v = (-A10 * y0 + A00 * y1) * s
        w = u + v
        live = np.broadcast_to(det != 0, u.shape)
        if live.any():
            with np.errstate(divide='ignore', invalid='ignore'):
                m = np.minimum.reduce([np.abs(u), np.abs(ad - u), np.abs(v), np.abs(ad - v), np.abs(w), np.abs(ad - w)]) / ad
            margin = min(margin, float(m[live].min()))
        hit = live & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < w) & (w < ad)
        v1, v2 = t3 - t1, t2 - t1                                                      # C5
        nn0 = v1[..., 1] * v2[..., 2] - v1[..., 2] * v2[..., 1]
        nn1 = v1[..., 2] * v2[..., 0] - v1[..., 0] * v2[..., 2]
        nn2 = v1[..., 0] * v2[..., 1] - v1[..., 1] * v2[..., 0]
        an, sn = np.abs(nn2), np.sign(nn2)
        hit &= nn2 != 0
        cols, tris = np.nonzero(hit)
        if len(cols) == 0:
            continue
        alpha = nn0 * (t1[..., 0] - px) + nn1 * (t1[..., 1] - py)
        depth = (t1[..., 2] * an + alpha * sn)[cols, tris]
        rhs = p[None, :, 2] * an[0, tris][:, None]                                     # B5: (hits, D)
        ge = (depth[:, None] >= rhs) & cand_z
        lt = (depth[:, None] < rhs) & cand_z
        np.add.at(n0, (ii[cols], jj[cols]), ge.astype(np.int32))
        np.add.at(n1, (ii[cols], jj[cols]), lt.astype(np.int32))
        with np.errstate(divide='ignore', invalid='ignore'):
            md = np.abs(depth[:, None] - rhs) / np.maximum(np.abs(depth[:, None]), np.abs(rhs))
        md = md[np.broadcast_to(cand_z, md.shape)]
        if md.size:
            margin = min(margin, float(np.nan_to_num(md, nan=0.0).min()))
    return n0, n1, margin, pairs


def restate(vertices, faces, voxel_size=M.VOXEL_SIZE):
    """B1 - B7 for one object -> Restated"""
    faces = np.asarray(faces).reshape(-1, 3)
    fr = M.frame(vertices, len(faces), voxel_size)                                      # B1 (M1)
    if fr is None:
        return Restated()
    lo, L, cell, D = fr
    unit = M.unit_vertices(vertices, lo, L)
    S = M.pack_words(R.voxelize_surface(unit, faces, D))                                # B2
    n0, n1, margin, pairs = parities(unit, faces, D)
    return Restated(D, lo, cell, S, M.pack_words((n0 & 1).astype(bool)), M.pack_words((n1 & 1).astype(bool)), margin, pairs)


def restate_batch(objects, voxel_size=M.VOXEL_SIZE):
    """objects: [(vertices, faces)] -> dict: dims (N) i32, off (N) i64, frame (N,4) f64, cnt (N,2) i32, words
    (max(sum D^2 W, 1)) u64, margins (N), objects [Restated]"""
    rs = [restate(v, f, voxel_size) if len(v) else Restated() for v, f in objects]
    N = len(rs)
    dims, off, frame, cnt = np.zeros(N, np.int32), np.zeros(N, np.int64), np.zeros((N, 4)), np.zeros((N, 2), np.int32)
    total = 0
    for k, r in enumerate(rs):
        if r.D == 0:
            continue
        dims[k], off[k] = r.D, total
        frame[k, :3], frame[k, 3] = r.lo, r.cell
        cnt[k] = r.cnt
        total += len(r.U)
    words = np.zeros(max(total, 1), np.uint64)
    for k, r in enumerate(rs):
        words[off[k]:off[k] + len(r.U)] = r.U
    return {"dims": dims, "off": off, "frame": frame, "cnt": cnt, "words": words,
            "margins": np.array([r.margin for r in rs]), "objects": rs}
