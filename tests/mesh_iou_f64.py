"""Numpy restatement of include/rfd_mesh_eval.h, rules M1 - M5 (no test in here; tests/test_mesh_eval_cpu.py and
tests/test_gpu_mesh_eval.py import it).  numpy evaluates every operation on its own, in float64, left to right as the
rules write them.  It is pinned to the reference's compute_mesh_iou by tests/golden/F_MIOU.npz."""
import numpy as np

VOXEL_SIZE = 0.047
MAX_D = 256


def frame(vertices, n_faces=1, voxel_size=VOXEL_SIZE):
    """M1: placed vertices (V,3) -> (lo (3,) f64, L, cell, D), or None for an object without grid"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    if v.shape[0] == 0 or n_faces == 0:
        return None
    lo, hi = v.min(0), v.max(0)
    return frame_of_extent(lo, hi, voxel_size)


def frame_of_extent(lo, hi, voxel_size=VOXEL_SIZE):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        L = np.max(hi - lo)
    if not np.isfinite(L) or L == 0:
        return None
    D = max(int(L / voxel_size), 2)
    if D > MAX_D:
        raise ValueError("D = %d > %d" % (D, MAX_D))
    return lo, L, L / D, D


def unit_vertices(vertices, lo, L):
    """M2's map to the unit cube"""
    return (np.asarray(vertices, np.float64) - lo) / L - 0.5


def centres(grid, lo, cell):
    """M3: the world centres of the set voxels of a (D,D,D) bool grid, in C order -> (n,3)"""
    idx = np.argwhere(grid)
    return lo + (idx + 0.5) * cell


def is_filled(grid, lo, cell, points):
    """M4 -> (n,) bool"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    D = grid.shape[0]
    with np.errstate(invalid='ignore'):
        t = np.floor((points - lo) / cell)
        ok = ((t >= 0) & (t < D)).all(1)
    out = np.zeros(len(points), bool)
    ti = t[ok].astype(np.int64)
    out[ok] = grid[ti[:, 0], ti[:, 1], ti[:, 2]]
    return out


class Obj(object):
    """one object: S, I (D,D,D) bool, lo (3,), cell; S = None: no grid"""

    def __init__(self, S=None, I=None, lo=None, cell=None):
        self.S, self.I, self.lo, self.cell = S, I, lo, cell
        self.U = None if S is None else (S | I)
        self._centres = None

    def centres(self):
        if self._centres is None:
            self._centres = centres(self.U, self.lo, self.cell)
        return self._centres


def counts(a, b):
    """-> (a_AB, a_BA)"""
    if a.U is None or b.U is None:
        return 0, 0
    ab = int(is_filled(b.U, b.lo, b.cell, a.centres()).sum())
    ba = int(is_filled(a.U, a.lo, a.cell, b.centres()).sum())
    return ab, ba


def iou_from_counts(a_ab, a_ba, n_a, n_b, s_a, s_b):
    """M5"""
    if s_a == 0 or s_b == 0 or a_ab == 0 or a_ba == 0:
        return 0.0
    a1, a2 = a_ab / n_a, a_ba / n_b
    return (a1 * a2) / (a1 + a2 - a1 * a2)


def iou_matrix(preds, gts):
    """lists of Obj -> iou (P,G) f64, counts (P,G,2) i32"""
    P, G = len(preds), len(gts)
    iou, cnt = np.zeros((P, G)), np.zeros((P, G, 2), np.int32)
    for p, a in enumerate(preds):
        for g, b in enumerate(gts):
            ab, ba = counts(a, b)
            cnt[p, g] = ab, ba
            if a.U is not None and b.U is not None:
                iou[p, g] = iou_from_counts(ab, ba, int(a.U.sum()), int(b.U.sum()), int(a.S.sum()), int(b.S.sum()))
    return iou, cnt


def pack_words(U):
    """(D,D,D) bool -> (D*D*W,) uint64: bit k & 63 of word k >> 6 of row i * D + j"""
    D = U.shape[0]
    W = (D + 63) // 64
    bits = np.zeros((D, D, W * 64), np.uint64)
    bits[:, :, :D] = U
    return (bits.reshape(D, D, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).reshape(-1)


def voxelize(vertices, faces, voxel_size=VOXEL_SIZE):
    """M1 + M2 on tests/mesh_sample_ref.py -> Obj"""
    import mesh_sample_ref as R
    faces = np.asarray(faces).reshape(-1, 3)
    fr = frame(vertices, len(faces), voxel_size)
    if fr is None:
        return Obj()
    lo, L, cell, D = fr
    v = unit_vertices(vertices, lo, L)
    S = R.voxelize_surface(v, faces, D)
    I = R.voxelize_interior(v, faces, D, np.zeros((D ** 3, 3)))
    return Obj(np.asarray(S, bool), np.asarray(I, bool).reshape(D, D, D), lo, cell)


def fixture_objects(fx):
    """tests/golden/F_MIOU.npz -> the list of Obj, indexed as its pred_obj / gt_obj arrays index them"""
    out = []
    for i, D in enumerate(fx['D']):
        D = int(D)
        grid = lambda a: np.unpackbits(a)[:D ** 3].reshape(D, D, D).astype(bool)
        out.append(Obj(grid(fx['S_%d' % i]), grid(fx['I_%d' % i]), fx['lo'][i].copy(), float(fx['cell'][i])))
    return out
