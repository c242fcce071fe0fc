"""Writes tests/golden/F_MIOU.npz: the reference's own mesh IoU and mesh / box true-positive flags on hand-made voxel
grids.  Run on the CPU where the reference lies (never shipped):

    python tests/golden/make_fixtures_mesh_iou.py

It imports the reference's compute_mesh_iou and eval_det_multiprocessing_w_mesh (net_utils/eval_det.py: numpy and
scipy only) and feeds them stand-in voxel objects -- the reference only asks a voxel object for `.points`,
`.is_filled(points)` and `.filled_count`.  The stand-ins answer by rules M3 and M4 of include/rfd_mesh_eval.h over
boolean arrays, in this script's own numpy.  Recorded: the grids (bit-packed), the frames, the reference's IoU of
every (prediction, ground truth) pair of a scene, the lookup counts (taken with the very calls the reference makes),
and for per_class_proposal on / off at IoU 0.25 and 0.5 the reference's rec / prec / ap per class for boxes and meshes
with the flags in score order (the increments of rec * npos).

Two scenes, three classes, 13 predictions and 8 ground truths with D from 2 to 130.  Edge cases: D = 2, 63, 64, 65,
130; an object against itself; disjoint cubes; a nested object; incommensurate cells (D = 12 over 1.0 against D = 9
over 1.3, shifted); source centres exactly on the target's cell boundaries and outer faces (binary-exact frames); an
object with empty S; a thin plate with empty I.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import eval_det_f64 as E  # noqa: E402   (box corners only)

THR = (0.25, 0.5)
CONF = 0.05
C = 3


class Vox(object):
    """what the reference asks of a trimesh VoxelGrid, by rules M3 / M4"""

    def __init__(self, grid, lo, cell):
        self.grid, self.lo, self.cell = grid, np.asarray(lo, np.float64), float(cell)
        self.filled_count = int(grid.sum())

    @property
    def points(self):
        return self.lo + (np.argwhere(self.grid) + 0.5) * self.cell

    def is_filled(self, points):
        D = self.grid.shape[0]
        t = np.floor((np.asarray(points, np.float64).reshape(-1, 3) - self.lo) / self.cell)
        ok = ((t >= 0) & (t < D)).all(1)
        out = np.zeros(len(t), bool)
        ti = t[ok].astype(np.int64)
        out[ok] = self.grid[ti[:, 0], ti[:, 1], ti[:, 2]]
        return out


# ---- shapes on a D^3 grid -> (S, I) ----------------------------------------------------------------------------------
def block(D, a, b):
    """the block [a, b)^3: S its boundary layer, I the rest of it"""
    full = np.zeros((D, D, D), bool)
    full[a:b, a:b, a:b] = True
    inner = np.zeros_like(full)
    inner[a + 1:b - 1, a + 1:b - 1, a + 1:b - 1] = True
    return full & ~inner, inner


def ball(D, r=0.45):
    c = (np.arange(D) + 0.5) / D - 0.5
    d = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return np.abs(d - r) < 0.75 / D, d < r


def shell_with_core(D):
    """a hollow box with a small solid core: few voxels for a large D"""
    S, _ = block(D, 0, D)
    I = np.zeros_like(S)
    I[D // 3:D // 2, D // 3:D // 2, D // 4:D - 3] = True
    return S, I


def plate(D, k):
    S = np.zeros((D, D, D), bool)
    S[2:D - 2, 1:D - 1, k] = True
    return S, np.zeros_like(S)


def objects():
    """-> list of dicts: S, I, lo, cell, cls, and which scene / side the object is on"""
    o = []

    def add(scene, side, cls, SI, lo, cell):
        o.append(dict(scene=scene, side=side, cls=cls, S=SI[0], I=SI[1], lo=np.asarray(lo, np.float64), cell=float(cell)))
    # scene 0, ground truths
    add(0, 'gt', 0, ball(12), (0, 0, 0), 1.0 / 12)
    add(0, 'gt', 1, block(64, 0, 64), (2, 0, 0), 1.0 / 64)
    add(0, 'gt', 2, shell_with_core(130), (4, 0, 0), 1.0 / 128)
    add(0, 'gt', 0, block(2, 0, 2), (0, 2, 0), 0.5)
    add(0, 'gt', 1, block(8, 1, 8), (2, 2, 0), 0.125)
    # scene 0, predictions
    # incommensurate with the D = 12 ball; of another class than it: only per_class_proposal scores it for class 0
    add(0, 'pred', 2, ball(9), (-0.1, 0.05, -0.2), 1.3 / 9)
    add(0, 'pred', 1, block(63, 2, 60), (2.01, 0.003, -0.004), 1.0 / 63)
    add(0, 'pred', 2, shell_with_core(130), (4, 0, 0), 1.0 / 128)           # the ground truth itself
    # centres at 2 + i / 64: exactly on the cell boundaries of the D = 64 block, i = 0 on its lo face (inside),
    # i = 64 on its lo + L face (outside)
    add(0, 'pred', 1, block(65, 0, 65), (2 - 1.0 / 128, -1.0 / 128, -1.0 / 128), 1.0 / 64)
    add(0, 'pred', 1, block(4, 0, 4), (2.25, 2.25, 0.25), 0.0625)           # nested in the D = 8 block
    add(0, 'pred', 2, block(5, 0, 5), (50, 50, 50), 0.2)                    # far away from everything
    SI = block(6, 1, 5)
    add(0, 'pred', 0, (np.zeros_like(SI[0]), SI[0] | SI[1]), (0.2, 0.2, 0.2), 0.1)   # empty S
    add(0, 'pred', 1, plate(16, 2), (2, 2, 0.4), 1.0 / 16)                  # empty I
    # scene 1
    add(1, 'gt', 2, ball(65), (0, 0, 0), 0.03)
    add(1, 'gt', 0, block(20, 0, 20), (3, 0, 0), 0.05)
    add(1, 'gt', 1, ball(10), (0, 3, 0), 0.1)
    add(1, 'pred', 2, ball(64), (0.02, -0.01, 0.03), 0.031)
    add(1, 'pred', 0, block(21, 1, 20), (3.02, 0.01, -0.02), 0.047)
    add(1, 'pred', 1, ball(10), (0, 3, 0), 0.1)                             # the ground truth itself
    add(1, 'pred', 0, block(7, 0, 7), (3.5, 0.3, 0.2), 0.1)
    add(1, 'pred', 1, block(3, 0, 3), (0.1, 3.2, 0.1), 0.2)
    return o


def box_of(obj, rng, jitter):
    """a box about the object's cube, in the upright camera frame; predictions are perturbed so that no two boxes
    have coincident edges (the reference's clip is ill-posed there)"""
    L = obj['cell'] * obj['S'].shape[0]
    centre = obj['lo'] + L / 2
    size = np.full(3, L)
    heading = 0.0
    if jitter:
        centre = centre + rng.normal(0, 0.04 * L, 3)
        size = size * rng.uniform(0.85, 1.1, 3)
        heading = rng.uniform(0.05, 0.3)
    return E.depth_box_corners(centre, size, heading)


def main():
    from net_utils import eval_det
    eval_det.Pool = None                      # the serial branch of its try / except: the stand-ins stay in this process
    rng = np.random.default_rng(5)
    objs = objects()
    N = len(objs)
    B = 2
    pred_ids = [[i for i, o in enumerate(objs) if o['scene'] == s and o['side'] == 'pred'] for s in range(B)]
    gt_ids = [[i for i, o in enumerate(objs) if o['scene'] == s and o['side'] == 'gt'] for s in range(B)]
    K, G = max(map(len, pred_ids)), max(map(len, gt_ids))
    vox = [(Vox(o['I'], o['lo'], o['cell']), Vox(o['S'], o['lo'], o['cell'])) for o in objs]     # (internal, surface)

    memo = {}

    def mesh_iou(a, b):                       # a, b: object indices; the reference's function, once per pair
        if (a, b) not in memo:
            memo[(a, b)] = eval_det.compute_mesh_iou(vox[a], vox[b])
        return memo[(a, b)]

    pred_obj = -np.ones((B, K), np.int32)
    gt_obj = -np.ones((B, G), np.int32)
    corners = np.zeros((B, K, 8, 3))
    gt_corners = np.zeros((B, G, 8, 3))
    sem = np.zeros((B, K, C), np.float32)
    obj_prob = np.zeros((B, K), np.float32)
    pred_mask = np.zeros((B, K), np.int64)
    gt_cls = np.zeros((B, G), np.int64)
    gt_mask = np.zeros((B, G), np.float32)
    iou_mesh = np.zeros((B, K, G))
    counts = np.zeros((B, K, G, 2), np.int32)
    for s in range(B):
        for g, i in enumerate(gt_ids[s]):
            gt_obj[s, g], gt_cls[s, g], gt_mask[s, g] = i, objs[i]['cls'], 1
            gt_corners[s, g] = box_of(objs[i], rng, False)
        for k, i in enumerate(pred_ids[s]):
            pred_obj[s, k], pred_mask[s, k] = i, 1
            corners[s, k] = box_of(objs[i], rng, True)
            p = rng.uniform(0.05, 0.2, C)
            p[objs[i]['cls']] = rng.uniform(0.6, 0.9)
            sem[s, k] = (p / p.sum()).astype(np.float32)
            obj_prob[s, k] = rng.uniform(0.3, 0.99)
            for g, j in enumerate(gt_ids[s]):
                iou_mesh[s, k, g] = mesh_iou(i, j)
                (ai, as_), (bi, bs) = vox[i], vox[j]
                pa = np.vstack([ai.points, as_.points[~ai.is_filled(as_.points)]])
                pb = np.vstack([bi.points, bs.points[~bi.is_filled(bs.points)]])
                counts[s, k, g] = (bs.is_filled(pa) | bi.is_filled(pa)).sum(), (as_.is_filled(pb) | ai.is_filled(pb)).sum()
    obj_prob[0, 5] = 0.01                      # the far-away object does not take part (below conf_thresh)
    pred_cls = sem.argmax(-1).astype(np.int64)
    take = (pred_mask == 1) & (obj_prob > CONF)

    out = {'D': np.array([o['S'].shape[0] for o in objs], np.int32), 'lo': np.stack([o['lo'] for o in objs]),
           'cell': np.array([o['cell'] for o in objs]), 'obj_cls': np.array([o['cls'] for o in objs], np.int32),
           'pred_obj': pred_obj, 'gt_obj': gt_obj, 'corners': corners, 'gt_corners': gt_corners, 'sem_cls_probs': sem,
           'obj_prob': obj_prob, 'pred_sem_cls': pred_cls, 'pred_mask': pred_mask, 'gt_sem_cls_label': gt_cls,
           'gt_box_label_mask': gt_mask, 'mesh_iou': iou_mesh, 'counts': counts, 'conf_thresh': np.float64(CONF),
           'thr': np.array(THR)}
    for i, o in enumerate(objs):
        out['S_%d' % i], out['I_%d' % i] = np.packbits(o['S']), np.packbits(o['I'])

    iou3d = np.zeros((B, K, G))
    for s in range(B):
        for k in range(len(pred_ids[s])):
            for g in range(len(gt_ids[s])):
                iou3d[s, k, g] = eval_det.get_iou_obb(corners[s, k], gt_corners[s, g])
    out['iou3d'] = iou3d
    for m, name in ((iou3d, 'box'), (iou_mesh, 'mesh')):
        live = m[(m > 0) & (m < 1)]
        assert np.abs(live[:, None] - np.array(THR)[None]).min() > 1e-6, "%s IoU within 1e-6 of a threshold" % name

    for tag, pcp in (("pcp1", True), ("pcp0", False)):
        pred_all, gt_all = {}, {}
        for s in range(B):
            js = [k for k in range(K) if take[s, k]]
            if pcp:
                pred_all[s] = [(c, corners[s, k], sem[s, k, c] * obj_prob[s, k], int(pred_obj[s, k]))
                               for c in range(C) for k in js]
            else:
                pred_all[s] = [(int(pred_cls[s, k]), corners[s, k], obj_prob[s, k], int(pred_obj[s, k])) for k in js]
            gt_all[s] = [(int(gt_cls[s, g]), gt_corners[s, g], int(gt_obj[s, g])) for g in range(G) if gt_mask[s, g] == 1]
        scores = np.array([p[2] for lst in pred_all.values() for p in lst])
        assert len(np.unique(scores)) == len(scores), "tied scores"
        npos = np.array([sum(1 for lst in gt_all.values() for g in lst if g[0] == c) for c in range(C)])
        assert (npos > 0).all() and {p[0] for lst in pred_all.values() for p in lst} == set(range(C))
        for t in THR:
            with contextlib.redirect_stdout(io.StringIO()):
                (rec, prec, ap), (rec_m, prec_m, ap_m) = eval_det.eval_det_multiprocessing_w_mesh(
                    pred_all, gt_all, ovthresh=t, get_iou_func=eval_det.get_iou_obb, get_iou_mesh=mesh_iou)
            key = "%s_%g" % (tag, t)
            metric = {}
            for sfx, r_, p_, a_ in (('', rec, prec, ap), ('_mesh', rec_m, prec_m, ap_m)):
                for c in sorted(a_):
                    out['%s_rec%s_%d' % (key, sfx, c)] = np.asarray(r_[c], np.float64)
                    out['%s_prec%s_%d' % (key, sfx, c)] = np.asarray(p_[c], np.float64)
                    out['%s_tp%s_%d' % (key, sfx, c)] = np.diff(np.rint(np.asarray(r_[c]) * npos[c]), prepend=0).astype(np.uint8)
                    metric['%d Average Precision%s' % (c, sfx)] = a_[c]       # ap_helper.py:93-122's keys and means
                metric['mAP' + sfx] = np.mean(list(a_.values()))
                for c in sorted(a_):
                    metric['%d Recall%s' % (c, sfx)] = r_[c][-1]
                metric['AR' + sfx] = np.mean([r_[c][-1] for c in sorted(a_)])
            out[key + '_metric_keys'] = np.array(list(metric.keys()))
            out[key + '_metric_values'] = np.array(list(metric.values()), np.float64)
            print(key, {k: round(float(v), 4) for k, v in metric.items() if k.startswith(('mAP', 'AR'))})
    path = os.path.join(HERE, "F_MIOU.npz")
    np.savez_compressed(path, **out)
    print("%s: %d objects, %d bytes; mesh IoU\n%s" % (path, N, os.path.getsize(path), np.round(iou_mesh, 4)))


if __name__ == "__main__":
    main()
