"""Plain numpy / Python restatement of the detection evaluation, written from the algorithm (not a test module):
oriented-box IoU by Sutherland-Hodgman clipping of the bird's-eye rectangles + shoelace area, the greedy VOC matching
per (scene, class, threshold), and the precision / recall / AP bookkeeping.  It is the CPU yardstick of
rfd_box3d_iou / rfd_ap_match / rfdnet_amd.iscnet.evaluation and is itself pinned to the reference's results in
tests/golden/F_AP.npz (tests/test_evaluation_cpu.py).

Where the reference raises (fewer than 3 clipped points, no area, a zero-volume box) the IoU is 0.
"""
import math

import numpy as np


def get_3d_box(size, heading, center):
    """size (l, w, h), heading about the y axis, centre (x, y, z) in the upright camera frame -> (8,3) corners"""
    l, w, h = (float(v) for v in size)
    c, s = math.cos(heading), math.sin(heading)
    xs = [l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2]
    ys = [h / 2, h / 2, h / 2, h / 2, -h / 2, -h / 2, -h / 2, -h / 2]
    zs = [w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2]
    out = np.empty((8, 3))
    for i in range(8):
        out[i] = (c * xs[i] + s * zs[i] + center[0], ys[i] + center[1], -s * xs[i] + c * zs[i] + center[2])
    return out


def depth_box_corners(center, size, heading):
    """box given in the scan's (depth) frame: centre (x,y,z), size (l,w,h), heading -> upright camera corners"""
    return get_3d_box(size, -heading, (center[0], -center[2], center[1]))


def _rect(c):
    return [(c[i][0], c[i][2]) for i in (3, 2, 1, 0)]


def _rect_area(r):
    s1 = s2 = 0.0
    for i in range(4):
        s1 += r[i][0] * r[i - 1][1]
        s2 += r[i][1] * r[i - 1][0]
    return 0.5 * abs(s1 - s2)


def clip(subject, clipper):
    """Sutherland-Hodgman: `subject` clipped by the convex counter-clockwise `clipper`; strict inside test"""
    out = list(subject)
    cp1 = clipper[-1]
    for cp2 in clipper:
        if not out:
            break
        inp, out = out, []
        ex, ey = cp2[0] - cp1[0], cp2[1] - cp1[1]

        def inside(p):
            return ex * (p[1] - cp1[1]) > ey * (p[0] - cp1[0])
        s = inp[-1]
        s_in = inside(s)
        for e in inp:
            e_in = inside(e)
            if e_in != s_in:
                dcx, dcy = cp1[0] - cp2[0], cp1[1] - cp2[1]
                dpx, dpy = s[0] - e[0], s[1] - e[1]
                n1 = cp1[0] * cp2[1] - cp1[1] * cp2[0]
                n2 = s[0] * e[1] - s[1] * e[0]
                det = dcx * dpy - dcy * dpx
                n3 = 1.0 / det if det != 0.0 else math.inf
                out.append(((n1 * dpx - n2 * dcx) * n3, (n1 * dpy - n2 * dcy) * n3))
            if e_in:
                out.append(e)
            s, s_in = e, e_in
        cp1 = cp2
    return out


def _shoelace(poly):
    if len(poly) < 3:
        return 0.0
    acc = 0.0
    p = poly[-1]
    for q in poly:
        acc += p[0] * q[1] - q[0] * p[1]
        p = q
    a = 0.5 * abs(acc)
    return a if (a > 0.0 and a < 1.0e300) else 0.0


def _edge(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def _vol(c):
    return _edge(c[0], c[1]) * _edge(c[1], c[2]) * _edge(c[0], c[4])


def box3d_iou(c1, c2):
    """(8,3), (8,3) -> (3-D IoU, bird's-eye-view IoU)"""
    if isinstance(c1, np.ndarray):
        c1 = c1.tolist()                             # Python floats: the same doubles, without numpy's scalar overhead
    if isinstance(c2, np.ndarray):
        c2 = c2.tolist()
    r1, r2 = _rect(c1), _rect(c2)
    area1, area2 = _rect_area(r1), _rect_area(r2)
    inter = _shoelace(clip(r1, r2))
    den2 = area1 + area2 - inter
    ymax = min(c1[0][1], c2[0][1])
    ymin = max(c1[4][1], c2[4][1])
    inter_vol = inter * max(0.0, ymax - ymin)
    den3 = _vol(c1) + _vol(c2) - inter_vol
    return (inter_vol / den3 if den3 > 0.0 else 0.0), (inter / den2 if den2 > 0.0 else 0.0)


def box3d_iou_matrix(pred, gt):
    """(K,8,3), (G,8,3) -> iou3d (K,G), iou2d (K,G)"""
    K, G = len(pred), len(gt)
    o3, o2 = np.zeros((K, G)), np.zeros((K, G))
    pred, gt = np.asarray(pred, np.float64).tolist(), np.asarray(gt, np.float64).tolist()
    for k in range(K):
        for g in range(G):
            o3[k, g], o2[k, g] = box3d_iou(pred[k], gt[g])
    return o3, o2


def ap_match(iou3d, order, det_valid, gt_cls, gt_valid, thr):
    """iou3d (b,K,G), order / det_valid (b,C,K), gt_cls / gt_valid (b,G), thr (nT) -> tp (nT,b,C,K) uint8"""
    b, C, K = order.shape
    G = gt_cls.shape[1]
    tp = np.zeros((len(thr), b, C, K), np.uint8)
    for ti, th in enumerate(thr):
        for bi in range(b):
            for c in range(C):
                taken = [False] * G
                gts = [g for g in range(G) if gt_valid[bi, g] and gt_cls[bi, g] == c]
                for d in order[bi, c]:
                    if not det_valid[bi, c, d]:
                        continue
                    ovmax, jmax = -math.inf, -1
                    for g in gts:
                        if iou3d[bi, d, g] > ovmax:
                            ovmax, jmax = iou3d[bi, d, g], g
                    if ovmax > th and not taken[jmax]:
                        taken[jmax] = True
                        tp[ti, bi, c, d] = 1
    return tp


def detection_scores(obj_prob, sem_cls_probs, pred_sem_cls, pred_mask, conf_thresh, per_class_proposal):
    """-> score (b,C,K) float32, valid (b,C,K) bool"""
    obj_prob = np.asarray(obj_prob, np.float32)
    sem = np.asarray(sem_cls_probs, np.float32)
    b, K, C = sem.shape
    take = (np.asarray(pred_mask) == 1) & (obj_prob > conf_thresh)
    if per_class_proposal:
        score = (sem * obj_prob[..., None]).transpose(0, 2, 1)
        valid = np.broadcast_to(take[:, None, :], (b, C, K))
    else:
        score = np.broadcast_to(obj_prob[:, None, :], (b, C, K))
        valid = take[:, None, :] & (np.asarray(pred_sem_cls)[:, None, :] == np.arange(C)[None, :, None])
    return np.ascontiguousarray(score, np.float32), np.ascontiguousarray(valid)


def scene_records(pred_corners, obj_prob, sem_cls_probs, pred_sem_cls, pred_mask, gt_corners, gt_cls, gt_valid,
                  thr=(0.25, 0.5), conf_thresh=0.05, per_class_proposal=True, iou3d=None):
    """-> records {'cls' (n), 'score' (n) f32, 'tp' (nT,n) u8, 'npos' (C), 'thr'} + the dense tp (nT,b,C,K)"""
    score, valid = detection_scores(obj_prob, sem_cls_probs, pred_sem_cls, pred_mask, conf_thresh, per_class_proposal)
    b, C, K = score.shape
    if iou3d is None:
        iou3d = np.zeros((b, K, gt_corners.shape[1]))
        for bi in range(b):
            gi = np.nonzero(gt_valid[bi])[0]
            ki = np.nonzero(valid[bi].any(0))[0]
            for k in ki:
                for g in gi:
                    iou3d[bi, k, g] = box3d_iou(pred_corners[bi, k], gt_corners[bi, g])[0]
    order = np.argsort(-score, axis=-1, kind='stable')
    tp = ap_match(iou3d, order, valid, np.asarray(gt_cls), np.asarray(gt_valid), thr)
    bi, ci, ki = np.nonzero(valid)
    npos = np.array([int(((np.asarray(gt_cls) == c) & (np.asarray(gt_valid) != 0)).sum()) for c in range(C)])
    rec = {'cls': ci.astype(np.int32), 'score': score[bi, ci, ki], 'tp': tp[:, bi, ci, ki], 'npos': npos,
           'thr': tuple(thr)}
    return rec, tp


def voc_ap(rec, prec, use_07_metric=True):
    """VOC 2007: mean over the recall levels k * 0.1, k = 0..10 (floating-point products: 3 * 0.1 is
    0.30000000000000004, which a recall of exactly 0.3 does not reach) of the best precision at or beyond the level.
    All points: sum over the detections of (recall step) x (best precision from this detection on)."""
    n = len(rec)
    if use_07_metric:
        total = 0.0
        for k in range(11):
            level = k * 0.1
            best = 0.0
            for i in range(n):
                if rec[i] >= level and prec[i] > best:
                    best = float(prec[i])
            total += best
        return total / 11.0
    area, best, steps = 0.0, 0.0, []
    for i in range(n - 1, -1, -1):                   # walk back: the envelope at i is known when i is reached
        best = max(best, float(prec[i]))
        steps.append((float(rec[i]) - (float(rec[i - 1]) if i else 0.0)) * best)
    for v in reversed(steps):
        area += v
    return area


def class_curves(records, ti, use_07_metric=True):
    """records: list of record dicts -> {cls: (rec, prec, ap, sorted tp flags)}; a class with ground truths and no
    detection maps to (0, 0, 0, [])"""
    cls = np.concatenate([r['cls'] for r in records])
    score = np.concatenate([r['score'] for r in records])
    tp = np.concatenate([r['tp'][ti] for r in records])
    npos = sum(np.asarray(r['npos'], np.int64) for r in records)
    out = {}
    for c in range(len(npos)):
        m = cls == c
        if not m.any():
            if npos[c] > 0:
                out[c] = (0, 0, 0, np.zeros(0, np.uint8))
            continue
        o = np.argsort(-score[m], kind='stable')
        flags = tp[m][o]
        tpc = np.cumsum(flags.astype(np.float64))
        fpc = np.cumsum(1.0 - flags.astype(np.float64))
        with np.errstate(divide='ignore', invalid='ignore'):
            rec = tpc / float(npos[c])
        prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
        out[c] = (rec, prec, voc_ap(rec, prec, use_07_metric), flags)
    return out


def metrics(records, ti, class2type=None, use_07_metric=True):
    cur = class_curves(records, ti, use_07_metric)
    name = lambda c: class2type[c] if class2type else str(c)
    ret = {}
    for c in sorted(cur):
        ret['%s Average Precision' % name(c)] = cur[c][2]
    ret['mAP'] = np.mean([cur[c][2] for c in sorted(cur)])
    recs = []
    for c in sorted(cur):
        r = cur[c][0][-1] if np.ndim(cur[c][0]) else 0
        ret['%s Recall' % name(c)] = r
        recs.append(r)
    ret['AR'] = np.mean(recs)
    return ret
