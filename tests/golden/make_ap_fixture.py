"""Writes tests/golden/F_AP.npz: detection-evaluation cases scored by the REFERENCE's own code
(net_utils/box_util.py box3d_iou, net_utils/eval_det.py, net_utils/ap_helper.py), imported where it lies.
Run in the development container only (the reference must be importable); the fixture holds arrays only.

    python tests/golden/make_ap_fixture.py

Scenes (K = 256 proposals, 8 classes, G = 64 ground-truth slots):
  0-2  ground truths = perturbed copies of a subset of the surviving proposals (centre sigma 0.15 m, size x U(0.8,
       1.25), heading sigma 0.2 rad) + a few unrelated boxes; near-duplicate proposals of the same class are added so
       that true positives, duplicates and misses all occur
  3    all-zero pred_mask (ground truths present)
  4    no ground truth (detections present)
Class 7 has no ground truth anywhere (predictions, no ground truth).  Class 6 has ground truths and is never a
proposal's arg-max class: with per_class_proposal False it is the class with ground truths and no prediction (with
per_class_proposal True every class is scored for every proposal, so no such class can exist).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_fixtures as mf  # noqa: E402

S, K, C, G = 5, 256, 8, 64
THRESHOLDS = (0.25, 0.5)
CONF = 0.05


class SerialPool(object):
    """eval_det_multiprocessing_wo_mesh's Pool, serially"""

    def __init__(self, processes=None):
        pass

    def map(self, fn, args):
        return [fn(a) for a in args]

    def close(self):
        pass

    def join(self):
        pass


def main():
    import torch
    mf.mount_reference()
    tm = sys.modules['trimesh']
    ex = mf.ns('trimesh.exchange')
    bx = mf.ns('trimesh.exchange.binvox')
    bx.voxelize_mesh = None
    tm.exchange = ex
    ex.binvox = bx
    ap = importlib.import_module('net_utils.ap_helper')
    box_util = importlib.import_module('net_utils.box_util')
    eval_det = importlib.import_module('net_utils.eval_det')
    libs = importlib.import_module('net_utils.libs')
    eval_det.Pool = SerialPool
    from rfdnet_amd.iscnet.config import ScannetConfig
    mean_size_arr = np.load(os.path.join(HERE, "F_NMS.npz"))['mean_size_arr']

    class DC(ScannetConfig):                       # scannet_config.py:43-73
        def class2angle(self, pred_cls, residual, to_label_format=True):
            angle = pred_cls * (2 * np.pi / float(self.num_heading_bin)) + residual
            if to_label_format and angle > np.pi:
                angle = angle - 2 * np.pi
            return angle

        def class2size(self, pred_cls, residual):
            return self.mean_size_arr[pred_cls, :] + residual

    dc = DC(mean_size_arr)
    rng = np.random.default_rng(41)

    # ---- predictions ------------------------------------------------------------------------------------------
    center = np.stack([rng.uniform(-2.6, 2.6, (S, K)), rng.uniform(-3.1, 3.1, (S, K)), rng.uniform(0.2, 1.2, (S, K))], -1)
    size = rng.uniform(0.4, 1.6, (S, K, 3))
    heading = rng.uniform(-np.pi, np.pi, (S, K))
    sem_logits = rng.normal(0, 1.5, (S, K, C)).astype(np.float32)
    sem_logits[..., 6] -= 12.0                      # class 6 is never the arg-max
    obj_logits = rng.normal(0.5, 2.0, (S, K, 2)).astype(np.float32)
    pred_mask = (rng.random((S, K)) < 0.45).astype(np.uint8)
    # near duplicates: proposal 2i+1 repeats proposal 2i (same class) for the first 40 pairs
    for i in range(40):
        a, b = 2 * i, 2 * i + 1
        center[:, b] = center[:, a] + rng.normal(0, 0.05, (S, 3))
        size[:, b] = size[:, a] * rng.uniform(0.95, 1.05, (S, 3))
        heading[:, b] = heading[:, a] + rng.normal(0, 0.05, S)
        sem_logits[:, b] = sem_logits[:, a] + rng.normal(0, 0.05, (S, C)).astype(np.float32)
        pred_mask[:, a] = pred_mask[:, b] = 1
    pred_mask[3] = 0
    sem_cls_probs = libs.softmax(sem_logits)
    obj_prob = libs.softmax(obj_logits)[:, :, 1]
    pred_sem_cls = np.argmax(sem_logits, -1)
    assert (pred_sem_cls != 6).all() and (pred_sem_cls == 7).any()
    cam = libs.flip_axis_to_camera(center)
    corners = np.zeros((S, K, 8, 3))
    for s in range(S):
        for k in range(K):
            corners[s, k] = box_util.get_3d_box(size[s, k], -heading[s, k], cam[s, k])

    # ---- ground-truth labels ----------------------------------------------------------------------------------
    nh = dc.num_heading_bin
    gt = {'center_label': np.zeros((S, G, 3), np.float32), 'heading_class_label': np.zeros((S, G), np.int64),
          'heading_residual_label': np.zeros((S, G), np.float32), 'size_class_label': np.zeros((S, G), np.int64),
          'size_residual_label': np.zeros((S, G, 3), np.float32), 'sem_cls_label': np.zeros((S, G), np.int64),
          'box_label_mask': np.zeros((S, G), np.float32)}
    for s in range(S):
        if s == 4:
            continue
        src_mask = pred_mask[s] if s != 3 else (rng.random(K) < 0.45)
        surv = np.nonzero((src_mask == 1) & (obj_prob[s] > CONF))[0]
        pick = rng.permutation(surv)[:min(len(surv) // 2, G - 8)]
        boxes = [(center[s, k] + rng.normal(0, 0.15, 3), size[s, k] * rng.uniform(0.8, 1.25, 3),
                  heading[s, k] + rng.normal(0, 0.2), int(pred_sem_cls[s, k])) for k in pick]
        boxes += [(np.array([rng.uniform(-2.6, 2.6), rng.uniform(-3.1, 3.1), rng.uniform(0.2, 1.2)]),
                   rng.uniform(0.4, 1.6, 3), rng.uniform(-np.pi, np.pi), int(rng.integers(0, 7))) for _ in range(8)]
        for j, (ctr, sz, ang, cls) in enumerate(boxes):
            if cls == 7:
                cls = 6                              # class 7: no ground truth anywhere
            if j % 9 == 4:
                cls = 6                              # class 6: ground truths, never predicted (arg-max)
            a = ang % (2 * np.pi)
            shifted = (a + np.pi / nh) % (2 * np.pi)
            hc = int(shifted / (2 * np.pi / nh))
            sc = int(rng.integers(0, dc.num_size_cluster))
            gt['center_label'][s, j] = ctr
            gt['heading_class_label'][s, j] = hc
            gt['heading_residual_label'][s, j] = shifted - (hc * (2 * np.pi / nh) + np.pi / nh)
            gt['size_class_label'][s, j] = sc
            gt['size_residual_label'][s, j] = sz - mean_size_arr[sc]
            gt['sem_cls_label'][s, j] = cls
            gt['box_label_mask'][s, j] = 1
    assert not (gt['sem_cls_label'][gt['box_label_mask'] == 1] == 7).any()
    assert (gt['sem_cls_label'][gt['box_label_mask'] == 1] == 6).any()
    parsed_gts = ap.parse_groundtruths({k: torch.from_numpy(v) for k, v in gt.items()}, {'dataset_config': dc})
    gt_corners = parsed_gts['gt_corners_3d_upright_camera']
    gt_valid = gt['box_label_mask'] == 1

    # ---- the reference's IoU for every (proposal, valid ground truth) pair -------------------------------------
    iou3d = np.zeros((S, K, G))
    iou2d = np.zeros((S, K, G))
    for s in range(S):
        for k in range(K):
            for g in np.nonzero(gt_valid[s])[0]:
                iou3d[s, k, g], iou2d[s, k, g] = box_util.box3d_iou(corners[s, k], gt_corners[s, g])   # must not raise
    v = iou3d[np.broadcast_to(gt_valid[:, None, :], iou3d.shape)]
    for t in THRESHOLDS:
        assert np.abs(v - t).min() > 1e-6, "an IoU lies within 1e-6 of %g" % t
    assert np.isfinite(iou3d).all() and np.isfinite(iou2d).all()

    out = {'corners': corners, 'sem_cls_probs': sem_cls_probs, 'obj_prob': obj_prob, 'pred_sem_cls': pred_sem_cls,
           'pred_mask': pred_mask, 'gt_corners': gt_corners, 'iou3d': iou3d, 'iou2d': iou2d,
           'mean_size_arr': mean_size_arr, 'thresholds': np.array(THRESHOLDS), 'conf_thresh': np.array(CONF)}
    out.update({'gt_' + k: v for k, v in gt.items()})

    # ---- the reference's records and metrics, both per_class_proposal settings -------------------------------
    parsed = {'pred_corners_3d_upright_camera': corners, 'sem_cls_probs': sem_cls_probs, 'obj_prob': obj_prob,
              'pred_sem_cls': torch.from_numpy(pred_sem_cls)}
    batch_gt_map_cls = ap.assembly_gt_map_cls({'sem_cls_label': torch.from_numpy(gt['sem_cls_label']),
                                               'gt_corners_3d_upright_camera': gt_corners,
                                               'box_label_mask': torch.from_numpy(gt['box_label_mask'])})
    for tag, pcp in (("pcp1", True), ("pcp0", False)):
        cfg = {'per_class_proposal': pcp, 'conf_thresh': CONF, 'dataset_config': dc}
        ed = ap.assembly_pred_map_cls({'pred_mask': pred_mask}, parsed, cfg)
        bp = ed['batch_pred_map_cls']
        # the reference's list, as arrays: scene, class, proposal index (found by identity of the box), score
        rows = []
        for s, lst in enumerate(bp):
            take = [j for j in range(K) if pred_mask[s, j] == 1 and obj_prob[s, j] > CONF]
            for n, (cls, box, score) in enumerate(lst):
                j = take[n % len(take)] if pcp else take[n]
                assert box is not None and np.array_equal(box, corners[s, j])
                rows.append((s, int(cls), j, np.float32(score)))
        out[tag + '_scene'] = np.array([r[0] for r in rows], np.int32)
        out[tag + '_cls'] = np.array([r[1] for r in rows], np.int32)
        out[tag + '_idx'] = np.array([r[2] for r in rows], np.int32)
        out[tag + '_score'] = np.array([r[3] for r in rows], np.float32)
        for c in range(C):
            sc = out[tag + '_score'][out[tag + '_cls'] == c]
            assert len(np.unique(sc)) == len(sc), "equal scores within class %d" % c
        for t in THRESHOLDS:
            pred_all = {i: bp[i] for i in range(S)}
            gt_all = {i: batch_gt_map_cls[i] for i in range(S)}
            with np.errstate(divide='ignore', invalid='ignore'):
                rec, prec, apv = eval_det.eval_det_multiprocessing_wo_mesh(pred_all, gt_all, ovthresh=t,
                                                                           get_iou_func=eval_det.get_iou_obb)
                _, _, ap_all = eval_det.eval_det_multiprocessing_wo_mesh(pred_all, gt_all, ovthresh=t, use_07_metric=False,
                                                                         get_iou_func=eval_det.get_iou_obb)
                calc = ap.APCalculator(t, None)
                calc.step(bp, batch_gt_map_cls)
                md = calc.compute_metrics()
            key = "%s_%g" % (tag, t)
            out[key + '_classes'] = np.array(sorted(apv.keys()), np.int32)
            for c in apv:
                out['%s_rec_%d' % (key, c)] = np.asarray(rec[c], np.float64)
                out['%s_prec_%d' % (key, c)] = np.asarray(prec[c], np.float64)
                out['%s_ap_%d' % (key, c)] = np.asarray(apv[c], np.float64)
                out['%s_apall_%d' % (key, c)] = np.asarray(ap_all[c], np.float64)      # use_07_metric=False
                if np.ndim(prec[c]):
                    # true-positive flags in the reference's sorted order: tp + fp = d + 1 at detection d
                    tpc = np.rint(np.asarray(prec[c]) * np.arange(1, len(prec[c]) + 1))
                    out['%s_tp_%d' % (key, c)] = np.diff(np.concatenate([[0.], tpc])).astype(np.uint8)
            out[key + '_metric_keys'] = np.array(list(md.keys()))
            out[key + '_metric_values'] = np.array([float(md[k]) for k in md], np.float64)
            print(key, "mAP %.4f AR %.4f" % (md['mAP'], md['AR']), "classes", sorted(apv.keys()),
                  "all-points AP", [round(float(ap_all[c]), 4) for c in sorted(ap_all)])
    path = os.path.join(HERE, "F_AP.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; valid gts per scene", gt_valid.sum(1),
          "detections per scene", ((pred_mask == 1) & (obj_prob > CONF)).sum(1))


if __name__ == "__main__":
    main()
