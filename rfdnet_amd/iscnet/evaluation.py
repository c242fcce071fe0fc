"""Detection evaluation: oriented-box IoU and true-positive matching on the device, mAP / AR on the host -- the
counterpart of the tail of the reference's `--mode test` sweep:

  parse_groundtruths   net_utils/ap_helper.py:326-368
  scene_records        assembly_pred_map_cls + assembly_gt_map_cls without meshes (:267-323, :371-401) and the
                       per-scene part of eval_det_cls_wo_mesh (net_utils/eval_det.py:304-331)
  APCalculator         ap_helper.py:25-82 over eval_det.py:259-343, :424-473

The reference moves every head output to the host, calls scipy's ConvexHull once per (detection, ground truth)
pair and opens a multiprocessing Pool.  The ground truths' `det` flags are per scene and per class, so the matching is
independent for each (scene, class, threshold) and runs where the boxes are: two kernels per scene
(csrc/box_eval.hip) and one small device-to-host copy the host does not wait for; only the global sort by confidence and the cumulative sums are
left to the host (compute_metrics).

Deviations from the reference, both on inputs it cannot score: a pair on which scipy raises QhullError (no
intersection area, a zero-volume box) has IoU 0; `evaluate_mesh=True` is not available (see APCalculator).
Boxes with exactly coincident edges (exact copies, boxes touching along a face) are ill-posed for the reference's clip --
its own IoU is arbitrary there, above 1 at times -- and the kernel's value, though finite, is no better (include/rfd_eval.h).
A class with predictions and no ground truth has AP 0 and -- as in the reference, whose recall is 0 / 0 there -- a
NaN recall, which makes 'AR' NaN.
"""
import numpy as np
import torch

from .. import _lib, ragged
from . import box_util, predictions

MAX_THRESHOLDS = 4
LIST_GROUPS = 16384          # (scene, class) groups per launch pair of records_from_lists


def _thresholds(ap_iou_thresh):
    thr = tuple(float(t) for t in np.atleast_1d(np.asarray(ap_iou_thresh, dtype=np.float64)))
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d IoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    return thr


@torch.no_grad()
def parse_groundtruths(gt_data, dataset_config):
    """Ground-truth labels -> {'sem_cls_label' (B,G), 'gt_corners_3d_upright_camera' (B,G,8,3) f64,
    'box_label_mask' (B,G)}, device tensors; rows with box_label_mask == 0 are zero."""
    center = gt_data['center_label'][:, :, 0:3].double()
    angle = box_util.class2angle(gt_data['heading_class_label'], gt_data['heading_residual_label'],
                                 dataset_config.num_heading_bin)
    size = box_util.class2size(gt_data['size_class_label'], gt_data['size_residual_label'], dataset_config.mean_size_arr)
    corners = box_util.box_corners_upright_camera(center, size, angle)
    mask = gt_data['box_label_mask']
    corners = corners * (mask != 0).view(*mask.shape, 1, 1).to(corners.dtype)
    return {'sem_cls_label': gt_data['sem_cls_label'], 'gt_corners_3d_upright_camera': corners,
            'box_label_mask': mask}


def box3d_iou(pred_corners, gt_corners, with_2d=False):
    """(B,K,8,3), (B,G,8,3) f64 device tensors -> iou3d (B,K,G) [, iou2d]: one rfd_box3d_iou launch."""
    pred = pred_corners.double().contiguous()
    gt = gt_corners.double().contiguous()
    B, K = pred.shape[:2]
    G = gt.shape[1]
    iou3d = torch.zeros(B, K, G, dtype=torch.float64, device=pred.device)
    iou2d = torch.zeros_like(iou3d) if with_2d else None
    _lib.call("rfd_box3d_iou", pred.device, B, K, G, pred.data_ptr(), gt.data_ptr(), iou3d.data_ptr(),
              _lib.ptr(iou2d))
    return (iou3d, iou2d) if with_2d else iou3d


def ap_match(iou3d, order, det_valid, gt_cls, gt_valid, thr):
    """One rfd_ap_match launch -> tp (nT,B,C,K) uint8; thr: (nT) f64 device tensor."""
    B, C, K = order.shape
    G = gt_cls.shape[1]
    tp = torch.empty(thr.numel(), B, C, K, dtype=torch.uint8, device=order.device)
    _lib.call("rfd_ap_match", order.device, B, C, K, G, thr.numel(), iou3d.data_ptr(), order.data_ptr(),
              det_valid.data_ptr(), gt_cls.data_ptr(), gt_valid.data_ptr(), thr.data_ptr(), tp.data_ptr())
    return tp


class SceneRecords(object):
    """What one scene_records call leaves for the host: per (scene, class, detection) the score, whether it takes part
    and its true-positive flag per threshold, plus the ground-truth count per (scene, class) -- packed into ONE pinned
    buffer filled by one copy queued on the caller's stream.  The views score (B,C,K) f32, valid (B,C,K) u8,
    tp (nT,B,C,K) u8 and npos (B,C) i32 are meaningful once `event` has passed; compact() waits for it (and for
    nothing else) and returns the records as flat arrays
    {'cls' (n) i32, 'score' (n) f32, 'tp' (nT,n) u8, 'npos' (C) i64, 'thr'}.
    mesh=True: the buffer carries a second flag array behind the first, tp_mesh (nT,B,C,K) u8 -- the same matching on the
    mesh IoU (mesh_eval.py) -- and compact() has the extra key 'tp_mesh' (nT,n)."""

    def __init__(self, thr, shape, buf, event, timing=None, mesh=False):
        B, C, K = shape
        n = B * C * K
        nT = len(thr)
        self.thr, self.buf, self.event = thr, buf, event
        self.score = buf[:4 * n].view(torch.float32).view(B, C, K)
        self.npos = buf[4 * n:4 * n + 4 * B * C].view(torch.int32).view(B, C)
        o = 4 * n + 4 * B * C
        self.valid = buf[o:o + n].view(B, C, K)
        self.tp = buf[o + n:o + n + nT * n].view(nT, B, C, K)
        self.tp_mesh = buf[o + n + nT * n:o + n + 2 * nT * n].view(nT, B, C, K) if mesh else None
        self.timing = timing                    # (start, end) events around the two launches, when asked for
        self._compact = None

    def device_ms(self):
        self.event.synchronize()
        return self.timing[0].elapsed_time(self.timing[1])

    def compact(self):
        if self._compact is None:
            self.event.synchronize()
            valid = self.valid.numpy() != 0
            bi, ci, ki = np.nonzero(valid)
            self._compact = {'cls': ci.astype(np.int32), 'score': self.score.numpy()[bi, ci, ki],
                             'tp': self.tp.numpy()[:, bi, ci, ki], 'npos': self.npos.numpy().sum(0).astype(np.int64),
                             'thr': self.thr}
            if self.tp_mesh is not None:
                self._compact['tp_mesh'] = self.tp_mesh.numpy()[:, bi, ci, ki]
        return self._compact


_thr_cache = _lib.ArtefactCache(64)      # the thresholds as an f64 device tensor, uploaded once per (device, thresholds)


def _records(pred_corners, score, valid, gt_corners, gt_cls, gt_valid, thr, timing=False, mesh_iou=None):
    """score (B,C,K) f32, valid (B,C,K) u8, gt_cls (B,G) i32, gt_valid (B,G) u8 on the device -> SceneRecords.
    Everything is queued on the current stream and the host waits for none of it: an argsort and a few small tensor
    kernels (ground-truth counts, packing), the two launches, and one device-to-host copy into pinned memory."""
    dev = score.device
    B, C, K = score.shape
    stream = torch.cuda.current_stream(dev)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if timing else None
    # the global sort by confidence is the host's; within a (scene, class) only the order matters (stable, so equal
    # scores go by index -- the reference's np.argsort(-confidence) leaves the order of ties undefined)
    order = torch.argsort(score, dim=-1, descending=True, stable=True).int().contiguous()
    thr_d = _thr_cache.get((str(dev), thr), lambda: torch.tensor(thr, dtype=torch.float64, device=dev), dev)
    if ev:
        ev[0].record(stream)
    iou3d = box3d_iou(pred_corners, gt_corners)
    tp = ap_match(iou3d, order, valid, gt_cls, gt_valid, thr_d)
    if ev:
        ev[1].record(stream)
    flags = [tp.flatten()]
    if mesh_iou is not None:                # the same matching -- order, validity, classes, thresholds -- on the mesh IoU
        flags.append(ap_match(mesh_iou, order, valid, gt_cls, gt_valid, thr_d).flatten())
    npos = ((gt_cls.unsqueeze(1) == torch.arange(C, device=dev, dtype=gt_cls.dtype).view(1, C, 1)) &
            (gt_valid.unsqueeze(1) != 0)).sum(-1).int()
    packed = torch.cat([score.contiguous().view(torch.uint8).flatten(), npos.contiguous().view(torch.uint8).flatten(),
                        valid.flatten()] + flags)
    buf = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
    buf.copy_(packed, non_blocking=True)
    done = torch.cuda.Event()
    done.record(stream)
    return SceneRecords(thr, (B, C, K), buf, done, ev, mesh=mesh_iou is not None)


@torch.no_grad()
def scene_records(eval_dict, parsed_predictions, parsed_gts, config=None, ap_iou_thresh=(0.25, 0.5), timing=False,
                  mesh_iou=None):
    """Device tensors in (numpy is uploaded) -> SceneRecords, queued on the current stream; the host does not wait.
    A detection takes part iff pred_mask == 1 and obj_prob > conf_thresh.  per_class_proposal (default): it is scored
    for every class with sem_cls_probs[..., c] * obj_prob (a float32 product); otherwise once, for pred_sem_cls, with
    obj_prob.  config: the eval config (predictions.DEFAULT_EVAL_CONFIG keys).
    mesh_iou: (B,K,G) f64, the mesh IoU of every (proposal, ground truth) pair (mesh_eval.scene_mesh_iou): the records
    also carry 'tp_mesh', the flags of a second rfd_ap_match launch on it (eval_det.py:189-234 keeps the two side by side)."""
    cfg = dict(predictions.DEFAULT_EVAL_CONFIG)
    cfg.update(config or {})
    thr = _thresholds(ap_iou_thresh)
    corners = parsed_predictions['pred_corners_3d_upright_camera']
    dev = corners.device if torch.is_tensor(corners) and corners.is_cuda else torch.device('cuda', torch.cuda.current_device())
    corners = _lib.as_tensor(corners, dev, torch.float64)
    obj_prob = _lib.as_tensor(parsed_predictions['obj_prob'], dev, torch.float32)
    sem = _lib.as_tensor(parsed_predictions['sem_cls_probs'], dev, torch.float32)
    pred_cls = _lib.as_tensor(parsed_predictions['pred_sem_cls'], dev, torch.int64)
    mask = _lib.as_tensor(eval_dict['pred_mask'], dev, torch.int64)
    B, K, C = sem.shape
    take = (mask == 1) & (obj_prob > cfg['conf_thresh'])
    if cfg['per_class_proposal']:
        score = (sem * obj_prob.unsqueeze(-1)).transpose(1, 2).contiguous()
        valid = take.unsqueeze(1).expand(B, C, K)
    else:
        score = obj_prob.unsqueeze(1).expand(B, C, K).contiguous()
        valid = take.unsqueeze(1) & (pred_cls.unsqueeze(1) == torch.arange(C, device=dev).view(1, C, 1))
    gt_corners = _lib.as_tensor(parsed_gts['gt_corners_3d_upright_camera'], dev, torch.float64)
    gt_cls = _lib.as_tensor(parsed_gts['sem_cls_label'], dev, torch.int32).contiguous()
    gt_valid = (_lib.as_tensor(parsed_gts['box_label_mask'], dev, torch.float32) == 1).to(torch.uint8).contiguous()
    if mesh_iou is not None:
        mesh_iou = _lib.as_tensor(mesh_iou, dev, torch.float64).contiguous()
        if tuple(mesh_iou.shape) != (B, K, gt_cls.shape[1]):
            raise ValueError("mesh_iou is %s, the scene has (B,K,G) = %s" % (tuple(mesh_iou.shape), (B, K, gt_cls.shape[1])))
    return _records(corners, score, valid.to(torch.uint8).contiguous(), gt_corners, gt_cls, gt_valid, thr, timing, mesh_iou)


def merge_records(records, thr=None, n_cls=0):
    """A list of records (SceneRecords or compact dicts; one record alone is a list of one) -> one compact dict
    {'cls' (n) i32, 'score' (n) f32, 'tp' (nT,n) u8, 'npos' (C) i64, 'thr'}.  An empty list needs `thr` and gives
    n = 0 with n_cls zero counts.  Records with 'tp_mesh' (nT,n) give a merged 'tp_mesh'; all of them have it or none
    (ValueError)."""
    recs = [r.compact() if isinstance(r, SceneRecords) else r
            for r in (records if isinstance(records, (list, tuple)) else [records])]
    if thr is None:
        if not recs:
            raise ValueError("no records and no thresholds")
        thr = recs[0]['thr']
    thr = tuple(float(t) for t in thr)
    if any(tuple(r['thr']) != thr for r in recs):
        raise ValueError("records were matched at other IoU thresholds than %r" % (thr,))
    npos = np.zeros(max([len(r['npos']) for r in recs] + [n_cls]), np.int64)
    for r in recs:
        npos[:len(r['npos'])] += np.asarray(r['npos'], np.int64)
    cat = lambda parts, empty: np.concatenate(parts, -1) if parts else empty
    with_mesh = [('tp_mesh' in r) for r in recs]
    if any(with_mesh) and not all(with_mesh):
        raise ValueError("records with and without mesh flags ('tp_mesh') cannot be merged")
    out = {'cls': cat([np.asarray(r['cls'], np.int32) for r in recs], np.zeros(0, np.int32)),
            'score': cat([np.asarray(r['score'], np.float32) for r in recs], np.zeros(0, np.float32)),
            'tp': cat([np.asarray(r['tp'], np.uint8).reshape(len(thr), -1) for r in recs], np.zeros((len(thr), 0), np.uint8)),
            'npos': npos, 'thr': thr}
    if any(with_mesh):
        out['tp_mesh'] = np.concatenate([np.asarray(r['tp_mesh'], np.uint8).reshape(len(thr), -1) for r in recs], -1)
    return out


VOC07_RECALL_GRID = np.arange(11) * 0.1


def voc_ap(rec, prec, use_07_metric=True):
    """Average precision of one class from its recall / precision after each detection (by descending score).
    VOC 2007: the mean over the eleven recall levels 0, 0.1, ... 1 of the best precision reached at or beyond that
    recall (0 if it is never reached).  The levels are k * 0.1 in floating point, as the reference's grid is: a recall
    of exactly 3 / 10 does NOT reach the level 0.30000000000000004.
    All points: the area under the precision envelope (at each detection the best precision from there on),
    integrated over the recall steps."""
    rec, prec = np.asarray(rec, np.float64), np.asarray(prec, np.float64)
    if use_07_metric:
        reached = rec[None, :] >= VOC07_RECALL_GRID[:, None]
        return float(np.where(reached, prec[None, :], 0.).max(axis=1, initial=0.).sum() / 11.)
    envelope = np.maximum.accumulate(prec[::-1])[::-1]
    return float(np.sum(np.diff(rec, prepend=0.) * envelope))


class APCalculator(object):
    """ap_helper.py:25-82.  step() takes the records of scene_records (SceneRecords, or their compact() dict -- what
    sharding.gather_records returns) or the reference's two lists; compute_metrics() returns the reference's dict
    ('<cls> Average Precision', 'mAP', '<cls> Recall', 'AR'), or one such dict per threshold when `ap_iou_thresh` is a
    sequence.

    evaluate_mesh=True raises: the reference's mesh mAP voxelises every predicted and ground-truth mesh through the
    external `binvox` program and loads the ShapeNet ground-truth meshes from disk; neither is available to this
    project, so the result could not be checked against anything.
    mesh_eval.MeshAPCalculator computes mesh mAP on this project's own voxel grids instead."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, evaluate_mesh=False):
        if evaluate_mesh:
            raise NotImplementedError(
                "evaluate_mesh=True: mesh mAP needs the external `binvox` voxeliser and the ShapeNet ground-truth "
                "meshes (ap_helper.py:429-478); neither exists here, so it cannot be computed or pinned. "
                "Box mAP (evaluate_mesh=False) is available.")
        self.single = np.ndim(ap_iou_thresh) == 0
        self.ap_iou_thresh = _thresholds(ap_iou_thresh)
        self.class2type_map = class2type_map
        self.evaluate_mesh = False
        self.reset()

    def reset(self):
        self.records = []
        self.scan_cnt = 0

    def step(self, records, batch_gt_map_cls=None):
        if batch_gt_map_cls is not None:
            assert len(records) == len(batch_gt_map_cls)
            self.scan_cnt += len(records)
            records = records_from_lists(records, batch_gt_map_cls, self.ap_iou_thresh)
        elif isinstance(records, SceneRecords):
            self.scan_cnt += records.score.shape[0]
        else:
            self.scan_cnt += 1
        if (records.thr if isinstance(records, SceneRecords) else tuple(records['thr'])) != self.ap_iou_thresh:
            raise ValueError("records were matched at other IoU thresholds than %r" % (self.ap_iou_thresh,))
        self.records.append(records)

    def class_curves(self, ti, use_07_metric=True, flags='tp'):
        """-> {class: (rec, prec, ap)}; a class with ground truths and no prediction: (0, 0, 0) as in the reference.
        flags: the record array the curves are drawn from ('tp', or 'tp_mesh' where the records have it)"""
        merged = merge_records(self.records, self.ap_iou_thresh)
        cls, score, tp, npos = merged['cls'], merged['score'], merged[flags][ti], merged['npos']
        n_cls = len(npos)
        out = {}
        for c in range(n_cls):
            m = cls == c
            if not m.any():
                if npos[c] > 0:
                    out[c] = (0, 0, 0)
                continue
            o = np.argsort(-score[m], kind='stable')
            flags = tp[m][o].astype(np.float64)
            tpc, fpc = np.cumsum(flags), np.cumsum(1. - flags)
            with np.errstate(divide='ignore', invalid='ignore'):
                rec = tpc / float(npos[c])                     # 0 / 0 = NaN without ground truths, as the reference
            prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
            out[c] = (rec, prec, voc_ap(rec, prec, use_07_metric))
        return out

    def compute_metrics(self, use_07_metric=True):
        """use_07_metric=True is what the reference's compute_metrics_wo_mesh runs with (the default of
        eval_det_multiprocessing_wo_mesh); False gives the all-points AP."""
        rets = [self.metrics_of(self.class_curves(ti, use_07_metric)) for ti in range(len(self.ap_iou_thresh))]
        return rets[0] if self.single else rets

    def metrics_of(self, cur, suffix=''):
        """class_curves' result -> the reference's dict; suffix: '_mesh' for the mesh keys (ap_helper.py:108-122)"""
        name = lambda c: self.class2type_map[c] if self.class2type_map else str(c)
        ret = {}
        for c in sorted(cur):
            ret['%s Average Precision%s' % (name(c), suffix)] = cur[c][2]
        ret['mAP' + suffix] = np.mean([cur[c][2] for c in sorted(cur)]) if cur else float('nan')
        rec_list = []
        for c in sorted(cur):
            r = cur[c][0][-1] if np.ndim(cur[c][0]) else 0
            ret['%s Recall%s' % (name(c), suffix)] = r
            rec_list.append(r)
        ret['AR' + suffix] = np.mean(rec_list) if cur else float('nan')
        return ret


def records_from_lists(batch_pred_map_cls, batch_gt_map_cls, ap_iou_thresh):
    """The reference's list format (ap_helper.py:40-54: [[(cls, corners (8,3), score), ...], ...] and
    [[(cls, corners), ...], ...]) through the same two kernels.  Detections and ground truths are grouped by (scene,
    class) -- the unit the matching is independent in -- padded to the largest group and uploaded as one batch of
    single-class scenes; more than 1024 detections or 256 ground truths in one group is the kernel's error."""
    thr = _thresholds(ap_iou_thresh)
    classes = sorted({int(p[0]) for lst in batch_pred_map_cls for p in lst} |
                     {int(g[0]) for lst in batch_gt_map_cls for g in lst})
    n_cls = (classes[-1] + 1) if classes else 0
    assert not classes or classes[0] >= 0, "class ids are non-negative integers"
    npos = np.zeros(n_cls, np.int64)
    groups = {}                                    # (scene, class) -> ([boxes], [scores], [gt boxes])
    for s, (preds, gts) in enumerate(zip(batch_pred_map_cls, batch_gt_map_cls)):
        for g in gts:
            npos[int(g[0])] += 1
            groups.setdefault((s, int(g[0])), ([], [], []))[2].append(np.asarray(g[1], np.float64))
        for p in preds:
            e = groups.setdefault((s, int(p[0])), ([], [], []))
            e[0].append(np.asarray(p[1], np.float64))
            e[1].append(np.float32(p[2]))
    keys = [k for k in sorted(groups) if groups[k][0]]
    if not keys:
        return {'cls': np.zeros(0, np.int32), 'score': np.zeros(0, np.float32),
                'tp': np.zeros((len(thr), 0), np.uint8), 'npos': npos, 'thr': thr}
    Kp = max(len(groups[k][0]) for k in keys)
    Gp = max(max(len(groups[k][2]) for k in keys), 1)
    b = len(keys)
    corners = np.zeros((b, Kp, 8, 3))
    score = np.full((b, 1, Kp), -np.inf, np.float32)
    valid = np.zeros((b, 1, Kp), np.uint8)
    gtc = np.zeros((b, Gp, 8, 3))
    gt_valid = np.zeros((b, Gp), np.uint8)
    for i, k in enumerate(keys):
        boxes, sc, gts = groups[k]
        corners[i, :len(boxes)] = np.stack(boxes)
        score[i, 0, :len(sc)] = sc
        valid[i, 0, :len(sc)] = 1
        if gts:
            gtc[i, :len(gts)] = np.stack(gts)
            gt_valid[i, :len(gts)] = 1
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev)
    # a whole sweep can hold more groups than one launch takes scenes (65535): a launch pair per LIST_GROUPS groups
    parts = [_records(up(corners[i:i + LIST_GROUPS]), up(score[i:i + LIST_GROUPS]), up(valid[i:i + LIST_GROUPS]),
                      up(gtc[i:i + LIST_GROUPS]), torch.zeros(min(LIST_GROUPS, b - i), Gp, dtype=torch.int32, device=dev),
                      up(gt_valid[i:i + LIST_GROUPS]), thr) for i in range(0, b, LIST_GROUPS)]
    rec = merge_records(parts, thr)
    # compact() walks the (group, detection) pairs in row-major order: the class of a record is its group's (the owner
    # map of DESIGN.md "Ragged batches")
    counts = valid[:, 0].sum(1, dtype=np.int64)
    cls = np.array([k[1] for k in keys], np.int32)[ragged.owners(counts)]
    return {'cls': cls, 'score': rec['score'], 'tp': rec['tp'], 'npos': npos, 'thr': thr}


# ---- completion half of the test output (network.py:126-150, :387-471) ------------------------------------------------
FAR_AWAY = 1.0e18        # where a masked-out ground-truth centroid is moved: squared distances stay finite in fp32


@torch.no_grad()
def proposal_to_gt(end_points, data, ids):
    """The reference's BATCH_PROPOSAL_IDs (network.py:404-413, :433): ids (B,K',1) proposal ids -> (B,K',3) int64 rows
    (proposal id, ground-truth box id, ground-truth class).  A proposal goes to the nearest ground-truth centroid among
    the rows with box_label_mask set (nn_distance over the compacted centroids in the reference; here the Chamfer
    nearest-neighbour kernel over all rows with the masked ones moved out of reach, so nothing waits for the host); a
    tie goes to the lowest index.  A scene without any ground-truth box maps everything to row 0."""
    from ..chamfer_distance import nearest
    centers = end_points['center']
    dev = centers.device
    mask = data['box_label_mask'].to(dev) != 0
    gt = data['center_label'].to(dev)[:, :, 0:3].float()
    gt = torch.where(mask.unsqueeze(-1), gt, torch.full_like(gt, FAR_AWAY))
    _, idx1, _, _ = nearest(centers, gt)
    pid = ids[..., 0].long()
    box = torch.gather(idx1.long(), 1, pid)
    cls = torch.gather(data['sem_cls_label'].to(dev).long(), 1, box)
    return torch.stack([pid, box, cls], dim=-1)


@torch.no_grad()
def prepare_data(data, proposal_ids):
    """network.py:438-458: the ground-truth occupancy samples of every selected proposal's box:
    data['object_points'] (B,G,T,3), data['object_points_occ'] (B,G,T), proposal_ids (B,K',3) ->
    points (B*K',T,3), occupancies (B*K',T)."""
    pts, occ = data['object_points'], data['object_points_occ']
    B, G, T, D = pts.shape
    Kp = proposal_ids.shape[1]
    box = proposal_ids[:, :, 1].to(pts.device)
    p = torch.gather(pts, 1, box.view(B, Kp, 1, 1).expand(B, Kp, T, D)).view(B * Kp, T, D)
    o = torch.gather(occ, 1, box.view(B, Kp, 1).expand(B, Kp, T)).view(B * Kp, T)
    return p, o


@torch.no_grad()
def voxel_iou(logits, logit_threshold, gt_voxels, return_counts=False):
    """compute_iou (net_utils/libs.py) of the predicted voxels `logits >= logit_threshold` against `gt_voxels >= 0.5`:
    logits (K,V) or (K,n,n,n) f32, gt_voxels the same shape (any dtype) -> iou (K,) f32 on the device =
    inter.float() / union.float() from one rfd_voxel_iou launch; NaN for an empty pair, as numpy's 0 / 0."""
    _lib.need_gpu(logits)
    K = logits.shape[0]
    logits, ld = _lib.rows(logits.reshape(K, -1).float())
    V = logits.shape[1]
    gt = gt_voxels.to(logits.device).reshape(K, -1).float().contiguous()
    assert gt.shape == (K, V)
    inter = torch.empty(K, dtype=torch.int32, device=logits.device)
    union = torch.empty(K, dtype=torch.int32, device=logits.device)
    _lib.call("rfd_voxel_iou", logits.device, K, V, logits.data_ptr(), ld,
              float(logit_threshold), gt.data_ptr(), inter.data_ptr(), union.data_ptr())
    iou = inter.float() / union.float()
    return (iou, inter, union) if return_counts else iou
