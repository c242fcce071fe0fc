"""float64 numpy restatement of the reference's detection loss (models/loss.py:41-271 on net_utils/nn_distance.py) and of
PointSeg's mask loss (pointseg.py:132-139, 168-177; skip_propagation.py:100-113): the yardstick of tests/test_gpu_loss.py
on shapes the fixture F_LOSS does not hold, and itself checked against the fixture's float64 run of the reference
(tests/test_loss_cpu.py).

It restates that float64 RUN, operation for operation.  The reference creates some tensors as fp32 whatever the inputs
are -- objectness_mask, objectness_label.float(), seed_gt_votes_mask.float(), mean_size_arr, the objectness weights --
so their sums, the `sum + 1e-6` denominators built on them and the three statistics pos_ratio / neg_ratio / obj_acc are
fp32 operations in that run too, and are fp32 here."""


def threshold_margin(est, gt):
    """smallest distance of sqrt(dist1 + 1e-6) to 0.3 or 0.6 over the proposals"""
    d = ((est['aggregated_vote_xyz'][:, :, None].astype(np.float64) - gt['center_label'][:, None, :, :3]) ** 2).sum(-1)
    e = np.sqrt(d.min(2) + 1e-6)
    return min(np.abs(e - NEAR_THRESHOLD).min(), np.abs(e - FAR_THRESHOLD).min())
import numpy as np

NEAR_THRESHOLD, FAR_THRESHOLD, GT_VOTE_FACTOR = 0.3, 0.6, 3
f32, f64 = np.float32, np.float64
OBJECTNESS_CLS_WEIGHTS = np.array([0.2, 0.8], f32).astype(f64)          # torch.Tensor([0.2, 0.8]): an fp32 tensor


def _den32(count):
    """torch.sum(<fp32 0/1 tensor>) + 1e-6, an fp32 operation"""
    return f64(f32(count) + f32(1e-6))


def huber(e, delta=1.0):
    a = np.abs(e)
    q = np.minimum(a, delta)
    return 0.5 * q ** 2 + delta * (a - q)


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def nn_distance(a, b, l1=False):
    """a (B,N,3), b (B,M,3) -> dist1 (B,N), idx1, dist2 (B,M), idx2; argmin takes the first minimum, as torch.min"""
    d = a[:, :, None, :] - b[:, None, :, :]
    d = np.abs(d).sum(-1) if l1 else (d ** 2).sum(-1)
    return d.min(2), d.argmin(2), d.min(1), d.argmin(1)


def vote_loss(est, gt):
    seed_xyz = est['seed_xyz'].astype(f64)
    B, S = seed_xyz.shape[:2]
    inds = est['seed_inds'].astype(np.int64)
    mask = np.take_along_axis(gt['vote_label_mask'], inds, 1).astype(f64)
    votes = np.take_along_axis(gt['vote_label'].astype(f64), inds[:, :, None], 1) + np.tile(seed_xyz, (1, 1, 3))
    pred = est['vote_xyz'].astype(f64).reshape(B * S, -1, 3)
    _, _, dist2, _ = nn_distance(pred, votes.reshape(B * S, GT_VOTE_FACTOR, 3), l1=True)
    votes_dist = dist2.min(1).reshape(B, S)
    return (votes_dist * mask).sum() / _den32(mask.sum())


def objectness_loss(est, gt):
    """-> loss, objectness_label (B,K) int64, objectness_mask (B,K) f32, object_assignment (B,K) int64"""
    agg = est['aggregated_vote_xyz'].astype(f64)
    center = gt['center_label'][:, :, :3].astype(f64)
    dist1, ind1, _, _ = nn_distance(agg, center)
    e = np.sqrt(dist1 + 1e-6)
    label = (e < NEAR_THRESHOLD).astype(np.int64)
    mask = ((e < NEAR_THRESHOLD) | (e > FAR_THRESHOLD)).astype(f32)
    logp = log_softmax(est['objectness_scores'].astype(f64))
    ce = -OBJECTNESS_CLS_WEIGHTS[label] * np.take_along_axis(logp, label[..., None], 2)[..., 0]
    loss = (ce * mask).sum() / _den32(mask.sum())
    return loss, label, mask, ind1


def distinct_gap(points, rows):
    """per point: second-smallest minus smallest DISTINCT squared distance to the rows (inf with one distinct value)"""
    d = ((points[:, :, None, :].astype(f64) - rows[:, None, :, :3].astype(f64)) ** 2).sum(-1)
    out = np.full(d.shape[:2], np.inf)
    for b in range(d.shape[0]):
        for k in range(d.shape[1]):
            u = np.unique(d[b, k])
            if u.size > 1:
                out[b, k] = u[1] - u[0]
    return out


def box_and_sem_cls_loss(est, gt, label, assignment, mean_size_arr, num_heading_bin):
    center = est['center'].astype(f64)
    dist1, _, dist2, _ = nn_distance(center, gt['center_label'][:, :, :3].astype(f64))
    blm = gt['box_label_mask'].astype(f64)
    lab = label.astype(f64)
    den = _den32(lab.sum())
    center_loss = (dist1 * lab).sum() / den + (dist2 * blm).sum() / (blm.sum() + 1e-6)

    def at(name):
        return np.take_along_axis(gt[name], assignment, 1)

    def ce(scores, cls):
        return -np.take_along_axis(log_softmax(est[scores].astype(f64)), cls[..., None], 2)[..., 0]
    hcls = at('heading_class_label')
    heading_cls = (ce('heading_scores', hcls) * lab).sum() / den
    hres = at('heading_residual_label').astype(f64) / (np.pi / num_heading_bin)
    hpred = np.take_along_axis(est['heading_residuals_normalized'].astype(f64), hcls[..., None], 2)[..., 0]
    heading_reg = (huber(hpred - hres) * lab).sum() / den
    scls = at('size_class_label')
    size_cls = (ce('size_scores', scls) * lab).sum() / den
    sres = np.take_along_axis(gt['size_residual_label'].astype(f64), assignment[..., None].repeat(3, 2), 1)
    spred = np.take_along_axis(est['size_residuals_normalized'].astype(f64), scls[..., None, None].repeat(3, 3), 2)[:, :, 0]
    mean = np.asarray(mean_size_arr).astype(f32).astype(f64)[scls]
    size_reg = (huber(spred - sres / mean).mean(-1) * lab).sum() / den
    sem = (ce('sem_cls_scores', at('sem_cls_label')) * lab).sum() / den
    return center_loss, heading_cls, heading_reg, size_cls, size_reg, sem


def ratios_f32(label, mask, objectness_scores):
    """pos_ratio, neg_ratio, obj_acc: the reference's fp32 operations on the counts"""
    total = f32(label.size)
    pos = f32(label.sum()) / total
    neg = f32(mask.sum()) / total - pos
    pred = np.argmax(objectness_scores, 2)
    acc = f32(((pred == label).astype(f32) * mask).sum()) / (f32(mask.sum()) + f32(1e-6))
    return pos, neg, acc


def detection_loss(est, gt, mean_size_arr, num_heading_bin=12):
    """-> (the thirteen-key dictionary, objectness_label, objectness_mask, object_assignment)"""
    vote = vote_loss(est, gt)
    obj, label, mask, assignment = objectness_loss(est, gt)
    center, hcls, hreg, scls, sreg, sem = box_and_sem_cls_loss(est, gt, label, assignment, mean_size_arr, num_heading_bin)
    box = center + 0.1 * hcls + hreg + 0.1 * scls + sreg
    total = vote + 0.5 * obj + box + 0.1 * sem
    total *= 10
    pos, neg, acc = ratios_f32(label, mask, est['objectness_scores'])
    out = {'total': total, 'vote_loss': vote, 'objectness_loss': obj, 'box_loss': box, 'sem_cls_loss': sem,
           'pos_ratio': pos, 'neg_ratio': neg, 'center_loss': center, 'heading_cls_loss': hcls, 'heading_reg_loss': hreg,
           'size_cls_loss': scls, 'size_reg_loss': sreg, 'obj_acc': acc}
    return out, label, mask, assignment


def mask_loss(logp, grouped_labels, proposal_labels, trans_feat, scale=0.001):
    """logp (Kp,P,2), grouped_labels (Kp,P), proposal_labels (Kp,), trans_feat (Kp,64,64) -> the scalar loss"""
    target = (grouped_labels == np.asarray(proposal_labels)[:, None]).astype(np.int64)
    nll = -np.take_along_axis(logp.astype(f64), target[..., None], 2).mean()
    T = trans_feat.astype(f64)
    prod = T @ (T.transpose(0, 2, 1) - np.eye(T.shape[1])[None])
    return nll + scale * np.sqrt((prod ** 2).sum((1, 2))).mean()
