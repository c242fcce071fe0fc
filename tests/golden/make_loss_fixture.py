"""Generate tests/golden/F_LOSS.npz (DEV CONTAINER ONLY): the reference's DetectionLoss (models/loss.py:205-271, torch CPU)
and PointSeg's get_loss (models/iscnet/modules/pointseg.py:132-177) on seeded inputs, in fp32 and in float64.

Same recipe as make_latent_fixture.py: the reference's modules are imported where they lie.  models.loss is written for
a GPU; four stubs let it load on a CPU: Tensor.cuda = identity, torch.cuda.FloatTensor = torch.FloatTensor, a namespace
module for the Chamfer extension, and a LOSSES registry.  For the float64 run every floating-point input and
objectness_criterion.weight are cast; what the reference itself creates as fp32 (objectness_mask, the .float() casts,
mean_size_arr) stays fp32, as tests/loss_f64.py restates.

Detection case: B = 2, N = 1000 points, S = 200 seeds, K = 96 proposals, G = 16 label rows, vote_factor 1 and 3.
  scene 0: six valid rows; proposals in the near zone (< 0.3 of a row), the grey zone and the far zone; proposal 0 lies
           within 0.3 of the origin, so a zero-padded row (the first one, row 6) wins it and it is a positive; the
           Huber arguments fall on both sides of 1;
  scene 1: box_label_mask all zero, every row padded, no proposal within 0.3 of the origin: denominators 0 + 1e-6.
Mask case: Kp = 5 proposals of P = 130 points, one proposal whose label no point carries, trans_feat = I + 0.1 noise.

Per vote_factor the file holds the reference's fp32 dictionary (`ref32_vf*`), the float64 one (`ref64_vf*`) and
`ref32_dev_vf*` = |fp32 - float64| per key, in the order of `keys`: the unit of the device tests' bounds.

Usage:  python tests/golden/make_loss_fixture.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
from make_fixtures import mount_reference, ns  # noqa: E402

SEED = 77
B, N, S, K, G, NH, NS, NC = 2, 1000, 200, 96, 16, 12, 8, 8
KP, P = 5, 130
KEYS = ('total', 'vote_loss', 'objectness_loss', 'box_loss', 'sem_cls_loss', 'pos_ratio', 'neg_ratio', 'center_loss',
        'heading_cls_loss', 'heading_reg_loss', 'size_cls_loss', 'size_reg_loss', 'obj_acc')


def directions(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def detection_inputs(rng):
    f = np.float32
    centers = np.array([[2.0, 1.5, 0.4], [-2.2, 1.8, 0.6], [2.4, -2.0, 0.5], [-1.8, -2.4, 0.3], [0.3, 2.9, 0.8],
                        [-0.2, -3.1, 0.7]])
    gt = {'center_label': np.zeros((B, G, 3), f), 'heading_class_label': np.zeros((B, G), np.int64),
          'heading_residual_label': np.zeros((B, G), f), 'size_class_label': np.zeros((B, G), np.int64),
          'size_residual_label': np.zeros((B, G, 3), f), 'sem_cls_label': np.zeros((B, G), np.int64),
          'box_label_mask': np.zeros((B, G), f)}
    gt['center_label'][0, :6] = centers
    gt['heading_class_label'][0, :6] = rng.integers(0, NH, 6)
    gt['heading_residual_label'][0, :6] = rng.uniform(-np.pi / NH, np.pi / NH, 6)
    gt['size_class_label'][0, :6] = rng.integers(0, NS, 6)
    gt['size_residual_label'][0, :6] = rng.normal(0, 0.3, (6, 3))
    gt['sem_cls_label'][0, :6] = rng.integers(0, NC, 6)
    gt['box_label_mask'][0, :6] = 1
    agg = np.zeros((B, K, 3))
    # scene 0: proposal 0 next to the origin (a padded row wins), 35 near, 24 grey, 36 far
    agg[0, 0] = [0.06, -0.05, 0.04]
    row = rng.integers(0, 6, K)
    radius = np.concatenate([[0], rng.uniform(0.02, 0.26, 35), rng.uniform(0.34, 0.56, 24), rng.uniform(0.75, 0.95, 36)])
    agg[0, 1:] = (centers[row] + radius[:, None] * directions(rng, K))[1:]
    # scene 1: every row is padded (the origin); grey and far only
    radius = np.concatenate([rng.uniform(0.34, 0.56, 30), rng.uniform(0.7, 3.0, K - 30)])
    agg[1] = radius[:, None] * directions(rng, K)
    est = {'aggregated_vote_xyz': agg.astype(f)}
    est['center'] = (agg + rng.normal(0, 0.08, agg.shape)).astype(f)
    est['objectness_scores'] = rng.normal(0, 2, (B, K, 2)).astype(f)
    est['heading_scores'] = rng.normal(0, 2, (B, K, NH)).astype(f)
    est['heading_residuals_normalized'] = rng.normal(0, 1.2, (B, K, NH)).astype(f)
    est['size_scores'] = rng.normal(0, 2, (B, K, NS)).astype(f)
    est['size_residuals_normalized'] = rng.normal(0, 1.2, (B, K, NS, 3)).astype(f)
    est['sem_cls_scores'] = rng.normal(0, 2, (B, K, NC)).astype(f)
    # seeds and votes
    points = rng.uniform(-3, 3, (B, N, 3))
    gt['vote_label_mask'] = (rng.random((B, N)) < 0.4).astype(np.int64)
    gt['vote_label'] = (rng.normal(0, 0.5, (B, N, 9)) * gt['vote_label_mask'][..., None]).astype(f)
    inds = np.stack([rng.permutation(N)[:S] for _ in range(B)]).astype(np.int32)
    est['seed_inds'] = inds
    est['seed_xyz'] = np.take_along_axis(points, inds.astype(np.int64)[..., None], 1).astype(f)
    true_vote = est['seed_xyz'].astype(np.float64)[:, :, None, :] + \
        np.take_along_axis(gt['vote_label'], inds.astype(np.int64)[..., None], 1).reshape(B, S, 3, 3)
    votes = {1: (true_vote[:, :, 1] + rng.normal(0, 0.2, (B, S, 3))).astype(f),
             3: (true_vote[:, :, ::-1] + rng.normal(0, 0.2, (B, S, 3, 3))).reshape(B, 3 * S, 3).astype(f)}
    return est, gt, votes, rng.uniform(0.4, 1.5, (NS, 3))


def main():
    import torch
    from loss_f64 import detection_loss, distinct_gap, mask_loss, threshold_margin
    mount_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor
    ns('external.pyTorchChamferDistance')
    ns('external.pyTorchChamferDistance.chamfer_distance').ChamferDistance = lambda: None
    reg = importlib.import_module('net_utils.registry')
    ns('models.registers').LOSSES = reg.Registry('loss')
    ref = importlib.import_module('models.loss')
    seg = importlib.import_module('models.iscnet.modules.pointseg')

    rng = np.random.default_rng(SEED)
    est, gt, votes, mean_size = detection_inputs(rng)
    config = types.SimpleNamespace(num_heading_bin=NH, num_size_cluster=NS, num_class=NC, mean_size_arr=mean_size)
    out = {"seed": SEED, "keys": np.array(KEYS), "mean_size_arr": mean_size}
    out.update({"est_" + k: v for k, v in est.items()})
    out.update({"gt_" + k: v for k, v in gt.items()})

    # ---- the conditions under which the discrete outputs are the reference's alone to decide
    _, label64, mask64, assign64 = detection_loss(dict(est, vote_xyz=votes[1]), gt, mean_size, NH)[0:4]
    assert threshold_margin(est, gt) > 1e-4
    assert distinct_gap(est['aggregated_vote_xyz'], gt['center_label']).min() > 1e-5
    assert distinct_gap(est['center'], gt['center_label']).min() > 1e-5
    assert (est['objectness_scores'][..., 0] != est['objectness_scores'][..., 1]).all()
    assert label64[0, 0] == 1 and assign64[0, 0] == 6                       # the padded row wins and is a positive
    grey = 1 - mask64
    assert label64[0].sum() >= 30 and grey[0].sum() >= 20 and (mask64[0] - label64[0]).sum() >= 30
    assert label64[1].sum() == 0 and grey[1].sum() >= 20 and gt['box_label_mask'][1].sum() == 0

    def run(vote_xyz, double):
        cast = (lambda a: torch.from_numpy(a).double() if a.dtype == np.float32 else torch.from_numpy(a)) if double \
            else torch.from_numpy
        e_t = {k: cast(v) for k, v in est.items()}
        e_t['vote_xyz'] = cast(vote_xyz)
        g_t = {k: cast(v) for k, v in gt.items()}
        w = ref.objectness_criterion.weight
        ref.objectness_criterion.weight = w.double() if double else w.float()
        with torch.no_grad():
            d = ref.DetectionLoss()(e_t, g_t, config)
            _, label, mask, assign = ref.compute_objectness_loss(e_t, g_t)
        d['total'] = d['total'].item()
        return d, label.numpy(), mask.numpy(), assign.numpy()

    for vf in (1, 3):
        out["vote_xyz_vf%d" % vf] = votes[vf]
        d32, label, mask, assign = run(votes[vf], False)
        d64, label2, mask2, assign2 = run(votes[vf], True)
        assert np.array_equal(label, label2) and np.array_equal(mask, mask2) and np.array_equal(assign, assign2)
        assert np.array_equal(label, label64) and np.array_equal(assign, assign64)
        v32 = np.array([d32[k] for k in KEYS], np.float64)
        v64 = np.array([d64[k] for k in KEYS], np.float64)
        mine = detection_loss(dict(est, vote_xyz=votes[vf]), gt, mean_size, NH)[0]
        print("vote_factor %d" % vf)
        for i, k in enumerate(KEYS):
            print("  %-18s f64 %.12g  fp32 dev %.2e (rel %.1e)  restatement dev %.1e"
                  % (k, v64[i], abs(v32[i] - v64[i]), abs(v32[i] - v64[i]) / max(abs(v64[i]), 1e-300), abs(mine[k] - v64[i])))
        out["ref32_vf%d" % vf], out["ref64_vf%d" % vf], out["ref32_dev_vf%d" % vf] = v32, v64, np.abs(v32 - v64)
        out["objectness_label"], out["objectness_mask"], out["object_assignment"] = label, mask, assign
    # Huber arguments on both sides of 1 among the positives
    hcls = np.take_along_axis(gt['heading_class_label'], assign64, 1)
    arg = np.take_along_axis(est['heading_residuals_normalized'], hcls[..., None], 2)[..., 0] - \
        np.take_along_axis(gt['heading_residual_label'], assign64, 1) / (np.pi / NH)
    pos = label64 == 1
    assert (np.abs(arg[pos]) > 1).sum() >= 5 and (np.abs(arg[pos]) < 1).sum() >= 5

    # ---- mask case
    logits = rng.normal(0, 2, (KP, P, 2))
    logp = torch.log_softmax(torch.from_numpy(logits.astype(np.float32)), -1)
    grouped = rng.integers(0, 5, (KP, P)).astype(np.float32)
    wanted = np.array([1, 2, 3, 9, 0], np.int64)                              # no point carries label 9
    trans = (np.eye(64)[None] + 0.1 * rng.normal(0, 1, (KP, 64, 64))).astype(np.float32)
    target = torch.from_numpy((grouped == wanted[:, None]).reshape(-1)).long()
    assert target.view(KP, P)[3].sum() == 0 and all(target.view(KP, P)[k].sum() > 0 for k in (0, 1, 2, 4))
    with torch.no_grad():
        m32 = seg.get_loss()(logp.view(-1, 2), target, torch.from_numpy(trans), weight=None).item()
        m64 = seg.get_loss()(logp.double().view(-1, 2), target, torch.from_numpy(trans).double(), weight=None).item()
    mine = mask_loss(logp.numpy(), grouped, wanted, trans)
    print("mask loss f64 %.12g fp32 dev %.2e restatement dev %.1e" % (m64, abs(m32 - m64), abs(mine - m64)))
    out.update(mask_logp=logp.numpy(), mask_grouped=grouped, mask_wanted=wanted, mask_trans=trans,
               mask_ref32=np.float64(m32), mask_ref64=np.float64(m64), mask_ref32_dev=np.float64(abs(m32 - m64)))
    path = os.path.join(HERE, "F_LOSS.npz")
    np.savez_compressed(path, **out)
    print("F_LOSS.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    assert mf.REF
    main()
