"""Cost of the test mode's losses on one GPU: DetectionLoss (three launches of csrc/det_loss.hip and one copy), PointSeg's
mask loss (two launches), and the same functions written as plain fp32 torch ops on the same device -- a comparison, not
a test.  Headline shape: B = 1, S = 1024 seeds, K = 256 proposals, G = 64 label rows; mask loss at K' = 13 and 256
proposals of P = 1024 points.

    python tools/loss_cost.py [--out profiles/test_mode_loss.json] [--reps 50]

Each figure is device milliseconds per call (HIP events around `reps` calls in a row after a warm-up, the median of five
such windows), with the number of launches through the library's C ABI beside it, or for the torch composition the number
of aten operators it dispatches (counted with a TorchDispatchMode; most of them are one kernel).  The DetectionLoss figure
includes its one device-to-host copy, as the torch figure includes the reference's twelve `.item()` reads."""
import argparse
import json
import os

import numpy as np
import torch

from cost_common import ROOT, device_ms


def nearest(a, b, l1=False):
    d = a.unsqueeze(2) - b.unsqueeze(1)
    d = d.abs().sum(-1) if l1 else d.pow(2).sum(-1)
    d1, i1 = d.min(2)
    return d1, i1, d.min(1)[0]


def torch_detection_loss(est, gt, mean_size, nhb):
    """the thirteen keys with torch ops, in the reference's steps (gathers, one-hot products, CrossEntropyLoss)"""
    from rfdnet_amd.iscnet.loss import huber_loss
    ce = torch.nn.functional.cross_entropy
    B, S = est['seed_xyz'].shape[:2]
    inds = est['seed_inds'].long()
    vmask = torch.gather(gt['vote_label_mask'], 1, inds).float()
    votes = torch.gather(gt['vote_label'], 1, inds.unsqueeze(-1).expand(-1, -1, 9)) + est['seed_xyz'].repeat(1, 1, 3)
    _, _, d2 = nearest(est['vote_xyz'].view(B * S, -1, 3), votes.view(B * S, 3, 3), l1=True)
    vote = (d2.min(1)[0].view(B, S) * vmask).sum() / (vmask.sum() + 1e-6)
    centers = gt['center_label'][:, :, :3]
    d1, assign, _ = nearest(est['aggregated_vote_xyz'], centers)
    e = torch.sqrt(d1 + 1e-6)
    label = (e < 0.3).long()
    mask = ((e < 0.3) | (e > 0.6)).float()
    w = torch.tensor([0.2, 0.8], device=e.device)
    obj = (ce(est['objectness_scores'].transpose(2, 1), label, w, reduction='none') * mask).sum() / (mask.sum() + 1e-6)
    lab = label.float()
    den = lab.sum() + 1e-6
    c1, _, c2 = nearest(est['center'], centers)
    center = (c1 * lab).sum() / den + (c2 * gt['box_label_mask']).sum() / (gt['box_label_mask'].sum() + 1e-6)
    hc = torch.gather(gt['heading_class_label'], 1, assign)
    hcls = (ce(est['heading_scores'].transpose(2, 1), hc, reduction='none') * lab).sum() / den
    hres = torch.gather(gt['heading_residual_label'], 1, assign) / (np.pi / nhb)
    hot = torch.nn.functional.one_hot(hc, nhb).float()
    hreg = (huber_loss((est['heading_residuals_normalized'] * hot).sum(-1) - hres) * lab).sum() / den
    sc = torch.gather(gt['size_class_label'], 1, assign)
    scls = (ce(est['size_scores'].transpose(2, 1), sc, reduction='none') * lab).sum() / den
    sres = torch.gather(gt['size_residual_label'], 1, assign.unsqueeze(-1).expand(-1, -1, 3))
    hot = torch.nn.functional.one_hot(sc, mean_size.shape[0]).float().unsqueeze(-1)
    pred = (est['size_residuals_normalized'] * hot).sum(2)
    sreg = (huber_loss(pred - sres / (hot * mean_size[None, None]).sum(2)).mean(-1) * lab).sum() / den
    sem = (ce(est['sem_cls_scores'].transpose(2, 1), torch.gather(gt['sem_cls_label'], 1, assign), reduction='none')
           * lab).sum() / den
    box = center + 0.1 * hcls + hreg + 0.1 * scls + sreg
    total = 10 * (vote + 0.5 * obj + box + 0.1 * sem)
    n = float(label.numel())
    pos = lab.sum() / n
    neg = mask.sum() / n - pos
    acc = ((est['objectness_scores'].argmax(2) == label).float() * mask).sum() / (mask.sum() + 1e-6)
    out = {'total': total}
    for k, v in (('vote_loss', vote), ('objectness_loss', obj), ('box_loss', box), ('sem_cls_loss', sem), ('pos_ratio', pos),
                 ('neg_ratio', neg), ('center_loss', center), ('heading_cls_loss', hcls), ('heading_reg_loss', hreg),
                 ('size_cls_loss', scls), ('size_reg_loss', sreg), ('obj_acc', acc)):
        out[k] = v.item()
    return out


def torch_mask_loss(logp, grouped, wanted, trans):
    from rfdnet_amd.iscnet.pointseg import feature_transform_reguliarzer
    target = (grouped == wanted.unsqueeze(-1)).view(-1).long()
    return torch.nn.functional.nll_loss(logp.view(-1, 2), target) + 0.001 * feature_transform_reguliarzer(trans)


def aten_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))
    with Count():
        fn()
    return Count.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "test_mode_loss.json"))
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from rfdnet_amd import _lib, synthetic
    from rfdnet_amd.iscnet import loss, pointseg
    from rfdnet_amd.iscnet.config import Config
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda")
    cfg = Config(mean_size_arr=np.random.default_rng(0).uniform(0.4, 1.5, (8, 3))).dataset_config
    calls = []
    call = _lib.call
    _lib.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
    rng = np.random.default_rng(1)
    B, N, S, K, G = 1, 4096, 1024, 256, 64
    pc, boxes, cls = synthetic.synthetic_scene(seed=3, n_raw=5000, n_points=N, return_boxes=True)
    gt = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.scene_labels(pc, boxes, cls, G=G,
                                                                         mean_size_arr=cfg.mean_size_arr).items()}
    f = lambda *shape: torch.from_numpy(rng.normal(0, 1.5, shape).astype(np.float32)).to(dev)     # noqa: E731
    inds = torch.from_numpy(rng.permutation(N)[:S].astype(np.int32)[None]).to(dev)
    seed_xyz = torch.from_numpy(pc[None, :, :3]).to(dev)[:, inds[0].long()].contiguous()
    agg = torch.from_numpy((boxes[rng.integers(0, 12, K), :3] + rng.normal(0, 0.25, (K, 3))).astype(np.float32)[None]).to(dev)
    est = {'seed_xyz': seed_xyz, 'seed_inds': inds, 'vote_xyz': seed_xyz + 0.3 * f(B, S, 3), 'aggregated_vote_xyz': agg,
           'center': agg + 0.05 * f(B, K, 3), 'objectness_scores': f(B, K, 2), 'heading_scores': f(B, K, 12),
           'heading_residuals_normalized': f(B, K, 12), 'size_scores': f(B, K, 8),
           'size_residuals_normalized': f(B, K, 8, 3), 'sem_cls_scores': f(B, K, 8)}
    mean_size = torch.from_numpy(cfg.mean_size_arr.astype(np.float32)).to(dev)
    det = loss.DetectionLoss()
    with torch.no_grad():
        mine, ref = det(est, gt, cfg), torch_detection_loss(est, gt, mean_size, 12)
        diff = max(abs(float(mine[k]) - float(ref[k])) for k in mine)
        del calls[:]
        det(est, gt, cfg)
        n_det = len(calls)
        rows = [{"what": "DetectionLoss", "B": B, "S": S, "K": K, "G": G, "max_abs_diff_vs_torch": diff,
                 "library": dict(zip(("ms", "ms_min", "ms_max"), device_ms(lambda: det(est, gt, cfg), args.reps)),
                                 abi_launches=n_det, host_copies=1),
                 "torch_ops": dict(zip(("ms", "ms_min", "ms_max"), device_ms(
                     lambda: torch_detection_loss(est, gt, mean_size, 12), args.reps)),
                     aten_ops=aten_ops(lambda: torch_detection_loss(est, gt, mean_size, 12)), host_copies=12)}]
        for Kp in (13, 256):
            P = 1024
            logp = torch.log_softmax(f(Kp, P, 2), -1)
            grouped = torch.from_numpy(rng.integers(0, 13, (Kp, P)).astype(np.float32)).to(dev)
            wanted = torch.from_numpy(rng.integers(0, 13, Kp)).to(dev)
            trans = torch.eye(64, device=dev)[None] + 0.1 * f(Kp, 64, 64) / 1.5
            a, b = pointseg.mask_loss_rows(logp, grouped, wanted, trans), torch_mask_loss(logp, grouped, wanted, trans)
            del calls[:]
            pointseg.mask_loss_rows(logp, grouped, wanted, trans)
            n_mask = len(calls)
            rows.append({"what": "mask loss", "K'": Kp, "P": P, "max_abs_diff_vs_torch": abs(float(a) - float(b)),
                         "library": dict(zip(("ms", "ms_min", "ms_max"), device_ms(
                             lambda: pointseg.mask_loss_rows(logp, grouped, wanted, trans), args.reps)),
                             abi_launches=n_mask),
                         "torch_ops": dict(zip(("ms", "ms_min", "ms_max"), device_ms(
                             lambda: torch_mask_loss(logp, grouped, wanted, trans), args.reps)),
                             aten_ops=aten_ops(lambda: torch_mask_loss(logp, grouped, wanted, trans)))})
    line = {"tool": "loss_cost", "device": torch.cuda.get_device_name(0), "reps_per_window": args.reps, "windows": 5,
            "rows": rows}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
