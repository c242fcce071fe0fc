"""GPU: the losses of the test mode (csrc/det_loss.hip, include/rfd_loss.h) -- DetectionLoss and PointSeg's mask loss
against float64 (the fixture F_LOSS's float64 run of the reference; tests/loss_f64.py on ragged shapes), their launch
budgets and bit-wise repeatability, SkipPropagation.forward against generate(), and ISCNet.evaluate(losses=True).

Bounds.  A loss key is a mean of non-negative fp32 terms, each the result of at most 64 rounded operations, summed in
f64: |device - f64| <= 64 * 2^-24 * |value|; on the fixture also 8 x `ref32_dev`, the reference fp32 run's own deviation
from float64 on that key, if that is larger.  pos_ratio, neg_ratio, obj_acc and the three per-proposal arrays are exact:
the inputs keep sqrt(dist1 + 1e-6) away from 0.3 / 0.6 and the nearest label row unambiguous (asserted here for the
ragged shapes, by the generator for the fixture)."""
import os

import numpy as np
import pytest
import torch

from rfdnet_amd import synthetic
from rfdnet_amd.iscnet.config import Config

import loss_f64
from test_gpu_latent import count_calls
from test_loss_cpu import REFERENCE_KEYS, fixture_inputs

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
EXACT = ('pos_ratio', 'neg_ratio', 'obj_acc')
NH, NS, NC = 12, 8, 8


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "F_LOSS.npz"))


def to_cuda(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def as_floats(d):
    return {k: float(d[k]) for k in REFERENCE_KEYS}


def check_arrays(got, label, mask, assignment):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
    np.testing.assert_array_equal(got[0].cpu().numpy(), label)
    np.testing.assert_array_equal(got[1].cpu().numpy(), mask)
    np.testing.assert_array_equal(got[2].cpu().numpy(), assignment)


def head_views(est):
    """the same predictions as slices of one (B, C, K) head output, as ProposalModule's decode_scores hands them on"""
    from rfdnet_amd.iscnet.proposal_module import head_layout
    layout, C = head_layout(NH, NS, NC)
    B, K = est['center'].shape[:2]
    net = torch.zeros(B, C, K, device="cuda")
    per_prop = net.transpose(2, 1)
    out = dict(est)
    for name, (at, width) in layout.items():
        if name == 'center_offset':
            continue
        per_prop[:, :, at:at + width] = est[name].reshape(B, K, width)
        piece = per_prop[:, :, at:at + width]
        out[name] = piece.view(B, K, NS, 3) if name == 'size_residuals_normalized' else piece
        assert not out[name].is_contiguous() or width == 1
    return out


@pytest.mark.parametrize("vote_factor", [1, 3])
def test_detection_loss_on_the_fixture(hip, fx, vote_factor, monkeypatch):
    """every key against the reference's float64 run.  Measured on the MI355X (the reference's own fp32 run in brackets):
    total 6.0e-7 (6.0e-7) / 6.9e-7 (1.2e-6) at vote_factor 1 / 3, vote_loss 6.6e-9 / 3.3e-8 (the same), objectness_loss
    1.2e-8 (1.2e-8), box_loss 7.7e-8 (4.3e-8), sem_cls_loss 6.5e-8 (1.7e-7), size_cls_loss 2.3e-7 (2.5e-7), size_reg_loss
    6.4e-9 (5.3e-8); bounds 1.7e-7 (center_loss) ... 1.2e-4 (total)."""
    from rfdnet_amd.iscnet import loss
    est_np, gt_np = fixture_inputs(fx, vote_factor)
    est, gt = to_cuda(est_np), to_cuda(gt_np)
    cfg = Config(mean_size_arr=fx["mean_size_arr"]).dataset_config
    loss.DetectionLoss()(est, gt, cfg)                                  # uploads the mean sizes, once per config
    names = count_calls(hip, monkeypatch)
    got = loss.DetectionLoss()(est, gt, cfg)
    assert names == ["rfd_vote_loss_partial", "rfd_proposal_loss_partial", "rfd_detection_loss_finish"] and len(names) <= 3
    assert tuple(got) == REFERENCE_KEYS
    assert torch.is_tensor(got['total']) and got['total'].is_cuda and got['total'].dim() == 0
    assert all(type(got[k]) is float for k in REFERENCE_KEYS[1:])
    ref64, ref32, dev = (fx[n % vote_factor] for n in ("ref64_vf%d", "ref32_vf%d", "ref32_dev_vf%d"))
    vals = as_floats(got)
    for i, k in enumerate(REFERENCE_KEYS):
        bound = max(8 * dev[i], 64 * ULP * abs(ref64[i]))
        print("vote_factor %d %-18s device %.9g f64 %.12g |diff| %.2e (reference fp32 %.2e) bound %.2e"
              % (vote_factor, k, vals[k], ref64[i], abs(vals[k] - ref64[i]), dev[i], bound))
    for i, k in enumerate(REFERENCE_KEYS):
        if k in EXACT:
            assert np.float32(vals[k]) == np.float32(ref32[i]) == np.float32(ref64[i]), k
        else:
            assert abs(vals[k] - ref64[i]) <= max(8 * dev[i], 64 * ULP * abs(ref64[i])), k
    # the three stand-alone functions agree with the dictionary
    del names[:]
    vote = loss.compute_vote_loss(est, gt)
    obj, label, mask, assignment = loss.compute_objectness_loss(est, gt)
    check_arrays((label, mask, assignment), fx["objectness_label"], fx["objectness_mask"], fx["object_assignment"])
    box = loss.compute_box_and_sem_cls_loss(est, gt, {'object_assignment': assignment, 'objectness_label': label}, cfg)
    assert len(names) == 6
    assert float(vote) == vals['vote_loss'] and float(obj) == vals['objectness_loss']
    for k, v in zip(('center_loss', 'heading_cls_loss', 'heading_reg_loss', 'size_cls_loss', 'size_reg_loss',
                     'sem_cls_loss'), box):
        assert v.is_cuda and v.dim() == 0 and float(v) == vals[k], k
    # another assignment gives other box terms: meta_data is read, not recomputed
    other = loss.compute_box_and_sem_cls_loss(est, gt, {'object_assignment': (assignment + 1) % 6,
                                                        'objectness_label': label}, cfg)
    assert float(other[1]) != vals['heading_cls_loss']
    # the head's strided slices are read in place and give the same bits
    views = head_views(est)
    again = loss.DetectionLoss()(views, gt, cfg)
    assert as_floats(again) == vals


RAGGED = [(1, 1, 1, 1, 1, 6), (1, 63, 65, 3, 2, 1), (3, 257, 256, 64, 3, 1)]        # (B, S, K, G, vote_factor, seed)


def ragged_inputs(B, S, K, G, vote_factor, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    N = S + 37
    valid = max(1, G // 2)                                               # the rest of the rows are zero-padded
    gt = {'center_label': np.zeros((B, G, 3), f), 'heading_class_label': np.zeros((B, G), np.int64),
          'heading_residual_label': np.zeros((B, G), f), 'size_class_label': np.zeros((B, G), np.int64),
          'size_residual_label': np.zeros((B, G, 3), f), 'sem_cls_label': np.zeros((B, G), np.int64),
          'box_label_mask': np.zeros((B, G), f)}
    gt['center_label'][:, :valid] = rng.uniform(-3, 3, (B, valid, 3))
    gt['heading_class_label'][:, :valid] = rng.integers(0, NH, (B, valid))
    gt['heading_residual_label'][:, :valid] = rng.uniform(-0.26, 0.26, (B, valid))
    gt['size_class_label'][:, :valid] = rng.integers(0, NS, (B, valid))
    gt['size_residual_label'][:, :valid] = rng.normal(0, 0.3, (B, valid, 3))
    gt['sem_cls_label'][:, :valid] = rng.integers(0, NC, (B, valid))
    gt['box_label_mask'][:, :valid] = 1
    row = rng.integers(0, G, (B, K))                                     # padded rows draw proposals too
    offset = rng.normal(0, 1, (B, K, 3))
    offset *= (rng.uniform(0.02, 0.9, (B, K, 1)) / np.linalg.norm(offset, axis=2, keepdims=True))
    agg = np.take_along_axis(gt['center_label'].astype(np.float64), row[..., None].repeat(3, 2), 1) + offset
    est = {'aggregated_vote_xyz': agg.astype(f), 'center': (agg + rng.normal(0, 0.08, agg.shape)).astype(f),
           'objectness_scores': rng.normal(0, 2, (B, K, 2)).astype(f), 'heading_scores': rng.normal(0, 2, (B, K, NH)).astype(f),
           'heading_residuals_normalized': rng.normal(0, 1.2, (B, K, NH)).astype(f),
           'size_scores': rng.normal(0, 2, (B, K, NS)).astype(f),
           'size_residuals_normalized': rng.normal(0, 1.2, (B, K, NS, 3)).astype(f),
           'sem_cls_scores': rng.normal(0, 2, (B, K, NC)).astype(f)}
    gt['vote_label_mask'] = (rng.random((B, N)) < 0.5).astype(np.int64)
    gt['vote_label_mask'][:, 0] = 1
    gt['vote_label'] = (rng.normal(0, 0.5, (B, N, 9)) * gt['vote_label_mask'][..., None]).astype(f)
    est['seed_inds'] = np.stack([rng.permutation(N)[:S] for _ in range(B)]).astype(np.int32)
    est['seed_inds'][:, 0] = 0
    est['seed_xyz'] = rng.uniform(-3, 3, (B, S, 3)).astype(f)
    est['vote_xyz'] = (np.repeat(est['seed_xyz'], vote_factor, 1) + rng.normal(0, 0.4, (B, S * vote_factor, 3))).astype(f)
    return est, gt, rng.uniform(0.4, 1.5, (NS, 3))


@pytest.mark.parametrize("B,S,K,G,vote_factor,seed", RAGGED)
def test_detection_loss_ragged_shapes(hip, B, S, K, G, vote_factor, seed):
    """one element of everything; sizes below and beside the 64-lane wave; more than one scene, 256 proposals = the whole
    workgroup and S one past it.  Measured on the MI355X: the nearest a key comes to its bound is objectness_loss at
    (1,1,1,1), 2.1e-8 of 7.4e-8 (one confident proposal: the term is log(1 + 0.02)); elsewhere a hundredth of the bound."""
    from rfdnet_amd.iscnet import loss
    est_np, gt_np, mean_size = ragged_inputs(B, S, K, G, vote_factor, seed)
    assert loss_f64.threshold_margin(est_np, gt_np) > 1e-4
    assert loss_f64.distinct_gap(est_np['aggregated_vote_xyz'], gt_np['center_label']).min() > 1e-4
    assert (est_np['objectness_scores'][..., 0] != est_np['objectness_scores'][..., 1]).all()
    want, label, mask, assignment = loss_f64.detection_loss(est_np, gt_np, mean_size)
    assert label.sum() >= 1 and (B * K == 1 or (1 - mask).sum() >= 1)
    est, gt = to_cuda(est_np), to_cuda(gt_np)
    cfg = Config(mean_size_arr=mean_size).dataset_config
    vals = as_floats(loss.DetectionLoss()(est, gt, cfg))
    for k in REFERENCE_KEYS:
        print("(%d,%d,%d,%d) %-18s device %.9g f64 %.12g |diff| %.2e bound %.2e"
              % (B, S, K, G, k, vals[k], want[k], abs(vals[k] - want[k]), 64 * ULP * abs(want[k])))
    for k in REFERENCE_KEYS:
        if k in EXACT:
            assert np.float32(vals[k]) == want[k], k
        else:
            assert abs(vals[k] - want[k]) <= 64 * ULP * abs(want[k]), k
    check_arrays(loss.compute_objectness_loss(est, gt)[1:], label, mask, assignment)


def test_detection_loss_is_deterministic(hip):
    from rfdnet_amd.iscnet import loss
    est_np, gt_np, mean_size = ragged_inputs(*RAGGED[2])
    est, gt = to_cuda(est_np), to_cuda(gt_np)
    cfg = Config(mean_size_arr=mean_size).dataset_config
    a, b = loss.DetectionLoss()(est, gt, cfg), loss.DetectionLoss()(est, gt, cfg)
    assert as_floats(a) == as_floats(b) and torch.equal(a['total'], b['total'])
    for x, y in zip(loss.compute_objectness_loss(est, gt), loss.compute_objectness_loss(est, gt)):
        assert torch.equal(x, y)


def test_mask_loss_on_the_fixture(hip, fx, monkeypatch):
    from rfdnet_amd.iscnet import pointseg
    logp, grouped, wanted, trans = to_cuda({k: fx["mask_" + k] for k in ("logp", "grouped", "wanted", "trans")}).values()
    names = count_calls(hip, monkeypatch)
    got = pointseg.mask_loss_rows(logp, grouped, wanted, trans)
    assert names == ["rfd_mask_loss_partial", "rfd_mask_loss_finish"] and len(names) <= 2
    ref64, dev = float(fx["mask_ref64"]), float(fx["mask_ref32_dev"])
    bound = max(8 * dev, 64 * ULP * abs(ref64))
    print("mask loss device %.9g f64 %.12g |diff| %.2e (reference fp32 %.2e) bound %.2e"
          % (float(got), ref64, abs(float(got) - ref64), dev, bound))
    assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
    assert abs(float(got) - ref64) <= bound
    assert torch.equal(got, pointseg.mask_loss_rows(logp, grouped, wanted, trans))
    # the reference's module interface: (M, 2) log-probabilities and (M,) 0/1 targets
    target = (grouped == wanted[:, None].float()).view(-1).long()
    assert torch.equal(pointseg.get_loss()(logp.view(-1, 2), target, trans, None), got)
    # a row-strided label view (the grouped feature channel) is read in place
    wide = torch.full((grouped.shape[0], grouped.shape[1] + 3), 7.0, device="cuda")
    wide[:, :grouped.shape[1]] = grouped
    assert torch.equal(pointseg.mask_loss_rows(logp, wide[:, :grouped.shape[1]], wanted, trans), got)


@pytest.mark.parametrize("P", [1, 63, 1024])
def test_mask_loss_ragged_shapes(hip, P):
    from rfdnet_amd.iscnet import pointseg
    rng = np.random.default_rng(P)
    Kp = 3
    logits = rng.normal(0, 2, (Kp, P, 2)).astype(np.float32)
    logp = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    grouped = rng.integers(0, 4, (Kp, P)).astype(np.float32)
    wanted = np.array([grouped[0, 0], 2, 11], np.int64)
    trans = (np.eye(64)[None] + 0.1 * rng.normal(0, 1, (Kp, 64, 64))).astype(np.float32)
    want = loss_f64.mask_loss(logp, grouped, wanted, trans)
    got = float(pointseg.mask_loss_rows(*to_cuda({'a': logp, 'b': grouped, 'c': wanted, 'd': trans}).values()))
    print("P = %d: device %.9g f64 %.12g |diff| %.2e bound %.2e" % (P, got, want, abs(got - want), 64 * ULP * abs(want)))
    assert abs(got - want) <= 64 * ULP * abs(want)


def labelled_scene():
    """the 4096-point synthetic scene with its twelve cuboids as label rows 0..11 of 64, votes and instance labels, and
    the completion ground truth of tests/test_gpu_latent.py in the same rows"""
    pc, boxes, cls = synthetic.synthetic_scene(seed=3, n_raw=5000, n_points=4096, return_boxes=True)
    data = synthetic.scene_labels(pc, boxes, cls, G=64)
    T = 200
    pts, occ, vox = synthetic.object_occupancy(boxes, n_points=T, seed=9)
    data.update(object_points=np.zeros((1, 64, T, 3), np.float32), object_points_occ=np.zeros((1, 64, T), np.float32),
                object_voxels=np.zeros((1, 64, 16, 16, 16), np.float32))
    data['object_points'][0, :12], data['object_points_occ'][0, :12], data['object_voxels'][0, :12] = pts, occ, vox
    data = to_cuda(data)
    data['point_clouds'] = torch.from_numpy(pc[None]).cuda()
    return data, boxes


def test_skip_propagation_forward(hip, monkeypatch):
    from rfdnet_amd.iscnet import pointseg
    from rfdnet_amd.iscnet.skip_propagation import SkipPropagation
    data, boxes = labelled_scene()
    sp = SkipPropagation(Config())
    synthetic.load_seeded(sp, 11)
    sp = sp.cuda().eval()
    rng = np.random.default_rng(2)
    K = 7
    pick = np.array([0, 3, 5, 5, 8, 11, 2])
    box_xyz = torch.from_numpy((boxes[pick, :3] + rng.normal(0, 0.05, (K, 3))).astype(np.float32)[None]).cuda()
    angles = torch.from_numpy(boxes[pick, 6].astype(np.float32)[None]).cuda()
    feats = torch.from_numpy(rng.normal(0, 1, (1, 128, K)).astype(np.float32)).cuda()
    wanted = data['object_instance_labels'][:, torch.from_numpy(pick).cuda()].clone()
    wanted[0, 6] = 40                                                     # a proposal whose label no point carries
    with torch.no_grad():
        sp.generate(box_xyz, angles, feats, data['point_clouds'])         # packs the weights, once per network
        names = count_calls(hip, monkeypatch)
        codes = sp.generate(box_xyz, angles, feats, data['point_clouds'])
    plain = list(names)
    del names[:]
    seen = {}
    rows = pointseg.mask_loss_rows
    monkeypatch.setattr(pointseg, "mask_loss_rows", lambda *a: (seen.update(args=a), rows(*a))[1])
    codes2, mask_loss = sp(box_xyz, angles, feats, data['point_clouds'], data['point_instance_labels'], wanted)
    assert torch.equal(codes, codes2) and codes.shape == (1, 512, K)
    extra = ["rfd_mask_loss_partial", "rfd_mask_loss_finish"]
    assert sorted(names) == sorted(plain + extra) and [n for n in names if n not in extra] == plain
    logp, grouped, want_labels, trans, scale = seen['args']
    assert logp.shape == (K, 1024, 2) and grouped.shape == (K, 1024) and scale == 0.001
    g = grouped.cpu().numpy()
    assert set(np.unique(g)) <= set(range(13)) and (g == wanted.cpu().numpy().reshape(K, 1)).sum(1)[:6].min() > 0
    assert (g[6] == 40).sum() == 0
    want = loss_f64.mask_loss(logp.cpu().numpy(), g, want_labels.cpu().numpy(), trans.cpu().numpy())
    print("SkipPropagation.forward: mask loss %.9g f64 %.12g |diff| %.2e" % (float(mask_loss), want, abs(float(mask_loss) - want)))
    assert mask_loss.dim() == 0 and abs(float(mask_loss) - want) <= 64 * ULP * abs(want)
    assert hip.stream_status_bits() == 0


def test_evaluate_with_losses(hip, monkeypatch):
    from rfdnet_amd.iscnet import loss
    from rfdnet_amd.iscnet.network import ISCNet
    cfg = Config({'data': {'latent_encoder': True}, 'generation': {'resolution_0': 8, 'upsampling_steps': 0}},
                 mean_size_arr=np.full((8, 3), 0.8))
    cfg.eval_overrides = dict(getattr(cfg, 'eval_overrides', None) or {}, remove_empty_box=False)
    net = ISCNet(cfg)
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    detect = net.detect

    def every_proposal_is_an_object(point_clouds):
        ep, pf = detect(point_clouds)
        ep['objectness_scores'] = torch.tensor([0.0, 4.0], device="cuda").expand_as(ep['objectness_scores']).contiguous()
        return ep, pf
    net.detect = every_proposal_is_an_object
    data, _ = labelled_scene()
    ep0, ids0, meshes0, rec0 = net.evaluate(data, fit=False)
    assert 'loss' not in ep0
    Kp = ids0.shape[1]
    eps = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (Kp, 32)).astype(np.float32)).cuda()
    ep, ids, meshes, rec = net.evaluate(data, fit=False, completion=True, completion_eps=eps, losses=True)
    # meshes and records are those of losses=False
    assert torch.equal(ids, ids0) and len(meshes) == len(meshes0) == Kp >= 1
    for a, b in zip(meshes, meshes0):
        assert torch.equal(torch.as_tensor(a.vertices), torch.as_tensor(b.vertices))
        assert torch.equal(torch.as_tensor(a.faces), torch.as_tensor(b.faces))
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(rec.compact()[k], rec0.compact()[k])
    out = ep['loss']
    assert tuple(out) == REFERENCE_KEYS + ('completion_loss', 'mask_loss') and len(out) == 15
    assert out['total'].is_cuda and out['total'].dim() == 0 and all(type(out[k]) is float for k in list(out)[1:])
    assert all(np.isfinite(float(v)) for v in out.values())
    # the detection part is DetectionLoss on the scene's end_points, bit for bit; the completion part ONet_Loss's
    det = loss.DetectionLoss()(ep, data, cfg.dataset_config)
    assert {k: out[k] for k in REFERENCE_KEYS[1:]} == {k: det[k] for k in REFERENCE_KEYS[1:]}
    assert out['completion_loss'] == float(ep['completion_loss']) and out['mask_loss'] > 0
    box = out['center_loss'] + 0.1 * out['heading_cls_loss'] + out['heading_reg_loss'] + 0.1 * out['size_cls_loss'] + \
        out['size_reg_loss']
    parts = [10 * out['vote_loss'], 5 * out['objectness_loss'], 10 * box, out['sem_cls_loss'],
             0.005 * out['completion_loss'], 0.5 * out['mask_loss']]
    print("K' = %d: %s" % (Kp, {k: float(v) for k, v in out.items()}))
    # each part is an fp32 rounding of its f64 value and `total` two more fp32 operations on them
    assert abs(float(out['total']) - sum(parts)) <= 8 * ULP * sum(abs(p) for p in parts)
    assert abs(out['box_loss'] - box) <= 8 * ULP * box
    # without the instance labels: mask loss 0, everything else unchanged
    bare = {k: v for k, v in data.items() if k not in ('point_instance_labels', 'object_instance_labels')}
    ep2, _, _, _ = net.evaluate(bare, fit=False, completion=True, completion_eps=eps, losses=True)
    assert ep2['loss']['mask_loss'] == 0.0
    assert {k: ep2['loss'][k] for k in REFERENCE_KEYS[1:]} == {k: out[k] for k in REFERENCE_KEYS[1:]}
    # without completion: the detection keys are the same and the completion loss is 0
    ep3, _, _, _ = net.evaluate(data, fit=False, losses=True)
    assert ep3['loss']['completion_loss'] == 0.0 and ep3['loss']['mask_loss'] == out['mask_loss']
    assert ep3['loss']['vote_loss'] == out['vote_loss']
    assert hip.stream_status_bits() == 0
