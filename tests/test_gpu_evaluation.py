"""GPU (-m gpu): rfd_box3d_iou / rfd_ap_match (csrc/box_eval.hip) and rfdnet_amd.iscnet.evaluation against the
reference's own results (tests/golden/F_AP.npz) and the restatement tests/eval_det_f64.py.

Bounds.  IoU: |d| <= 1e-12 -- the kernel and the restatement run the same double arithmetic (the shoelace sums may
associate differently by an ulp of ~1e-16 on coordinates of a few metres), and the reference's ConvexHull area is
within 1.5e-14 of a shoelace sum (tests/test_evaluation_cpu.py); 1e-12 is two orders above both and six below the 1e-6
band the fixture keeps clear around the thresholds, so every true-positive flag must then be identical.
Ground-truth corners decoded on the device: 1e-12 as well (a few ulp of sin / cos on lengths of a few metres)."""
import os

import numpy as np
import pytest
import torch

import eval_det_f64 as E
from rfdnet_amd import synthetic
from rfdnet_amd.iscnet.config import ScannetConfig

pytestmark = pytest.mark.gpu
THR = (0.25, 0.5)
SETTINGS = (("pcp1", True), ("pcp0", False))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "F_AP.npz"))


def fixture_inputs(fx):
    parsed = {'pred_corners_3d_upright_camera': torch.from_numpy(fx['corners']).cuda(),
              'sem_cls_probs': torch.from_numpy(fx['sem_cls_probs']).cuda(),
              'obj_prob': torch.from_numpy(fx['obj_prob']).cuda(),
              'pred_sem_cls': torch.from_numpy(fx['pred_sem_cls']).cuda()}
    gts = {'gt_corners_3d_upright_camera': torch.from_numpy(fx['gt_corners']).cuda(),
           'sem_cls_label': torch.from_numpy(fx['gt_sem_cls_label']).cuda(),
           'box_label_mask': torch.from_numpy(fx['gt_box_label_mask']).cuda()}
    return {'pred_mask': torch.from_numpy(fx['pred_mask']).cuda()}, parsed, gts


def assert_metrics_equal(got, fx, key):
    keys = list(fx[key + '_metric_keys'])
    assert list(got.keys()) == keys
    np.testing.assert_allclose(np.array([got[k] for k in keys], np.float64), fx[key + '_metric_values'],
                               rtol=0, atol=1e-12, equal_nan=True)


# ---------------------------------------------------------------------------------------------------- rfd_box3d_iou
def test_iou_matches_the_reference(hip, fx):
    from rfdnet_amd.iscnet import evaluation
    i3, i2 = evaluation.box3d_iou(torch.from_numpy(fx['corners']).cuda(), torch.from_numpy(fx['gt_corners']).cuda(), True)
    i3, i2 = i3.cpu().numpy(), i2.cpu().numpy()
    m = np.broadcast_to((fx['gt_box_label_mask'] == 1)[:, None, :], i3.shape)
    d3, d2 = np.abs(i3 - fx['iou3d'])[m].max(), np.abs(i2 - fx['iou2d'])[m].max()
    print("vs reference: max |d iou3d| %.3g, max |d iou2d| %.3g over %d pairs" % (d3, d2, m.sum()))
    assert d3 <= 1e-12 and d2 <= 1e-12
    assert not np.isnan(i3).any() and not np.isnan(i2).any()
    assert (i3[~m] == 0).all() and (i2[~m] == 0).all()                   # all-zero (masked) ground truths: 0, not NaN


def generated_pairs():
    """K = 200 boxes x G = 100 boxes = 20 000 pairs; ground truth g is built FROM box g in a named way, every other
    pair of the matrix is a random one (mostly disjoint, some overlapping)"""
    rng = np.random.default_rng(12)
    K, G = 200, 100
    ctr = np.stack([rng.uniform(-2.5, 2.5, K), rng.uniform(-3, 3, K), rng.uniform(0.2, 1.2, K)], -1)
    size = rng.uniform(0.3, 1.8, (K, 3))
    ang = rng.uniform(-np.pi, np.pi, K)
    ang[:20] = 0.0                                                       # axis-aligned
    g_ctr, g_size, g_ang = ctr[:G].copy(), size[:G].copy(), ang[:G].copy()
    kind = np.arange(G) % 6
    for g in range(G):
        if kind[g] == 0:                                                 # identical
            pass
        elif kind[g] == 1:                                               # contained
            g_size[g] *= 0.5
        elif kind[g] == 2:                                               # touching: shifted by its own length along l
            g_ctr[g, 0] += np.cos(ang[g]) * size[g, 0]
            g_ctr[g, 1] += np.sin(ang[g]) * size[g, 0]
        elif kind[g] == 3:                                               # rotated by 90 degrees about the centre
            g_ang[g] += np.pi / 2
        elif kind[g] == 4:                                               # disjoint: far away
            g_ctr[g, 0] += 40.0
        else:                                                            # perturbed
            g_ctr[g] += rng.normal(0, 0.1, 3)
            g_size[g] *= rng.uniform(0.8, 1.25, 3)
            g_ang[g] += rng.normal(0, 0.2)
    pred = np.stack([E.depth_box_corners(ctr[k], size[k], ang[k]) for k in range(K)])
    gt = np.stack([E.depth_box_corners(g_ctr[g], g_size[g], g_ang[g]) for g in range(G)])
    return pred, gt, kind


def test_iou_matches_the_restatement_on_generated_pairs(hip):
    from rfdnet_amd.iscnet import evaluation
    pred, gt, kind = generated_pairs()
    r3, r2 = E.box3d_iou_matrix(pred, gt)
    i3, i2 = evaluation.box3d_iou(torch.from_numpy(pred[None]).cuda(), torch.from_numpy(gt[None]).cuda(), True)
    i3, i2 = i3[0].cpu().numpy(), i2[0].cpu().numpy()
    print("vs restatement: max |d iou3d| %.3g, max |d iou2d| %.3g, %d of %d pairs overlap" %
          (np.abs(i3 - r3).max(), np.abs(i2 - r2).max(), (r3 > 0).sum(), r3.size))
    assert not np.isnan(i3).any() and not np.isnan(i2).any()
    assert np.abs(i3 - r3).max() <= 1e-12 and np.abs(i2 - r2).max() <= 1e-12
    assert ((i3 == 0) == (r3 == 0)).all() and ((i2 == 0) == (r2 == 0)).all()
    # the well-posed cases are what they say.  Not so the exactly identical and exactly touching pairs: their edges
    # coincide, the clip's intersection formula divides by a rounding residue, and the reference's own result is
    # arbitrary there (values above 1 occur, as do QhullErrors) -- kernel and restatement still agree to the bit
    d = np.arange(len(kind))
    assert (r3[d, d][kind == 4] == 0).all() and np.abs(r3[d, d][kind == 1] - 0.125).max() < 1e-9
    assert (r3[d, d][kind == 5] > 0.05).all()


def test_iou_of_a_zero_volume_box_is_zero(hip):
    from rfdnet_amd.iscnet import evaluation
    box = E.depth_box_corners((0, 0, 0.5), (1, 1, 1), 0.3)
    near = E.depth_box_corners((0.1, 0.05, 0.5), (1, 1, 1), 0.5)
    flat = E.depth_box_corners((0, 0, 0.5), (1, 1, 0), 0.3)               # no height
    line = E.depth_box_corners((0, 0, 0.5), (0, 1, 1), 0.3)               # no length: the rectangle is a segment
    point = np.zeros((8, 3))
    pred = torch.from_numpy(np.stack([near, flat, line, point])[None]).cuda()
    gt = torch.from_numpy(np.stack([box, flat, line, point])[None]).cuda()
    i3, i2 = evaluation.box3d_iou(pred, gt, True)
    i3, i2 = i3[0].cpu().numpy(), i2[0].cpu().numpy()
    assert not np.isnan(i3).any() and not np.isnan(i2).any()
    assert 0.5 < i3[0, 0] < 1
    assert (i3[1:] == 0).all() and (i3[:, 1:] == 0).all()
    r3, r2 = E.box3d_iou_matrix(pred[0].cpu().numpy(), gt[0].cpu().numpy())
    np.testing.assert_allclose(i3, r3, rtol=0, atol=1e-12)
    np.testing.assert_allclose(i2, r2, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- rfd_ap_match
@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_match_flags_equal_restatement_and_reference(hip, fx, tag, pcp):
    from rfdnet_amd.iscnet import evaluation
    eval_dict, parsed, gts = fixture_inputs(fx)
    rec = evaluation.scene_records(eval_dict, parsed, gts, {'per_class_proposal': pcp}, THR)
    want, want_tp = E.scene_records(fx['corners'], fx['obj_prob'], fx['sem_cls_probs'], fx['pred_sem_cls'],
                                    fx['pred_mask'], fx['gt_corners'], fx['gt_sem_cls_label'],
                                    fx['gt_box_label_mask'] == 1, thr=THR, per_class_proposal=pcp, iou3d=fx['iou3d'])
    rec.event.synchronize()
    tp = rec.tp.numpy()                                                   # the kernel's output, as it was copied
    assert tp.shape == want_tp.shape == (2, 5, 8, 256)                    # both thresholds in one launch
    np.testing.assert_array_equal(tp, want_tp)
    assert want_tp[0].sum() > want_tp[1].sum() > 0
    got = rec.compact()
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(got[k], want[k])
    zero_mask = np.nonzero(fx['pred_mask'].sum(1) == 0)[0]
    assert len(zero_mask) and (rec.valid.numpy()[zero_mask] == 0).all() and (tp[:, zero_mask] == 0).all()
    for ti, t in enumerate(THR):                                          # the reference's flags, in its sorted order
        key = "%s_%g" % (tag, t)
        cur = E.class_curves([got], ti)
        for c in cur:
            if np.ndim(cur[c][0]):
                np.testing.assert_array_equal(cur[c][3], fx['%s_tp_%d' % (key, c)])


def test_match_without_ground_truths(hip, fx):
    from rfdnet_amd.iscnet import evaluation
    eval_dict, parsed, gts = fixture_inputs(fx)
    none = {'gt_corners_3d_upright_camera': gts['gt_corners_3d_upright_camera'][:, :0],
            'sem_cls_label': gts['sem_cls_label'][:, :0], 'box_label_mask': gts['box_label_mask'][:, :0]}
    records = evaluation.scene_records(eval_dict, parsed, none, None, THR)                       # G = 0
    rec = records.compact()
    assert (records.tp.numpy() == 0).all() and rec['tp'].shape[1] == len(rec['cls']) > 0
    assert (rec['npos'] == 0).all()


def test_match_rejects_sizes_beyond_its_limits(hip):
    from rfdnet_amd.iscnet import evaluation
    for K, G in ((1025, 4), (8, 257)):
        iou = torch.zeros(1, K, G, dtype=torch.float64, device="cuda")
        order = torch.arange(K, dtype=torch.int32, device="cuda").view(1, 1, K).contiguous()
        valid = torch.ones(1, 1, K, dtype=torch.uint8, device="cuda")
        with pytest.raises(hip.RfdHipError):
            evaluation.ap_match(iou, order, valid, torch.zeros(1, G, dtype=torch.int32, device="cuda"),
                                torch.ones(1, G, dtype=torch.uint8, device="cuda"),
                                torch.tensor(THR, dtype=torch.float64, device="cuda"))
    # the stream is still usable: a launch at the limits, checked against the restatement
    rng = np.random.default_rng(2)
    K, G = 1024, 256
    iou = rng.random((1, K, G))
    score = rng.random((1, 2, K))
    gt_cls = rng.integers(0, 2, (1, G)).astype(np.int32)
    order = np.argsort(-score, -1, kind='stable').astype(np.int32)
    valid = (rng.random((1, 2, K)) < 0.7).astype(np.uint8)
    thr = (0.9, 0.99, 0.995, 0.999)
    tp = evaluation.ap_match(torch.from_numpy(iou).cuda(), torch.from_numpy(order).cuda(), torch.from_numpy(valid).cuda(),
                             torch.from_numpy(gt_cls).cuda(), torch.ones(1, G, dtype=torch.uint8, device="cuda"),
                             torch.tensor(thr, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tp.cpu().numpy(), E.ap_match(iou, order, valid, gt_cls, np.ones((1, G), np.uint8), thr))
    assert hip.stream_status_bits() == 0


# ---------------------------------------------------------------------------------- scene_records -> APCalculator
@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_metrics_equal_the_reference(hip, fx, tag, pcp):
    from rfdnet_amd.iscnet import evaluation
    eval_dict, parsed, gts = fixture_inputs(fx)
    calc = evaluation.APCalculator(THR)
    S = fx['pred_mask'].shape[0]
    for s in range(S):                                                    # scene by scene, as a sweep would
        one = lambda d: {k: v[s:s + 1] for k, v in d.items()}
        calc.step(evaluation.scene_records(one(eval_dict), one(parsed), one(gts), {'per_class_proposal': pcp}, THR))
    for ti, t in enumerate(THR):
        assert_metrics_equal(calc.compute_metrics()[ti], fx, "%s_%g" % (tag, t))
    # the reference's list format through the same kernels
    take = (fx['pred_mask'] == 1) & (fx['obj_prob'] > float(fx['conf_thresh']))
    pred_lists, gt_lists = [], []
    for s in range(S):
        js = np.nonzero(take[s])[0]
        if pcp:
            pred_lists.append([(c, fx['corners'][s, j], fx['sem_cls_probs'][s, j, c] * fx['obj_prob'][s, j])
                               for c in range(8) for j in js])
        else:
            pred_lists.append([(int(fx['pred_sem_cls'][s, j]), fx['corners'][s, j], fx['obj_prob'][s, j]) for j in js])
        gt_lists.append([(int(fx['gt_sem_cls_label'][s, g]), fx['gt_corners'][s, g])
                         for g in np.nonzero(fx['gt_box_label_mask'][s] == 1)[0]])
    lists = evaluation.APCalculator(THR)
    lists.step(pred_lists, gt_lists)
    for ti, t in enumerate(THR):
        assert_metrics_equal(lists.compute_metrics()[ti], fx, "%s_%g" % (tag, t))
    single = evaluation.APCalculator(0.5)
    single.step(pred_lists, gt_lists)
    assert_metrics_equal(single.compute_metrics(), fx, tag + "_0.5")


def test_parse_groundtruths_matches_the_reference(hip, fx):
    from rfdnet_amd.iscnet import evaluation
    names = ('center_label', 'heading_class_label', 'heading_residual_label', 'size_class_label',
             'size_residual_label', 'sem_cls_label', 'box_label_mask')
    out = evaluation.parse_groundtruths({k: torch.from_numpy(fx['gt_' + k]).cuda() for k in names},
                                        ScannetConfig(fx['mean_size_arr']))
    got = out['gt_corners_3d_upright_camera']
    assert got.dtype == torch.float64 and got.is_cuda
    np.testing.assert_allclose(got.cpu().numpy(), fx['gt_corners'], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------ end to end
def labels_from_proposals(parsed, pred_mask, mean_size_arr, conf=0.05, G=64):
    """ground-truth labels = perturbed copies of half of the surviving proposals (as the fixture's)"""
    rng = np.random.default_rng(8)
    box = parsed['box_params'][0].cpu().numpy()
    cls = parsed['pred_sem_cls'][0].cpu().numpy()
    surv = np.nonzero((pred_mask[0].cpu().numpy() == 1) & (parsed['obj_prob'][0].cpu().numpy() > conf))[0]
    pick = surv[::2][:G]
    gt = {'center_label': np.zeros((1, G, 3), np.float32), 'heading_class_label': np.zeros((1, G), np.int64),
          'heading_residual_label': np.zeros((1, G), np.float32), 'size_class_label': np.zeros((1, G), np.int64),
          'size_residual_label': np.zeros((1, G, 3), np.float32), 'sem_cls_label': np.zeros((1, G), np.int64),
          'box_label_mask': np.zeros((1, G), np.float32)}
    for j, k in enumerate(pick):
        ang = (box[k, 6] + rng.normal(0, 0.2)) % (2 * np.pi)
        shifted = (ang + np.pi / 12) % (2 * np.pi)
        hc = int(shifted / (np.pi / 6))
        gt['center_label'][0, j] = box[k, :3] + rng.normal(0, 0.15, 3)
        gt['heading_class_label'][0, j] = hc
        gt['heading_residual_label'][0, j] = shifted - (hc * (np.pi / 6) + np.pi / 12)
        gt['size_class_label'][0, j] = j % 8
        gt['size_residual_label'][0, j] = box[k, 3:6] * rng.uniform(0.8, 1.25, 3) - mean_size_arr[j % 8]
        gt['sem_cls_label'][0, j] = cls[k]
        gt['box_label_mask'][0, j] = 1
    return {k: torch.from_numpy(v).cuda() for k, v in gt.items()}, len(pick)


def test_evaluate_end_to_end(hip, golden_dir, monkeypatch):
    """ISCNet.evaluate on the F_NET scene with F_NMS's head overrides and mean sizes (tests/test_gpu_predictions.py)"""
    from rfdnet_amd.iscnet import evaluation
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    fn = np.load(os.path.join(golden_dir, "F_NET.npz"))
    fnms = np.load(os.path.join(golden_dir, "F_NMS.npz"))
    seed, n_raw, n_pts = (int(v) for v in fn["pc_seed"])
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=seed, n_raw=n_raw, n_points=n_pts)[None]).cuda()
    cfg = Config({'generation': {'resolution_0': 8, 'upsampling_steps': 1}}, mean_size_arr=fnms['mean_size_arr'])
    net = ISCNet(cfg)
    for name, s in (('backbone', 101), ('voting', 102), ('detection', 103), ('skip_propagation', 104),
                    ('completion', 105)):
        synthetic.load_seeded(getattr(net, name), s)
    net = net.cuda().eval()
    detect = net.detect

    def detect_like_the_fixture(point_clouds):
        ep, pf = detect(point_clouds)
        ep['objectness_scores'] = torch.from_numpy(fnms['objectness_scores']).cuda()
        ep['size_residuals_normalized'] = ep['size_residuals_normalized'] * 0.2
        return ep, pf
    net.detect = detect_like_the_fixture
    end_points, ids, meshes = net.generate({'point_clouds': pc}, selection='nms')
    np.testing.assert_array_equal(end_points['pred_mask'].cpu().numpy(), fnms['default_pred_mask'])
    labels, n_gt = labels_from_proposals(end_points['parsed_predictions'], end_points['pred_mask'], fnms['mean_size_arr'])
    assert n_gt > 5
    data = dict(labels, point_clouds=pc)
    unrefined = end_points['parsed_predictions']['pred_corners_3d_upright_camera'].clone()

    seen = []
    kernel = evaluation.box3d_iou
    monkeypatch.setattr(evaluation, "box3d_iou", lambda p, g, *a: (seen.append(p.clone()), kernel(p, g, *a))[1])
    take = ((end_points['pred_mask'] == 1) & (end_points['parsed_predictions']['obj_prob'] > 0.05)).cpu().numpy()
    results = {}
    for fit in (False, True):
        ep, ids2, meshes2, rec = net.evaluate(data, fit=fit)
        np.testing.assert_array_equal(ids2.cpu().numpy(), ids.cpu().numpy())
        assert len(meshes2) == len(meshes)
        # the records are those of parse_predictions' mask: every surviving proposal once per class
        np.testing.assert_array_equal(rec.compact()['npos'].sum(), n_gt)
        np.testing.assert_array_equal(rec.valid.numpy()[0], np.broadcast_to(take[0][None], (8, 256)).astype(np.uint8))
        assert len(rec.compact()['cls']) == 8 * take.sum()
        scored = ep['parsed_predictions']['pred_corners_3d_upright_camera']
        assert torch.equal(seen[-1], scored)                              # what the IoU kernel was given
        calc = evaluation.APCalculator(THR)
        calc.step(rec)
        results[fit] = calc.compute_metrics()
        want, _ = E.scene_records(scored.cpu().numpy(), ep['parsed_predictions']['obj_prob'].cpu().numpy(),
                                  ep['parsed_predictions']['sem_cls_probs'].cpu().numpy(),
                                  ep['parsed_predictions']['pred_sem_cls'].cpu().numpy(), ep['pred_mask'].cpu().numpy(),
                                  evaluation.parse_groundtruths(data, cfg.dataset_config)
                                  ['gt_corners_3d_upright_camera'].cpu().numpy(),
                                  labels['sem_cls_label'].cpu().numpy(), labels['box_label_mask'].cpu().numpy() == 1, thr=THR)
        got = rec.compact()
        np.testing.assert_array_equal(got['cls'], want['cls'])
        np.testing.assert_array_equal(got['score'], want['score'])
        np.testing.assert_array_equal(got['tp'], want['tp'])
        if fit:
            moved = (scored - unrefined).abs().amax(dim=(2, 3))[0]
            fitted = [j for _, j in ep['parsed_predictions']['fit_indices']]
            assert fitted and float(moved[fitted].max()) > 1e-4, "fit_mesh_to_scan moved no box"
            assert float(moved[[j for j in range(256) if j not in fitted]].max()) == 0.0
        else:
            assert torch.equal(scored, unrefined)
        assert hip.stream_status_bits() == 0                              # the stream's status word is clean
    assert results[False][0]['mAP'] > 0                                   # perturbed copies of proposals are found
