"""CPU: the detection-evaluation restatement (tests/eval_det_f64.py) against the reference's own results in
tests/golden/F_AP.npz, the host half of rfdnet_amd.iscnet.evaluation (APCalculator), gather_records over two gloo
ranks, and synthetic_scene(return_boxes=True).

Tolerance 1e-12 on IoU / rec / prec / ap: the restatement takes the clipped polygon's area as a shoelace sum where the
reference asks scipy's ConvexHull; on 6000 random and near-duplicate pairs the two differ by at most 1.5e-14, so 1e-12
is two orders above that rounding and six below the 1e-6 band the fixture keeps clear around the thresholds.
A class with predictions and no ground truth has recall 0 / 0 = NaN in the reference; NaN must sit in the same
places (assert_allclose with equal_nan)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_det_f64 as E
from rfdnet_amd import sharding, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = (("pcp1", True), ("pcp0", False))
THR = (0.25, 0.5)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "F_AP.npz"))


def restated_records(fx, pcp, iou3d=None):
    return E.scene_records(fx['corners'], fx['obj_prob'], fx['sem_cls_probs'], fx['pred_sem_cls'], fx['pred_mask'],
                           fx['gt_corners'], fx['gt_sem_cls_label'], fx['gt_box_label_mask'] == 1, thr=THR,
                           conf_thresh=float(fx['conf_thresh']), per_class_proposal=pcp, iou3d=iou3d)


def assert_metrics_equal(got, fx, key):
    keys = list(fx[key + '_metric_keys'])
    assert list(got.keys()) == keys
    np.testing.assert_allclose(np.array([got[k] for k in keys], np.float64), fx[key + '_metric_values'],
                               rtol=0, atol=1e-12, equal_nan=True)


def test_fixture_covers_the_cases(fx):
    S, K = fx['pred_mask'].shape
    gtv = fx['gt_box_label_mask'] == 1
    assert S >= 4 and K == 256 and fx['sem_cls_probs'].shape[2] == 8 and gtv.sum(1).max() <= 64
    assert (fx['pred_mask'].sum(1) == 0).any() and (gtv.sum(1) == 0).any()
    labels = fx['gt_sem_cls_label'][gtv]
    assert 7 not in labels and (fx['pcp0_cls'] == 7).any()                    # predictions, no ground truth
    assert 6 in labels and not (fx['pcp0_cls'] == 6).any()                    # ground truths, no prediction
    v = fx['iou3d'][np.broadcast_to(gtv[:, None, :], fx['iou3d'].shape)]
    assert min(np.abs(v - t).min() for t in THR) > 1e-6
    assert ((v > 0.5).sum() > 10) and ((v > 0.25) & (v < 0.5)).sum() > 10


def test_restated_iou_matches_the_reference(fx):
    gtv = fx['gt_box_label_mask'] == 1
    for s in range(gtv.shape[0]):
        gi = np.nonzero(gtv[s])[0]
        i3, i2 = E.box3d_iou_matrix(fx['corners'][s], fx['gt_corners'][s][gi])
        d3 = np.abs(i3 - fx['iou3d'][s][:, gi]).max() if len(gi) else 0.0
        d2 = np.abs(i2 - fx['iou2d'][s][:, gi]).max() if len(gi) else 0.0
        print("scene %d: max |d iou3d| %.3g, max |d iou2d| %.3g" % (s, d3, d2))
        assert d3 <= 1e-12 and d2 <= 1e-12


def test_restated_gt_corners_match_the_reference(fx):
    """parse_groundtruths' decoding, restated: class2angle / class2size / get_3d_box"""
    gtv = fx['gt_box_label_mask'] == 1
    for s, g in zip(*np.nonzero(gtv)):
        ang = fx['gt_heading_class_label'][s, g] * (2 * np.pi / 12.) + np.float64(fx['gt_heading_residual_label'][s, g])
        ang = ang - 2 * np.pi if ang > np.pi else ang
        size = fx['mean_size_arr'][fx['gt_size_class_label'][s, g]] + fx['gt_size_residual_label'][s, g].astype(np.float64)
        c = E.depth_box_corners(fx['gt_center_label'][s, g].astype(np.float64), size, ang)
        np.testing.assert_allclose(c, fx['gt_corners'][s, g], rtol=0, atol=1e-12)


@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_restated_matching_and_curves_match_the_reference(fx, tag, pcp):
    iou3d = np.zeros_like(fx['iou3d'])
    gtv = fx['gt_box_label_mask'] == 1
    for s in range(gtv.shape[0]):
        gi = np.nonzero(gtv[s])[0]
        if len(gi):
            iou3d[s][:, gi] = E.box3d_iou_matrix(fx['corners'][s], fx['gt_corners'][s][gi])[0]
    rec, _ = restated_records(fx, pcp, iou3d)
    # the reference's batch_pred_map_cls scores, as a multiset per class
    for c in range(8):
        np.testing.assert_array_equal(np.sort(rec['score'][rec['cls'] == c]), np.sort(fx[tag + '_score'][fx[tag + '_cls'] == c]))
    for ti, t in enumerate(THR):
        key = "%s_%g" % (tag, t)
        cur = E.class_curves([rec], ti)
        assert sorted(cur) == list(fx[key + '_classes'])
        for c in cur:
            np.testing.assert_allclose(cur[c][2], fx['%s_ap_%d' % (key, c)], rtol=0, atol=1e-12)
            np.testing.assert_allclose(cur[c][0], fx['%s_rec_%d' % (key, c)], rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(cur[c][1], fx['%s_prec_%d' % (key, c)], rtol=0, atol=1e-12)
            if np.ndim(cur[c][0]):
                np.testing.assert_array_equal(cur[c][3], fx['%s_tp_%d' % (key, c)])       # every tp / fp flag
        assert_metrics_equal(E.metrics([rec], ti), fx, key)
        every = E.class_curves([rec], ti, use_07_metric=False)               # the all-points AP
        for c in every:
            np.testing.assert_allclose(every[c][2], fx['%s_apall_%d' % (key, c)], rtol=0, atol=1e-12, equal_nan=True)
        assert sum(np.isfinite(every[c][2]) and every[c][2] > 0 for c in every) >= 5


@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_apcalculator_on_restated_records(fx, tag, pcp):
    from rfdnet_amd.iscnet.evaluation import APCalculator
    rec, _ = restated_records(fx, pcp, fx['iou3d'])
    calc = APCalculator(THR)
    calc.step(rec)
    both = calc.compute_metrics()
    assert len(both) == 2
    for ti, t in enumerate(THR):
        assert_metrics_equal(both[ti], fx, "%s_%g" % (tag, t))
    one = APCalculator(0.25)
    one.step(dict(rec, tp=rec['tp'][:1], thr=(0.25,)))
    assert_metrics_equal(one.compute_metrics(), fx, tag + "_0.25")
    named = APCalculator(0.25, {i: "c%d" % i for i in range(8)})
    named.step(dict(rec, tp=rec['tp'][:1], thr=(0.25,)))
    assert 'c0 Average Precision' in named.compute_metrics()
    all_points = one.compute_metrics(use_07_metric=False)
    assert list(all_points) == list(one.compute_metrics())
    want = {c: float(fx['%s_0.25_apall_%d' % (tag, c)]) for c in fx[tag + '_0.25_classes']}
    for c, v in want.items():
        np.testing.assert_allclose(all_points['%d Average Precision' % c], v, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(all_points['mAP'], np.mean(list(want.values())), rtol=0, atol=1e-12, equal_nan=True)
    for ti, t in enumerate(THR):                                            # and both forms of voc_ap, class by class
        for use07, name in ((True, 'ap'), (False, 'apall')):
            for c, cur in calc.class_curves(ti, use07).items():
                np.testing.assert_allclose(cur[2], fx['%s_%g_%s_%d' % (tag, t, name, c)], rtol=0, atol=1e-12, equal_nan=True)
    with pytest.raises(ValueError):
        one.step(rec)                                                          # matched at other thresholds


def test_evaluate_mesh_raises():
    from rfdnet_amd.iscnet.evaluation import APCalculator
    with pytest.raises(NotImplementedError, match="binvox"):
        APCalculator(0.25, None, evaluate_mesh=True)


def test_native_symbols_and_module_present():
    from rfdnet_amd import _lib
    from rfdnet_amd.iscnet import evaluation
    assert {"rfd_box3d_iou", "rfd_ap_match"} <= set(_lib.exported_symbols())
    assert os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "include", "rfd_eval.h"))
    for n in ("parse_groundtruths", "scene_records", "APCalculator"):
        assert hasattr(evaluation, n)


# ------------------------------------------------------------------------------------------------ gather_records
def _split(rec, rank, world, rng_seed=0):
    """a permuted share of the records for `rank`; the ground-truth counts are split too"""
    n = len(rec['cls'])
    perm = np.random.default_rng(rng_seed).permutation(n)
    mine = perm[rank::world] if rank else perm[0::world][:-7]                 # unequal lengths
    if rank == world - 1:
        mine = np.concatenate([mine, perm[0::world][-7:]])
    npos = np.asarray(rec['npos']) // world + (np.asarray(rec['npos']) % world if rank == 0 else 0)
    return {'cls': rec['cls'][mine], 'score': rec['score'][mine], 'tp': rec['tp'][:, mine], 'npos': npos,
            'thr': rec['thr']}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, rec, q, idle_rank=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if idle_rank is None:
        g = sharding.gather_records(_split(rec, rank, world), dist)
    else:                                       # one rank was dealt no scene: it has no record at all
        g = sharding.gather_records([] if rank == idle_rank else [rec], dist, thr=THR)
    q.put((rank, {k: (v if k == 'thr' else np.asarray(v)) for k, v in g.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_records_two_gloo_ranks(fx):
    from rfdnet_amd.iscnet.evaluation import APCalculator
    rec, _ = restated_records(fx, True, fx['iou3d'])
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, rec, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g0, g1 = res[0][1], res[1][1]
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(g0[k], g1[k])                           # identical on every rank
    # the permuted union: the same (class, score, flags) rows, and the same ground-truth counts
    rows = lambda r: sorted(zip(r['cls'].tolist(), r['score'].tolist(), *[t.tolist() for t in r['tp']]))
    assert rows(g0) == rows(rec)
    np.testing.assert_array_equal(g0['npos'], rec['npos'])
    single, sharded = APCalculator(THR), APCalculator(THR)
    single.step(rec)
    sharded.step(g0)
    for a, b in zip(single.compute_metrics(), sharded.compute_metrics()):
        assert list(a) == list(b)
        np.testing.assert_array_equal(np.array(list(a.values()), np.float64), np.array(list(b.values()), np.float64))


@pytest.mark.parametrize("idle_rank", [0, 1])
def test_gather_records_with_a_rank_that_has_none(fx, idle_rank):
    rec, _ = restated_records(fx, True, fx['iou3d'])
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, rec, q, idle_rank)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, g in res:
        for k in ('cls', 'score', 'tp', 'npos'):
            np.testing.assert_array_equal(g[k], rec[k])
    with pytest.raises(ValueError):
        sharding.gather_records([], None)                                     # nothing to take the thresholds from
    empty = sharding.gather_records([], None, thr=THR)
    assert len(empty['cls']) == 0 and empty['tp'].shape == (2, 0) and empty['thr'] == THR


def test_gather_records_without_dist_is_the_identity(fx):
    rec, _ = restated_records(fx, False, fx['iou3d'])
    g = sharding.gather_records(rec, None)
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(g[k], rec[k])


# ------------------------------------------------------------------------------------------------ synthetic boxes
def test_synthetic_scene_boxes():
    kw = dict(seed=7, n_raw=30000, n_points=20000)
    pc = synthetic.synthetic_scene(**kw)
    pc2, boxes, cls = synthetic.synthetic_scene(return_boxes=True, **kw)
    assert pc.tobytes() == pc2.tobytes() and pc.dtype == pc2.dtype and pc.shape == pc2.shape     # bit-identical
    assert boxes.shape == (12, 7) and cls.shape == (12,) and cls.min() >= 0 and cls.max() < 8
    # every box holds its own surface: 38 % of the raw points are furniture, a twelfth of them on each cuboid, all
    # within the 5 mm noise (6 sigma = 3 cm) of its faces -- and no face point lies deeper inside than that
    expect = 0.38 * kw['n_raw'] / 12 * kw['n_points'] / kw['n_raw']
    p = pc[:, :3].astype(np.float64)
    for b in boxes:
        c, s = np.cos(b[6]), np.sin(b[6])
        d = p - b[:3]
        local = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
        inside = (np.abs(local) <= b[3:6] / 2 + 0.03).all(1)
        deep = (np.abs(local) <= b[3:6] / 2 - 0.03).all(1)
        assert (inside & ~deep).sum() >= 0.8 * expect, ((inside & ~deep).sum(), expect)
