"""GPU (-m gpu): the kernels of csrc/boxes.hip (rfd_points_in_boxes, rfd_nms3d) through their C entry points, and
predictions.parse_predictions / get_proposal_id on crafted head outputs, against the float64 restatement
tests/predictions_f64.py (tied to the reference's run and to scipy by tests/test_predictions_cpu.py).

Every comparison is exact.  So that an exact comparison cannot hinge on the last place of a device cos/sin, each test
asserts its premise on the restatement alone: random NMS cases compare no overlap within IOU_MARGIN of the threshold,
and the few points within FACE_MARGIN of a face plane of any box are taken out of the input of both sides.  The
threshold cases are the opposite premise: small integers, exact in float64 by construction."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predictions_f64 as P  # noqa: E402
from predictions_f64 import MEAN_SIZES, all_bins_end_points, clustered_aabb  # noqa: E402

pytestmark = pytest.mark.gpu

IOU_MARGIN = 1e-9           # random NMS cases: no compared overlap may be this close to the threshold
FACE_MARGIN = 1e-6          # metres
FACE_SHARE = 1e-3           # at most this share of a case's points may lie within FACE_MARGIN of a face plane
FAR = 1e3                   # where such points are moved to: outside every box


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_nms(hip, aabb, order, cls, valid, thr, old_type, use_cls, keep_fill=7):
    """(B,K,...) numpy -> (return code, keep (B,K) uint8 as the kernel left it)"""
    B, K = cls.shape
    keep = torch.full((B, K), keep_fill, dtype=torch.uint8, device="cuda")
    t = [dev(aabb.astype(np.float64)), dev(order.astype(np.int32)), dev(cls.astype(np.int32)),
         dev(valid.astype(np.uint8))]
    rc = hip.lib().rfd_nms3d(B, K, float(thr), int(old_type), int(use_cls), *[x.data_ptr() for x in t],
                             keep.data_ptr(), hip.current_stream())
    torch.cuda.synchronize()
    return rc, keep.cpu().numpy()


def want_nms(aabb, order, cls, valid, thr, old_type, use_cls):
    both = [P.nms3d(aabb[b], order[b], cls[b], valid[b], thr, old_type, use_cls) for b in range(len(cls))]
    return np.stack([k for k, _ in both]), min(m for _, m in both)


# ------------------------------------------------------------------------------------------------ rfd_nms3d

@pytest.mark.parametrize("K", [1, 63, 64, 65, 256, 1000, 1024])
@pytest.mark.parametrize("old_type,use_cls", list(itertools.product((0, 1), repeat=2)))
def test_nms3d_dense_clusters_three_scenes(hip, K, old_type, use_cls):
    """three scenes with their own boxes, classes (4 to 8 interleaved), validity and a random order; boxes in dense
    clusters so that most are suppressed; a few zero-volume boxes among them"""
    B = 3
    rng = np.random.default_rng(1000 * K + 2 * old_type + use_cls)
    aabb = np.stack([clustered_aabb(rng, K, max(1, K // 64), flat_share=0.05, jitter=0.1, half=(0.4, 0.6)) for _ in range(B)])
    order = np.stack([rng.permutation(K) for _ in range(B)])
    cls = np.stack([rng.permutation(K) % n for n in rng.permutation(5)[:B] + 4])
    valid = rng.random((B, K)) < 0.85
    thr = (0.1, 0.25, 0.5)[K % 3]
    want, margin = want_nms(aabb, order, cls, valid, thr, old_type, use_cls)
    assert margin > IOU_MARGIN
    if K > 1:
        assert (order != np.arange(K)).any(1).all()
        assert all(len(set(c)) >= 4 for c in cls)
        assert (2 * want.sum(1) < valid.sum(1)).all(), (want.sum(1), valid.sum(1))     # fewer than half survive
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    rc, keep = run_nms(hip, aabb, order, cls, valid, thr, old_type, use_cls)
    assert rc == 0
    np.testing.assert_array_equal(keep, want)


@pytest.mark.parametrize("K", [65, 256])
def test_nms3d_valid_none_and_valid_one(hip, K):
    rng = np.random.default_rng(K)
    B = 3
    aabb = np.stack([clustered_aabb(rng, K, 2) for _ in range(B)])
    order = np.stack([rng.permutation(K) for _ in range(B)])
    cls = rng.integers(0, 4, (B, K))
    valid = np.zeros((B, K), dtype=bool)
    rc, keep = run_nms(hip, aabb, order, cls, valid, 0.25, 0, 1)
    assert rc == 0 and not keep.any()
    one = rng.integers(0, K, B)
    valid[np.arange(B), one] = True                                  # a different single box per scene
    valid[1] = False                                                 # ... and none in the middle scene
    rc, keep = run_nms(hip, aabb, order, cls, valid, 0.25, 0, 1)
    assert rc == 0
    np.testing.assert_array_equal(keep, valid.astype(np.uint8))


@pytest.mark.parametrize("old_type", [0, 1])
def test_nms3d_zero_volume_boxes(hip, old_type):
    """0/0 is not above any threshold: coincident flat boxes keep each other, and a flat box neither suppresses nor is
    suppressed by a solid one under intersection over union"""
    flat = np.array([[0., 0, 0, 1, 1, 0]] * 3)
    mixed = np.array([[0., 0, 0, 1, 1, 1], [0., 0, 0, 1, 1, 0], [0., 0, 0, 1, 1, 0.9]])
    aabb = np.stack([flat, mixed, flat + 2.0])
    order = np.array([[0, 1, 2], [0, 1, 2], [2, 0, 1]])
    cls = np.zeros((3, 3), dtype=np.int64)
    valid = np.ones((3, 3), dtype=bool)
    want, _ = want_nms(aabb, order, cls, valid, 0.25, old_type, 1)
    np.testing.assert_array_equal(want, [[1, 1, 1], [1, 1, 0], [1, 1, 1]])
    rc, keep = run_nms(hip, aabb, order, cls, valid, 0.25, old_type, 1)
    assert rc == 0
    np.testing.assert_array_equal(keep, want)


def test_nms3d_overlap_exactly_on_the_threshold(hip):
    """[0,5] and [3,8] along x, unit y and z: 2 / (5 + 5 - 2) = 0.25 exactly.  Suppression needs overlap > nms_iou: at
    0.25 the second box stays, at the next float64 below it goes.  Integers only: exact on both sides."""
    below = np.nextafter(0.25, 0.0)
    pair = np.array([[0., 0, 0, 5, 1, 1], [3., 0, 0, 8, 1, 1]])
    aabb = np.stack([pair, pair[::-1], pair + 16.0])                 # the second scene holds the pair the other way
    order = np.array([[0, 1], [1, 0], [0, 1]])                       # ... and still picks [0,5] first
    cls = np.zeros((3, 2), dtype=np.int64)
    valid = np.ones((3, 2), dtype=bool)
    for thr, want in ((0.25, [[1, 1], [1, 1], [1, 1]]), (below, [[1, 0], [0, 1], [1, 0]])):
        for use_cls in (0, 1):
            w, margin = want_nms(aabb, order, cls, valid, thr, 0, use_cls)
            np.testing.assert_array_equal(w, want)
            assert margin == 0.25 - thr
            rc, keep = run_nms(hip, aabb, order, cls, valid, thr, 0, use_cls)
            assert rc == 0
            np.testing.assert_array_equal(keep, want)


def test_nms3d_old_type_divides_by_the_volume_of_the_box_it_may_drop(hip):
    """volumes 5 and 8, intersection 2.  Picking the small box first the overlap is 2/8 = 0.25 (the large one stays at
    nms_iou = 0.25, goes just below); picking the large one first it is 2/5 = 0.4.  With the denominators swapped the
    first scene drops a box at 0.25 and the second keeps both at 0.3."""
    below = np.nextafter(0.25, 0.0)
    pair = np.array([[0., 0, 0, 5, 1, 1], [3., 0, 0, 11, 1, 1]])
    aabb = np.stack([pair, pair])
    order = np.array([[0, 1], [1, 0]])
    cls = np.zeros((2, 2), dtype=np.int64)
    valid = np.ones((2, 2), dtype=bool)
    for thr, want in ((0.25, [[1, 1], [0, 1]]), (below, [[1, 0], [0, 1]]), (0.3, [[1, 1], [0, 1]]),
                      (0.4, [[1, 1], [1, 1]]), (np.nextafter(0.4, 0.0), [[1, 1], [0, 1]])):
        w, _ = want_nms(aabb, order, cls, valid, thr, 1, 1)
        np.testing.assert_array_equal(w, want)
        rc, keep = run_nms(hip, aabb, order, cls, valid, thr, 1, 1)
        assert rc == 0
        np.testing.assert_array_equal(keep, want)


def test_nms3d_refuses_more_than_1024_boxes(hip):
    K, B = 1025, 2
    rng = np.random.default_rng(0)
    aabb = np.stack([clustered_aabb(rng, K, 8) for _ in range(B)])
    order = np.stack([rng.permutation(K) for _ in range(B)])
    rc, keep = run_nms(hip, aabb, order, np.zeros((B, K), dtype=np.int64), np.ones((B, K), dtype=bool), 0.25, 0, 1,
                       keep_fill=7)
    assert rc != 0
    assert b"1024" in hip.lib().rfd_last_error_string()
    assert (keep == 7).all()
    with pytest.raises(hip.RfdHipError, match="1024"):
        hip.check(rc, "rfd_nms3d")


# -------------------------------------------------------------------------------------- rfd_points_in_boxes

def run_points_in_boxes(hip, pts, boxes):
    """pts (B,n,stride) float32, boxes (B,K,7) float64 -> counts (B,K)"""
    B, n, stride = pts.shape
    K = boxes.shape[1]
    p, b = dev(pts), dev(boxes)
    counts = torch.full((B, K), -1, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().rfd_points_in_boxes(B, K, n, stride, p.data_ptr(), b.data_ptr(), counts.data_ptr(),
                                            hip.current_stream()), "rfd_points_in_boxes")
    torch.cuda.synchronize()
    return counts.cpu().numpy()


def clear_of_faces(pts, box_corners_cam):
    """move the points within FACE_MARGIN of a face plane of any box of their scene out of every box (at most
    FACE_SHARE of them, or one point of a small case) and assert that none is left -> the restatement's counts (B,K)"""
    for b in range(len(pts)):
        _, dist = P.count_points(pts[b, :, :3], box_corners_cam[b])
        near = dist <= FACE_MARGIN
        assert near.sum() <= max(1, FACE_SHARE * near.size), near.sum()
        pts[b, near, :3] = FAR
    both = [P.count_points(pts[b, :, :3], box_corners_cam[b]) for b in range(len(pts))]
    assert min(d.min() for _, d in both) > FACE_MARGIN
    return np.stack([c for c, _ in both])


def full_circle_boxes(rng, B, K):
    """(B,K,7) boxes: headings over [-2 pi, 2 pi] with the exact multiples of pi/2 among them, extents of every
    combination of signs"""
    center = rng.uniform(-1, 1, (B, K, 3))
    signs = np.array(list(itertools.product((1, -1), repeat=3)), dtype=np.float64)
    size = rng.uniform(0.3, 2.5, (B, K, 3)) * signs[(np.arange(K) + np.arange(B)[:, None]) % 8]
    angle = rng.uniform(-2 * np.pi, 2 * np.pi, (B, K))
    angle[:, :9] = np.arange(-4, 5) * (np.pi / 2)
    angle[1] = angle[1, ::-1]
    return np.concatenate([center, size, angle[..., None]], -1)


@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 80000])
@pytest.mark.parametrize("stride", [3, 4, 6])
def test_points_in_boxes_counts_equal_the_hull_test(hip, n, stride):
    from rfdnet_amd.iscnet import fit
    B, K = 2, 24
    rng = np.random.default_rng(10 * n + stride)
    boxes = full_circle_boxes(rng, B, K)
    assert (boxes[..., 3:6] < 0).any(1).all() and (boxes[..., 3:6] > 0).all(2).any()
    # small cases: the points sit where the boxes are, so that the counts are not all zero
    pts = rng.uniform(-2, 2, (B, n, stride)).astype(np.float32) if n > 300 else \
        rng.uniform(-0.6, 0.6, (B, n, stride)).astype(np.float32)
    cam = P.corners(boxes[..., 0:3], boxes[..., 3:6], boxes[..., 6])
    want = clear_of_faces(pts, cam)
    assert want.sum() > 0 and not np.array_equal(want[0], want[1])
    if n >= 255:
        assert 2 * (want > 0).sum() > want.size
    got = run_points_in_boxes(hip, pts, boxes)
    np.testing.assert_array_equal(got, want)
    # the package's other in-box test (fit_mesh_to_scan works from the corners) sees the same boxes
    depth = torch.from_numpy(P.to_depth(cam))
    for b, k in itertools.product(range(B), range(K)):
        inside = fit.points_in_box(torch.from_numpy(pts[b, :, :3].astype(np.float64)), depth[b, k])
        assert int(inside.sum()) == got[b, k], (b, k)


def test_points_in_boxes_negative_length_box_of_the_reference(hip):
    """centre (0.1, -0.2, 0.3), size (-1.2, 0.8, 1.0), heading 0.7: the reference's hull test finds the points of the
    box of length +1.2 (tests/test_predictions_cpu.py: scipy agrees); `|u| <= l/2` with the signed l found none"""
    rng = np.random.default_rng(0)
    pts = rng.uniform(-2, 2, (1, 20000, 3)).astype(np.float32)
    boxes = np.array([[[0.1, -0.2, 0.3, -1.2, 0.8, 1.0, 0.7], [0.1, -0.2, 0.3, 1.2, 0.8, 1.0, 0.7],
                       [0.1, -0.2, 0.3, 1.2, -0.8, 1.0, 0.7], [0.1, -0.2, 0.3, -1.2, -0.8, -1.0, 0.7]]])
    want = clear_of_faces(pts, P.corners(boxes[..., 0:3], boxes[..., 3:6], boxes[..., 6]))
    assert want[0, 0] > 200 and (want == want[0, 0]).all()
    np.testing.assert_array_equal(run_points_in_boxes(hip, pts, boxes), want)


def four_and_five_scene(n=4096):
    """two scenes, boxes 0 and 1 far apart: scene 0 holds exactly 5 points in box 0 and 4 in box 1, scene 1 the other
    way round; every other point is outside both"""
    rng = np.random.default_rng(45)
    boxes = np.array([[[-2.0, 0.5, 0.4, 0.9, 0.7, 0.8, 0.3], [2.0, -0.5, 0.6, 0.8, -1.1, 0.6, 2.0]]] * 2)
    pts = np.empty((2, n, 4), dtype=np.float32)
    pts[..., 0] = rng.uniform(-0.5, 0.5, (2, n))                     # a slab between the two boxes
    pts[..., 1:] = rng.uniform(-3, 3, (2, n, 3))
    for b, (n0, n1) in enumerate(((5, 4), (4, 5))):
        at = rng.permutation(n)[:n0 + n1]
        pts[b, at[:n0], :3] = boxes[b, 0, :3] + rng.uniform(-0.15, 0.15, (n0, 3))
        pts[b, at[n0:], :3] = boxes[b, 1, :3] + rng.uniform(-0.15, 0.15, (n1, 3))
    return boxes, pts


def test_points_in_boxes_exactly_four_and_exactly_five(hip):
    boxes, pts = four_and_five_scene()
    want = clear_of_faces(pts, P.corners(boxes[..., 0:3], boxes[..., 3:6], boxes[..., 6]))
    np.testing.assert_array_equal(want, [[5, 4], [4, 5]])
    np.testing.assert_array_equal(run_points_in_boxes(hip, pts, boxes), want)


# ------------------------------------------------------------------------ predictions.parse_predictions

def crafted_scenes(seed=21, B=2, K=256, n=20000):
    """head outputs over all 12 heading bins, 8 size classes and 5 semantic classes; centres in clusters so that NMS
    suppresses many boxes, one cluster outside the scan (empty boxes) and a few boxes of negative extent; objectness
    logits well apart (ranks and the 0.5 threshold cannot depend on float32 rounding of the softmax)"""
    rng = np.random.default_rng(seed)
    ep = all_bins_end_points(rng, B, K, MEAN_SIZES, n_sem=5)
    cc = np.concatenate([rng.uniform([-2, -2, 0.3], [2, 2, 1.2], (11, 3)), [[0.0, 0.0, 6.0]]])
    which = rng.integers(0, len(cc), (B, K))
    which[:, :6] = np.arange(6)                                      # the boxes of negative extent lie in the scan
    ep['center'] = (cc[which] + rng.uniform(-0.12, 0.12, (B, K, 3))).astype(np.float32)
    ep['size_residuals_normalized'] *= 0.5
    ep['size_residuals_normalized'][:, :6] = rng.uniform(-2.4, -2.0, (B, 6, 8, 3)).astype(np.float32)
    ep['size_residuals_normalized'][:, 3:6, :, 1:] *= -0.1
    logit = np.stack([rng.permutation(np.linspace(-4, 4, K)) for _ in range(B)])
    ep['objectness_scores'] = np.stack([-logit / 2, logit / 2], -1).astype(np.float32)
    pc = np.concatenate([rng.uniform([-2.6, -2.6, -0.2], [2.6, 2.6, 1.8], (B, n, 3)),
                         rng.uniform(0, 1, (B, n, 1))], -1).astype(np.float32)
    return ep, pc


def clear_scene_of_faces(ep, pc):
    center, size, angle = P.decode_boxes(ep, MEAN_SIZES)
    return clear_of_faces(pc, P.corners(center, size, angle))


def to_device(ep):
    return {k: dev(v) for k, v in ep.items()}


@pytest.fixture(scope="module")
def crafted(hip):
    ep, pc = crafted_scenes()
    counts = clear_scene_of_faces(ep, pc)
    return ep, pc, counts


def test_crafted_scenes_cover_what_they_claim(crafted):
    ep, pc, counts = crafted
    center, size, angle = P.decode_boxes(ep, MEAN_SIZES)
    for b in range(2):
        assert set(ep['heading_scores'][b].argmax(-1)) == set(range(12))
        assert set(ep['size_scores'][b].argmax(-1)) == set(range(8))
        assert set(ep['sem_cls_scores'][b].argmax(-1)) == set(range(5))
        assert (size[b] < 0).any(1).sum() >= 6 and (size[b] < 0).all(1).any()
        assert (angle[b] < -1).any() and (angle[b] > 1).any()
        assert 10 <= (counts[b] < 5).sum() <= 60 and (counts[b][:6] >= 5).all()
        prob = np.sort(P.softmax(ep['objectness_scores'][b])[:, 1])
        assert np.diff(prob).min() > 1e-5 and np.abs(prob - 0.5).min() > 1e-5


@pytest.mark.parametrize("nms_iou", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("tag,cfg", [("default", {}), ("nocls", {'cls_nms': False}),
                                     ("old", {'use_old_type_nms': True}),
                                     ("keepempty", {'remove_empty_box': False})])
def test_parse_predictions_two_crafted_scenes(hip, crafted, tag, cfg, nms_iou):
    """pred_mask, points_in_box and the proposal ids equal the restatement's; corners to 1e-9 (coordinates stay below
    16 m, where one float64 ulp is 3.6e-15, and a corner is a dozen operations after cos / sin)"""
    from rfdnet_amd.iscnet import predictions
    from rfdnet_amd.iscnet.config import ScannetConfig
    ep, pc, counts = crafted
    cfg = dict(cfg, nms_iou=nms_iou)
    want = P.parse_predictions(ep, pc, MEAN_SIZES, cfg)
    assert want['iou_margin'] > IOU_MARGIN
    valid = counts >= 5 if cfg.get('remove_empty_box', True) else np.ones_like(counts, dtype=bool)
    assert (valid.sum(1) - want['pred_mask'].sum(1) >= 40).all()               # NMS has suppressed many
    assert np.abs(want['corners']).max() < 16
    dep = to_device(ep)
    eval_dict, parsed = predictions.parse_predictions(dep, dev(pc), ScannetConfig(MEAN_SIZES), cfg)
    np.testing.assert_array_equal(eval_dict['pred_mask'].cpu().numpy(), want['pred_mask'])
    if cfg.get('remove_empty_box', True):
        np.testing.assert_array_equal(want['points_in_box'], counts)
        np.testing.assert_array_equal(parsed['points_in_box'].cpu().numpy(), counts)
    else:
        assert parsed['points_in_box'] is None
    np.testing.assert_allclose(parsed['pred_corners_3d_upright_camera'].cpu().numpy(), want['corners'],
                               rtol=0, atol=1e-9)
    np.testing.assert_array_equal(parsed['pred_sem_cls'].cpu().numpy(), want['pred_sem_cls'])
    np.testing.assert_array_equal(parsed['box_params'].cpu().numpy()[..., :6], want['box_params'][..., :6])
    np.testing.assert_allclose(parsed['box_params'].cpu().numpy()[..., 6], want['box_params'][..., 6],
                               rtol=0, atol=1e-15)
    for b in range(2):
        one = {k: v[b:b + 1] for k, v in dep.items()}
        ids = predictions.get_proposal_id(one, eval_dict['pred_mask'][b:b + 1], 0.5)
        want_ids = P.proposal_ids(ep['objectness_scores'][b], want['pred_mask'][b], 0.5)
        assert ids.shape == (1, len(want_ids), 1) and 0 < len(want_ids) <= want['pred_mask'][b].sum()
        np.testing.assert_array_equal(ids.cpu().numpy()[0, :, 0], want_ids)


def test_parse_predictions_keeps_a_box_of_five_points_and_drops_one_of_four(hip):
    """ap_helper.py:196: a box is empty with fewer than 5 points"""
    from rfdnet_amd.iscnet import predictions
    from rfdnet_amd.iscnet.config import ScannetConfig
    boxes, pts = four_and_five_scene()
    mean = np.abs(boxes[0, :, 3:6])                                  # two size classes: the two boxes themselves
    mean = np.concatenate([mean, np.ones((6, 3))])
    B, K = 2, 2
    ep = {'center': boxes[..., :3].astype(np.float32),
          'heading_scores': np.zeros((B, K, 12), dtype=np.float32),
          'heading_residuals_normalized': np.zeros((B, K, 12), dtype=np.float32),
          'size_scores': np.zeros((B, K, 8), dtype=np.float32),
          'size_residuals_normalized': np.zeros((B, K, 8, 3), dtype=np.float32),
          'sem_cls_scores': np.zeros((B, K, 8), dtype=np.float32),
          'objectness_scores': np.array([[[0, 1], [0, 2]]] * 2, dtype=np.float32)}
    ep['size_scores'][:, 1, 1] = 1.0
    ep['heading_scores'][:, 1, 4] = 1.0                              # bin 4 is 2 pi / 3
    ep['heading_residuals_normalized'][:, 0, 0] = 0.5
    center, size, angle = P.decode_boxes(ep, mean)
    counts = clear_of_faces(pts, P.corners(center, size, angle))
    np.testing.assert_array_equal(counts, [[5, 4], [4, 5]])
    want = P.parse_predictions(ep, pts, mean)
    np.testing.assert_array_equal(want['pred_mask'], [[1, 0], [0, 1]])
    eval_dict, parsed = predictions.parse_predictions(to_device(ep), dev(pts), ScannetConfig(mean))
    np.testing.assert_array_equal(parsed['points_in_box'].cpu().numpy(), counts)
    np.testing.assert_array_equal(eval_dict['pred_mask'].cpu().numpy(), want['pred_mask'])


def test_parse_predictions_scene_without_a_box_of_five_points(hip, crafted):
    """the reference stops on `assert len(pick) > 0` (ap_helper.py:256); this package returns an empty selection"""
    from rfdnet_amd.iscnet import predictions
    from rfdnet_amd.iscnet.config import ScannetConfig
    ep, pc, _ = crafted
    away = pc.copy()
    away[1, :, 2] += 40.0                                            # the second scene's scan misses every box
    away[1, :4, :3] = ep['center'][1, 10]                            # ... but for 4 points in the middle of one
    want = P.parse_predictions(ep, away, MEAN_SIZES)
    assert want['points_in_box'][1].max() == 4 and want['pred_mask'][0].any() and not want['pred_mask'][1].any()
    dep = to_device(ep)
    eval_dict, parsed = predictions.parse_predictions(dep, dev(away), ScannetConfig(MEAN_SIZES))
    np.testing.assert_array_equal(eval_dict['pred_mask'].cpu().numpy(), want['pred_mask'])
    assert parsed['points_in_box'][1].max() == 4
    ids = predictions.get_proposal_id({k: v[1:2] for k, v in dep.items()}, eval_dict['pred_mask'][1:2], 0.5)
    assert ids.shape == (1, 0, 1) and ids.dtype == torch.int64


def test_generate_with_reference_selection_returns_no_meshes_for_an_empty_selection(hip, golden_dir):
    """ISCNet.generate(selection='nms') on a scene whose boxes hold no scan points: no meshes, no exception"""
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    cfg = Config({'generation': {'resolution_0': 8, 'upsampling_steps': 1}}, mean_size_arr=MEAN_SIZES)
    net = ISCNet(cfg)
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=3, n_raw=9000, n_points=8192)[None]).cuda()
    detect = net.detect

    def detect_boxes_off_the_scan(point_clouds):
        ep, pf = detect(point_clouds)
        ep['center'] = ep['center'] + 50.0
        return ep, pf
    net.detect = detect_boxes_off_the_scan
    end_points, ids, meshes = net.generate({'point_clouds': pc}, selection='nms')
    assert int(end_points['parsed_predictions']['points_in_box'].max()) == 0
    assert not end_points['pred_mask'].any() and end_points['pred_mask'].shape == (1, 256)
    assert ids.shape == (1, 0, 1) and meshes == []
