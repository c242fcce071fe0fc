"""float64 restatement of the stage between detection and completion (rfdnet_amd/iscnet/predictions.py on top of
csrc/boxes.hip) in plain numpy: the ground truth of tests/test_predictions_cpu.py and tests/test_gpu_postprocess.py.

Written from the description of the algorithm (net_utils/ap_helper.py:131-264 parse_predictions, box_util.py:183-198
get_3d_box, libs.py:98-137, nms.py:79-118, demo.py:50-75), one scene at a time, with the premises a test needs to state
returned next to the results: every point's distance to the nearest face plane of a box, and the smallest |IoU - thr|
the greedy pick compared.  tests/test_predictions_cpu.py ties it to the reference's own run (tests/golden/F_NMS.npz) and
to scipy's Delaunay hull test.
"""
import numpy as np

DEFAULT_EVAL_CONFIG = {'remove_empty_box': True, 'nms_iou': 0.25, 'use_old_type_nms': False, 'cls_nms': True}
NUM_HEADING_BIN = 12
MIN_POINTS = 5              # ap_helper.py:196: a box with fewer scan points is empty

# get_3d_box's corner order: signs of (l/2, h/2, w/2) along the box's own x, y (up), z in the upright camera frame
_SX = np.array([1, 1, -1, -1, 1, 1, -1, -1], dtype=np.float64)
_SY = np.array([1, 1, 1, 1, -1, -1, -1, -1], dtype=np.float64)
_SZ = np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.float64)


def decode_boxes(end_points, mean_size_arr, num_heading_bin=NUM_HEADING_BIN):
    """head outputs (numpy, (B,K,...)) -> centre (B,K,3), size (B,K,3) [l,w,h], angle (B,K), float64.  The two residual
    products are float32 like the reference's tensors; the sums, and the wrap of angles above pi, are float64."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    mean = np.asarray(mean_size_arr, dtype=np.float64)
    center = f32(end_points['center']).astype(np.float64)
    hcls = np.argmax(end_points['heading_scores'], -1)
    hres = f32(end_points['heading_residuals_normalized']) * np.float32(np.pi / num_heading_bin)
    hres = np.take_along_axis(hres, hcls[..., None], 2)[..., 0]
    assert hres.dtype == np.float32
    angle = hcls.astype(np.float64) * (2 * np.pi / float(num_heading_bin)) + hres.astype(np.float64)
    angle = np.where(angle > np.pi, angle - 2 * np.pi, angle)
    scls = np.argmax(end_points['size_scores'], -1)
    sres = f32(end_points['size_residuals_normalized']) * mean.astype(np.float32)[None, None]
    sres = np.take_along_axis(sres, scls[..., None, None], 2)[:, :, 0]
    assert sres.dtype == np.float32
    size = mean[scls] + sres.astype(np.float64)
    return center, size, angle


def to_camera(p):
    """depth (x, y, z) -> upright camera (x, -z, y)"""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([p[..., 0], -p[..., 2], p[..., 1]], -1)


def to_depth(p):
    """upright camera (x, y, z) -> depth (x, z, -y)"""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)


def corners(center, size, angle):
    """centre (...,3) in the depth frame, size (...,3) [l,w,h], heading (...) -> (...,8,3) corners in the upright camera
    frame: the box is turned by -heading about the camera's y (up) axis, roty(t) = [[c,0,s],[0,1,0],[-s,0,c]]."""
    center, size, angle = (np.asarray(a, dtype=np.float64) for a in (center, size, angle))
    c, s = np.cos(-angle)[..., None], np.sin(-angle)[..., None]
    xc = size[..., 0:1] / 2 * _SX
    yc = size[..., 2:3] / 2 * _SY
    zc = size[..., 1:2] / 2 * _SZ
    cam = to_camera(center)
    return np.stack([c * xc + s * zc + cam[..., 0:1], yc + cam[..., 1:2], -s * xc + c * zc + cam[..., 2:3]], -1)


def points_in_hull(points, box_corners):
    """points (N,3), box_corners (8,3) in get_3d_box order, same frame -> (inside (N) bool, dist (N)).

    The convex hull of the eight corners of a box is the box.  Corner 2 is taken as the origin and the three edges that
    leave it (to corners 1, 3 and 6) as axes: a point is inside when its projection on every edge lies within the edge.
    Only the corners enter, so a box decoded with a negative extent (its corners in another order) is the same box.
    dist is the distance to the nearest of the six face planes -- never more than the distance to the nearest face."""
    p = np.asarray(points, dtype=np.float64)
    cr = np.asarray(box_corners, dtype=np.float64)
    o = cr[2]
    edges = np.stack([cr[1] - o, cr[3] - o, cr[6] - o])            # (3,3)
    length = np.sqrt((edges * edges).sum(1))
    assert (length > 0).all(), "degenerate box"
    t = (p - o) @ (edges / length[:, None]).T                       # (N,3) metres along each edge
    inside = ((t >= 0) & (t <= length)).all(1)
    dist = np.minimum(np.abs(t), np.abs(t - length)).min(1)
    return inside, dist


def count_points(points, box_corners_cam):
    """points (N,3) depth frame, box_corners_cam (K,8,3) -> (counts (K) int64, dist (N): nearest face plane of any box)"""
    counts = np.zeros(len(box_corners_cam), dtype=np.int64)
    dist = np.full(len(points), np.inf)
    for k, cr in enumerate(box_corners_cam):
        inside, d = points_in_hull(points, to_depth(cr))
        counts[k] = inside.sum()
        dist = np.minimum(dist, d)
    return counts, dist


def score_order(score):
    """box indices by descending score; among equal scores the higher index first (a stable ascending sort, read from
    its end)"""
    return np.argsort(np.asarray(score), kind='stable')[::-1].copy()


def nms3d(aabb, order, cls, valid, thr, old_type=False, use_cls=True):
    """Greedy suppression over axis-aligned boxes.  aabb (K,6) [x1,y1,z1,x2,y2,z2]; order (K): the boxes by descending
    score; cls (K); valid (K): boxes that take part.  The best box still alive is kept; every other box alive whose
    overlap with it is STRICTLY above thr is dropped.  Overlap: intersection over union, or with old_type intersection
    over the volume of the box that may be dropped; with use_cls, 0 between boxes of different classes.  0/0 (two
    zero-volume boxes) is not a number and does not suppress.
    -> (keep (K) uint8, the smallest |overlap - thr| over all pairs compared (inf if none))"""
    aabb = np.asarray(aabb, dtype=np.float64)
    cls = np.asarray(cls)
    alive = np.asarray(valid).astype(bool).copy()
    keep = np.zeros(len(aabb), dtype=np.uint8)
    vol = (aabb[:, 3] - aabb[:, 0]) * (aabb[:, 4] - aabb[:, 1]) * (aabb[:, 5] - aabb[:, 2])
    margin = np.inf
    for i in np.asarray(order):
        if not alive[i]:
            continue
        keep[i] = 1
        alive[i] = False
        js = np.nonzero(alive)[0]
        if js.size == 0:
            break
        ext = np.maximum(0.0, np.minimum(aabb[i, 3:], aabb[js, 3:]) - np.maximum(aabb[i, :3], aabb[js, :3]))
        inter = ext[:, 0] * ext[:, 1] * ext[:, 2]
        with np.errstate(invalid='ignore', divide='ignore'):
            o = inter / vol[js] if old_type else inter / (vol[i] + vol[js] - inter)
        if use_cls:
            o = np.where(cls[js] == cls[i], o, 0.0)
        num = ~np.isnan(o)
        if num.any():
            margin = min(margin, float(np.abs(o[num] - thr).min()))
        alive[js[o > thr]] = False
    return keep, margin


def softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def parse_predictions(end_points, point_clouds, mean_size_arr, config=None):
    """end_points: numpy head outputs (B,K,...); point_clouds (B,N,3+) -> dict of
    pred_mask (B,K) uint8, points_in_box (B,K) int64 (None without remove_empty_box), corners (B,K,8,3), box_params
    (B,K,7), obj_prob (B,K), pred_sem_cls (B,K), iou_margin (smallest |overlap - nms_iou| compared in any scene),
    face_dist (B,N): every point's distance to the nearest face plane of any box of its scene."""
    cfg = dict(DEFAULT_EVAL_CONFIG)
    cfg.update(config or {})
    center, size, angle = decode_boxes(end_points, mean_size_arr)
    cr = corners(center, size, angle)
    B, K = angle.shape
    sem = np.argmax(end_points['sem_cls_scores'], -1)
    obj_prob = softmax(end_points['objectness_scores'])[..., 1]
    pts = np.asarray(point_clouds)[:, :, :3].astype(np.float64)
    counts, face_dist = None, None
    valid = np.ones((B, K), dtype=bool)
    if cfg['remove_empty_box']:
        both = [count_points(pts[b], cr[b]) for b in range(B)]
        counts = np.stack([c for c, _ in both])
        face_dist = np.stack([d for _, d in both])
        valid = counts >= MIN_POINTS
    aabb = np.concatenate([cr.min(2), cr.max(2)], -1)
    mask = np.zeros((B, K), dtype=np.uint8)
    margin = np.inf
    for b in range(B):
        mask[b], m = nms3d(aabb[b], score_order(obj_prob[b]), sem[b], valid[b], cfg['nms_iou'],
                           cfg['use_old_type_nms'], cfg['cls_nms'])
        margin = min(margin, m)
    return {'pred_mask': mask, 'points_in_box': counts, 'corners': cr, 'obj_prob': obj_prob, 'pred_sem_cls': sem,
            'box_params': np.concatenate([center, size, angle[..., None]], -1), 'iou_margin': margin,
            'face_dist': face_dist}


def proposal_ids(objectness_scores, pred_mask, conf_thresh):
    """one scene: objectness_scores (K,2), pred_mask (K) -> ids of the proposals above the threshold that survived"""
    prob = softmax(objectness_scores)[..., 1]
    return np.nonzero((prob > conf_thresh) & (np.asarray(pred_mask) != 0))[0]


# ------------------------------------------------------------------------------- inputs the tests share

def clustered_aabb(rng, K, n_clusters, flat_share=0.0, jitter=0.15, half=(0.35, 0.65)):
    """K boxes of about unit size around n_clusters centres: boxes of one cluster overlap heavily"""
    cc = rng.uniform(-4, 4, (n_clusters, 3))
    c = cc[rng.integers(0, n_clusters, K)] + rng.uniform(-jitter, jitter, (K, 3))
    half = rng.uniform(half[0], half[1], (K, 3))
    flat = rng.random(K) < flat_share
    half[flat, rng.integers(0, 3, int(flat.sum()))] = 0.0           # zero-volume boxes
    return np.concatenate([c - half, c + half], 1)


def all_bins_end_points(rng, B, K, mean_size_arr, n_sem=8):
    """head outputs whose decoded boxes run over every heading bin with residuals of both signs (bin 6 lands on both
    sides of pi) and over every size class"""
    nh, ns = NUM_HEADING_BIN, len(mean_size_arr)
    hcls = np.stack([rng.permutation(K) % nh for _ in range(B)])
    scls = np.stack([rng.permutation(K) % ns for _ in range(B)])
    sem = np.stack([rng.permutation(K) % n_sem for _ in range(B)])

    def scores(c, n):
        s = rng.normal(0, 1, (B, K, n)).astype(np.float32)
        np.put_along_axis(s, c[..., None], 5.0, 2)
        return s
    return {'center': rng.uniform(-2, 2, (B, K, 3)).astype(np.float32),
            'heading_scores': scores(hcls, nh),
            'heading_residuals_normalized': rng.uniform(-1, 1, (B, K, nh)).astype(np.float32),
            'size_scores': scores(scls, ns),
            'size_residuals_normalized': rng.uniform(-0.6, 0.6, (B, K, ns, 3)).astype(np.float32),
            'sem_cls_scores': scores(sem, 8),
            'objectness_scores': rng.normal(0, 2, (B, K, 2)).astype(np.float32)}


MEAN_SIZES = np.array([[0.76, 1.41, 0.80], [1.87, 1.96, 0.93], [0.61, 0.63, 0.71], [1.40, 1.54, 0.75],
                       [0.79, 1.32, 1.01], [0.59, 0.55, 0.87], [1.06, 1.61, 0.72], [0.53, 0.48, 0.41]]) + 1e-3 / 3
