"""Deterministic, torch-version-independent synthetic weights and scenes
(stand-ins for the absent pretrained weights and ScanNet scans).

torch's RNG is not stable across versions/devices, so every synthetic tensor
used by fixtures, tests and bench comes from numpy's PCG64 (`default_rng`),
which is specified bit-for-bit.  Shared by tests/golden/make_fixtures.py (dev
container, with the reference importable) and the tests themselves (anywhere).
"""
from collections import OrderedDict

import numpy as np


def seeded_tensor(name, shape, rng):
    """Value rule by parameter name (BN running_mean~N(0,0.1),
    running_var~U(0.5,1.5), conv weights uniform(+-1/sqrt(fan_in)), CBN
    gamma/beta convs N(0,0.02) so the conditioning path is exercised -- the
    reference zero-initialises them, layers.py:220-224)."""
    shape = tuple(int(s) for s in shape)
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    if name.endswith("running_var"):
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if name.endswith("running_mean"):
        return rng.normal(0.0, 0.1, shape).astype(np.float32)
    if "conv_gamma.weight" in name or "conv_beta.weight" in name:
        return rng.normal(0.0, 0.02, shape).astype(np.float32)
    if "conv_gamma.bias" in name:
        return (1.0 + rng.normal(0.0, 0.1, shape)).astype(np.float32)
    if name.endswith(".weight") and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        b = 1.0 / np.sqrt(fan_in)
        return rng.uniform(-b, b, shape).astype(np.float32)
    if name.endswith(".weight"):          # affine BN scale
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if name.endswith(".bias"):
        return rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    raise KeyError("no seeding rule for %s" % name)


def seeded_state_dict(shapes, seed):
    """shapes: ordered {name: shape}.  Returns ordered {name: ndarray}."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for k, s in shapes.items():
        out[k] = seeded_tensor(k, s, rng)
    return out


def load_seeded(module, seed):
    """Overwrite every parameter/buffer of a torch module from the seed.
    Returns the ordered {name: shape} map (for key-parity checks)."""
    import torch
    sd = module.state_dict()
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in sd.items())
    new = seeded_state_dict(shapes, seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
    return shapes


def synthetic_scene(seed=10, n_raw=120000, n_points=80000, with_origin_pts=True, return_boxes=False):
    """ScanNet-like room: 6x7x2.8 m, floor + 4 walls + 12
    cuboid 'furniture' surfaces, sigma=5 mm noise, 16 points within 0.02 m of
    the origin (exercise the FPS |p|^2 <= 1e-3 skip), height channel =
    z - percentile(z, 0.99) (demo.py:38-40), random subsample to n_points
    (with replacement when n_raw < n_points, pc_util.py:35-47).
    Returns (n_points, 4) float32; with return_boxes also the 12 furniture cuboids as (12, 7) float64 [centre xyz,
    size lwh, heading] in the scan's frame (the layout of parse_predictions' box_params) and a class id per box
    (12,) int64 -- ground truth for an evaluation sweep.  The random stream and the points do not depend on the flag."""
    rng = np.random.default_rng(seed)
    W, L, Hh = 6.0, 7.0, 2.8
    parts = []

    def plane(n, o, u, v):
        a = rng.random((n, 1))
        b = rng.random((n, 1))
        return np.asarray(o)[None] + a * np.asarray(u)[None] + b * np.asarray(v)[None]

    n_floor = int(n_raw * 0.30)
    n_wall = int(n_raw * 0.08)
    parts.append(plane(n_floor, (-W / 2, -L / 2, 0), (W, 0, 0), (0, L, 0)))
    parts.append(plane(n_wall, (-W / 2, -L / 2, 0), (W, 0, 0), (0, 0, Hh)))
    parts.append(plane(n_wall, (-W / 2, L / 2, 0), (W, 0, 0), (0, 0, Hh)))
    parts.append(plane(n_wall, (-W / 2, -L / 2, 0), (0, L, 0), (0, 0, Hh)))
    parts.append(plane(n_wall, (W / 2, -L / 2, 0), (0, L, 0), (0, 0, Hh)))
    n_left = n_raw - n_floor - 4 * n_wall - (16 if with_origin_pts else 0)
    n_obj = 12
    per = n_left // n_obj
    boxes = np.zeros((n_obj, 7))
    for i in range(n_obj):
        size = rng.uniform(0.4, 1.6, 3) * np.array([1.0, 1.0, 0.7])
        ctr = np.array([rng.uniform(-W / 2 + 0.8, W / 2 - 0.8),
                        rng.uniform(-L / 2 + 0.8, L / 2 - 0.8), size[2] / 2])
        ang = rng.uniform(0, np.pi)
        boxes[i] = np.concatenate([ctr, size, [ang]])
        n_i = per if i < n_obj - 1 else n_left - per * (n_obj - 1)
        face = rng.integers(0, 5, n_i)          # 4 sides + top
        uv = rng.random((n_i, 2)) - 0.5
        p = np.zeros((n_i, 3))
        for f in range(5):
            m = face == f
            if f == 4:
                p[m] = np.stack([uv[m, 0] * size[0], uv[m, 1] * size[1],
                                 np.full(m.sum(), size[2] / 2)], 1)
            elif f < 2:
                p[m] = np.stack([np.full(m.sum(), (f - 0.5) * size[0]),
                                 uv[m, 0] * size[1], uv[m, 1] * size[2]], 1)
            else:
                p[m] = np.stack([uv[m, 0] * size[0],
                                 np.full(m.sum(), (f - 2.5) * size[1]),
                                 uv[m, 1] * size[2]], 1)
        c, s = np.cos(ang), np.sin(ang)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        parts.append(p @ R.T + ctr[None])
    pts = np.concatenate(parts, 0)
    pts = pts + rng.normal(0, 0.005, pts.shape)
    if with_origin_pts:
        pts = np.concatenate([pts, rng.uniform(-0.0115, 0.0115, (16, 3))], 0)
    pts = pts.astype(np.float32)
    floor_h = np.percentile(pts[:, 2], 0.99)
    height = (pts[:, 2] - floor_h).astype(np.float32)
    pc = np.concatenate([pts, height[:, None]], 1).astype(np.float32)
    replace = pc.shape[0] < n_points
    choice = rng.choice(pc.shape[0], n_points, replace=replace)
    if return_boxes:
        return np.ascontiguousarray(pc[choice]), boxes, np.arange(n_obj, dtype=np.int64) % 8
    return np.ascontiguousarray(pc[choice])


def object_occupancy(boxes, n_points=2048, seed=11, fill=0.9):
    """Per-object completion ground truth for the cuboids `boxes` (G, 7) of synthetic_scene(return_boxes=True), in the
    layout the reference's test loader gives ISCNet (object_points, object_points_occ, object_voxels):
    points (G, n_points, 3) float32 uniform in the unit cube [-0.5, 0.5]^3, their occupancies (G, n_points) float32 (1
    inside) and voxels (G, 16, 16, 16) float32 sampled at the centres of the 16^3 lattice of ONet.compute_loss
    (-0.5 + 1/32 ... 0.5 - 1/32, x slowest).  The inside of object g is the ellipsoid with semi-axes
    fill / 2 * size_g / max(size_g): the box's proportions, scaled so that its longest side spans `fill` of the cube."""
    boxes = np.asarray(boxes, dtype=np.float64)
    rng = np.random.default_rng(seed)
    G = boxes.shape[0]
    axes = 0.5 * fill * boxes[:, 3:6] / boxes[:, 3:6].max(axis=1, keepdims=True)            # (G, 3)
    pts = rng.random((G, n_points, 3)) - 0.5
    inside = lambda q: ((q / axes[:, None, :]) ** 2).sum(-1) <= 1.0
    lin = np.linspace(-0.5 + 1 / 32, 0.5 - 1 / 32, 16)
    lattice = np.stack(np.meshgrid(lin, lin, lin, indexing='ij'), axis=-1).reshape(1, -1, 3)
    voxels = inside(np.broadcast_to(lattice, (G, 4096, 3))).reshape(G, 16, 16, 16)
    return pts.astype(np.float32), inside(pts).astype(np.float32), voxels.astype(np.float32)


def scene_labels(pc, boxes, cls, G=64, mean_size_arr=None, margin=0.02):
    """The dataloader-shaped label dictionary (numpy, batch of one) of a synthetic_scene(return_boxes=True) scene: what
    ISCNet.evaluate(losses=True) reads beside the point cloud.  Box g fills label row g of G; the padded rows are zero.
      center_label (1,G,3) f32, heading_class_label / size_class_label / sem_cls_label (1,G) int64,
      heading_residual_label (1,G) f32, size_residual_label (1,G,3) f32, box_label_mask (1,G) f32:
        ScanNet's angle2class (12 bins) and size2class (one size cluster per class, residual = size - mean size);
      vote_label (1,N,9) f32, vote_label_mask (1,N) int64: a point within `margin` of a cuboid votes for its centre
        (centre - point, three copies); a point in several cuboids votes for the first;
      point_instance_labels (1,N) int64, object_instance_labels (1,G) int64: instance id = row + 1, 0 = no object."""
    pc = np.asarray(pc)
    boxes = np.asarray(boxes, dtype=np.float64)
    cls = np.asarray(cls, dtype=np.int64)
    n = boxes.shape[0]
    assert n <= G and pc.ndim == 2
    if mean_size_arr is None:
        mean_size_arr = np.full((8, 3), 0.8)
    mean_size_arr = np.asarray(mean_size_arr, dtype=np.float64)
    N = pc.shape[0]
    out = {'center_label': np.zeros((1, G, 3), np.float32), 'heading_class_label': np.zeros((1, G), np.int64),
           'heading_residual_label': np.zeros((1, G), np.float32), 'size_class_label': np.zeros((1, G), np.int64),
           'size_residual_label': np.zeros((1, G, 3), np.float32), 'sem_cls_label': np.zeros((1, G), np.int64),
           'box_label_mask': np.zeros((1, G), np.float32), 'vote_label': np.zeros((1, N, 9), np.float32),
           'vote_label_mask': np.zeros((1, N), np.int64), 'point_instance_labels': np.zeros((1, N), np.int64),
           'object_instance_labels': np.zeros((1, G), np.int64)}
    per_bin = 2 * np.pi / 12
    shifted = (boxes[:, 6] % (2 * np.pi) + per_bin / 2) % (2 * np.pi)
    hcls = (shifted / per_bin).astype(np.int64)
    out['center_label'][0, :n] = boxes[:, :3]
    out['heading_class_label'][0, :n] = hcls
    out['heading_residual_label'][0, :n] = shifted - (hcls * per_bin + per_bin / 2)
    out['size_class_label'][0, :n] = cls
    out['size_residual_label'][0, :n] = boxes[:, 3:6] - mean_size_arr[cls]
    out['sem_cls_label'][0, :n] = cls
    out['box_label_mask'][0, :n] = 1
    out['object_instance_labels'][0, :n] = np.arange(1, n + 1)
    xyz = pc[:, :3].astype(np.float64)
    for g in range(n - 1, -1, -1):                                         # the first cuboid is written last: it wins
        c, s = np.cos(boxes[g, 6]), np.sin(boxes[g, 6])
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        local = (xyz - boxes[g, :3]) @ R
        inside = (np.abs(local) <= boxes[g, 3:6] / 2 + margin).all(1)
        out['vote_label'][0, inside] = np.tile(boxes[g, :3] - xyz[inside], (1, 3))
        out['vote_label_mask'][0, inside] = 1
        out['point_instance_labels'][0, inside] = g + 1
    return out
