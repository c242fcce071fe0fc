"""Scan ground truth on the device: from a scan with instance ids and aligned CAD models to the label batch that
ISCNet.evaluate and the losses read.  Two stages of the reference:

  prepare_scan   utils/scannet/gen_scannet_w_orientation.py's generate(): instance boxes (load_scannet_data.export),
                 one upright yawed box per CAD model, the instance each box belongs to, the votes of every vertex
                 -> the contents of bbox.pkl and full_scan.npz, and the sizes that feed the class means
  make_sample    models/iscnet/dataloader.py, ISCNet_ScanNet.__getitem__: the sampled point cloud with colour and
                 height, flips and the z-rotation, the 64-row label arrays, and the completion keys

The kernels are csrc/scan_labels.hip; their rules are written out in include/rfd_labels.h and restated in numpy in
tests/scan_labels_f64.py; tests/golden/F_SCAN.npz is the reference's own output.  What runs on the device is what
grows with the scan (vertices x boxes) or with the CAD meshes; the per-model 4x4 algebra, the axis rectification and
the 64-row label arrays are small float64 host math.  The GPU guard is _lib.need_gpu, offsets come from ragged.
Not here: export's segment and aggregation JSON readers (the instance ids come in as an array) and a multi-worker
DataLoader.
"""
import os

import numpy as np
import torch

from . import _lib, ragged

MAX_NUM_OBJ = 64
MEAN_COLOR_RGB = np.array([121.87661, 109.73591, 95.61673])
# ShapeNet synset -> the reference's class id (the position in its class list), for the eight classes of
# ScanNet_OBJ_CLASS_IDS: table, chair, bookshelf, sofa, trash bin, cabinet, display, bathtub.  Every other synset is
# outside the filter.
OBJ_CLASS_IDS = (1, 7, 8, 13, 20, 31, 34, 43)
SYNSET_CLASS = {'04379243': 1, '03001627': 7, '02871439': 8, '04256520': 13, '02747177': 20, '02933112': 31,
                '03211117': 34, '02808440': 43}
EXTENT_STEP = 2048               # vertices per workgroup of rfd_labels_cad_extents


# ---- small host algebra ------------------------------------------------------------------------------------------------
def rotation_from_quaternion(q):
    """(w, x, y, z), any norm but 0 -> the 3x3 rotation matrix (the formula of numpy-quaternion's as_rotation_matrix,
    which divides by the squared norm instead of normalising first)"""
    w, x, y, z = (float(t) for t in q)
    n = w * w + x * x + y * y + z * z
    if n == 0:
        raise ZeroDivisionError("rotation_from_quaternion: a zero quaternion")
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


def matrix_from_trs(trs):
    """{'translation', 'rotation' (w, x, y, z), 'scale'} -> the 4x4 matrix T R S (tools.py: make_M_from_tqs)"""
    T, R, S = np.eye(4), np.eye(4), np.eye(4)
    T[0:3, 3] = trs['translation']
    R[0:3, 0:3] = rotation_from_quaternion(trs['rotation'])
    S[0:3, 0:3] = np.diag(np.asarray(trs['scale'], np.float64))
    return T.dot(R).dot(S)


def unit(a):
    n = np.linalg.norm(a)
    return a / (n if n != 0 else 1.)


def yaw_axes(yaw):
    return np.array([[np.cos(yaw), np.sin(yaw), 0], [-np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])


def box_corners(box):
    """box (7,) -> (8,3): tools.py's get_box_corners over the half-size vectors of the yawed box"""
    c, v = box[:3], np.diag(box[3:6] / 2.).dot(yaw_axes(box[6]))
    signs = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    return np.array([c + a * v[0] + b * v[1] + d * v[2] for a, b, d in signs])


def rectify(axes):
    """the transformed, normalised (forward, left, up) rows -> (order: which of them is the box's x, y, z, yaw): lines
    134-156 of generate().  The row that points up most becomes z; the box's x is `forward` unless that went up."""
    up = int(np.argmax(axes[:, 2]))
    fwd = 0 if up != 0 else (up + 1) % 3
    left = int(np.setdiff1d([0, 1, 2], [up, fwd])[0])
    f = unit(np.array([axes[fwd][0], axes[fwd][1], 0.]))
    return [fwd, left, up], float(np.arctan2(f[1], f[0]))


def class_of(catid):
    """a model's catid_cad -> the class id, or None outside the filter"""
    return SYNSET_CLASS.get(str(catid).zfill(8))


# ---- device stages -----------------------------------------------------------------------------------------------------
def _xyz_rows(vertices):
    """a (N, >= 3) float32 device tensor as the kernels read it -> (tensor, stride)"""
    _lib.need_gpu(vertices)
    if vertices.dim() != 2 or vertices.shape[1] < 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices are (N, >= 3) float32, got %s %s" % (vertices.dtype, tuple(vertices.shape)))
    v = vertices.contiguous()
    ragged.offsets([v.numel()])
    return v, int(v.shape[1])


@torch.no_grad()
def instance_boxes(vertices, instance_ids, n_instances=None):
    """vertices (N, >= 3) f32, instance_ids (N,) integer, both on the device -> (I,6) f64 numpy: centre and size of the
    axis-aligned box of the vertices of every id 1 .. I (export's instance_bboxes without the label column).  The box is
    finished in f32, as numpy does on the f32 columns, and then widened; an id without a vertex has a row of zeros.  I
    defaults to the largest id (one read-back)."""
    v, stride = _xyz_rows(vertices)
    _lib.need_gpu(instance_ids)
    if instance_ids.dtype.is_floating_point or instance_ids.shape != (v.shape[0],):
        raise ValueError("instance_ids are (N,) integers, got %s %s" % (instance_ids.dtype, tuple(instance_ids.shape)))
    N, dev = int(v.shape[0]), v.device
    ids = instance_ids.to(torch.int32).contiguous()          # u32 on the device: a negative id is above I, ignored
    I = int(n_instances) if n_instances is not None else (int(instance_ids.max()) if N else 0)
    if I < 0:
        raise ValueError("n_instances = %d" % I)
    box = torch.zeros(I, 6, dtype=torch.float32, device=dev)
    if I:
        keys = torch.empty(I, 6, dtype=torch.int32, device=dev)
        _lib.call("rfd_labels_instance_aabb", dev, N, I, stride, v.data_ptr(), ids.data_ptr(), keys.data_ptr(),
                  box.data_ptr())
    lo, hi = box[:, :3], box[:, 3:]
    return torch.cat([(lo + hi) / 2, hi - lo], 1).double().cpu().numpy()


@torch.no_grad()
def cad_extents(vertex_sets, L, device):
    """vertex_sets: M arrays (V_m,3); L (M,3,3) f64 -> (M,12) f64 numpy: min p, max p, min L p, max L p per model
    (rule E of include/rfd_labels.h).  One upload of the flat ragged batch, one read-back."""
    M = len(vertex_sets)
    if M == 0:
        return np.zeros((0, 12))
    sets = [np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1, 3) for v in vertex_sets]
    counts = [len(s) for s in sets]
    if min(counts) == 0:
        raise ValueError("cad_extents: model %d has no vertex" % counts.index(0))
    if not all(np.isfinite(s).all() for s in sets):
        raise ValueError("cad_extents: a vertex is not finite")
    off = ragged.offsets(counts)
    ragged.offsets([3 * int(off[-1])])
    owner, start = ragged.runs(counts, EXTENT_STEP)
    dev = torch.device(device)
    _lib.need_gpu(torch.empty(0, device=dev))
    pts = torch.from_numpy(np.concatenate(sets)).to(dev)
    maps = ragged.to_int32(np.concatenate([off, owner, start]), dev)
    d_off, d_owner, d_start = maps[:M + 1], maps[M + 1:M + 1 + len(owner)], maps[M + 1 + len(owner):]
    d_L = torch.from_numpy(np.ascontiguousarray(np.asarray(L, np.float64).reshape(M, 9))).to(dev)
    keys = torch.empty(M, 12, dtype=torch.int64, device=dev)
    ext = torch.empty(M, 12, dtype=torch.float64, device=dev)
    _lib.call("rfd_labels_cad_extents", dev, M, len(owner), EXTENT_STEP, pts.data_ptr(), d_off.data_ptr(),
              d_owner.data_ptr(), d_start.data_ptr(), d_L.data_ptr(), keys.data_ptr(), ext.data_ptr())
    return ext.cpu().numpy()


def cad_boxes(models, scan_transform, axis_align, device='cuda'):
    """models: Scan2CAD's aligned_models, each {'catid_cad', 'id_cad', 'trs': {...}, 'vertices': (V,3)};
    scan_transform: the annotation's own 'trs'; axis_align: the scan's 4x4 axisAlignment
    -> (boxes, mean_sizes): one {'box3D' (7,) f64, 'cls_id', 'shapenet_catid', 'shapenet_id'} per model INSIDE the class
    filter, in annotation order, and {cls_id: [size, ...]} over OBJ_CLASS_IDS.

    box3D = (centre, size along the box's x, y, z, yaw), as generate() defines it: the CAD vertices go through
    T = axis_align inv(M_scan) M_cad, their extents are taken along the transformed, normalised model axes A
    (forward = -z, left = -x, up = +y of the model), and the axis that points up most becomes the box's z.  The
    reference measures (T p - c_t) A^T; that is L (p - c) with L = A T_lin, so max - min needs neither centre and one
    pass over the vertices gives it, together with the model's own bounding box for the centre."""
    kept = [(m, class_of(m['catid_cad'])) for m in models]
    kept = [(m, c) for m, c in kept if c is not None]
    mean_sizes = {c: [] for c in OBJ_CLASS_IDS}
    if not kept:
        return [], mean_sizes
    R_transform = np.asarray(axis_align, np.float64).reshape(4, 4).dot(np.linalg.inv(matrix_from_trs(scan_transform)))
    Ts = [R_transform.dot(matrix_from_trs(m['trs'])) for m, _ in kept]
    axes = [np.array([unit(-T[:3, 2]), unit(-T[:3, 0]), unit(T[:3, 1])]) for T in Ts]
    L = np.array([A.dot(T[:3, :3]) for A, T in zip(axes, Ts)])
    ext = cad_extents([m['vertices'] for m, _ in kept], L, device)
    boxes = []
    for (m, cls_id), T, A, e in zip(kept, Ts, axes, ext):
        centre = (e[3:6] + e[0:3]) / 2.
        centre_t = np.append(centre, 1.).dot(T.T)[:3]
        sizes = e[9:12] - e[6:9]
        order, yaw = rectify(A)
        box3D = np.hstack([centre_t, sizes[order], [yaw]])
        mean_sizes[cls_id].append(box3D[3:6])
        boxes.append({'box3D': box3D, 'cls_id': cls_id, 'shapenet_catid': m['catid_cad'], 'shapenet_id': m['id_cad']})
    return boxes, mean_sizes


@torch.no_grad()
def match_instances(boxes, inst_boxes, device='cuda'):
    """boxes (M,7) f64 CAD boxes, inst_boxes (I, >= 6) f64 centre + size -> (instance_id (M,) int64 numpy: the 1-based
    instance of the largest cuboid IoU, the first of equals, 0 when no IoU is positive; best (M,) f64; second (M,) f64:
    the runner-up's IoU)"""
    b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 7))
    a = np.asarray(inst_boxes, np.float64)
    a = np.ascontiguousarray(a.reshape(len(a), -1)[:, :6]) if a.size else np.zeros((0, 6))
    M, I, dev = len(b), len(a), torch.device(device)
    _lib.need_gpu(torch.empty(0, device=dev))
    d_b, d_a = torch.from_numpy(b).to(dev), torch.from_numpy(a).to(dev)
    out = torch.zeros(2, M, dtype=torch.float64, device=dev)
    ids = torch.zeros(M, dtype=torch.int32, device=dev)
    _lib.call("rfd_labels_match_instances", dev, M, I, d_b.data_ptr(), d_a.data_ptr(), out[0].data_ptr(),
              ids.data_ptr(), out[1].data_ptr())
    out = out.cpu().numpy()
    return ids.cpu().numpy().astype(np.int64), out[0], out[1]


@torch.no_grad()
def point_votes(vertices, boxes):
    """vertices (N, >= 3) f32 on the device, boxes (M,7) f64 (any M) -> (votes (N,10) f64: the mask and three votes of
    every vertex as full_scan.npz holds them, hits (N,) i32: the boxes that contain it), both on the device"""
    v, stride = _xyz_rows(vertices)
    N, dev = int(v.shape[0]), v.device
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 7))).to(dev)
    ragged.offsets([10 * N])
    votes = torch.zeros(N, 10, dtype=torch.float64, device=dev)
    hits = torch.zeros(N, dtype=torch.int32, device=dev)
    _lib.call("rfd_labels_point_votes", dev, N, int(b.shape[0]), stride, v.data_ptr(), b.data_ptr(), votes.data_ptr(),
              hits.data_ptr())
    return votes, hits


@torch.no_grad()
def align_vertices(vertices, axis_align):
    """export's axis alignment: xyz (f32) through the 4x4 matrix in f64, stored back as f32; other columns kept"""
    A = torch.as_tensor(np.asarray(axis_align, np.float64).reshape(4, 4), device=vertices.device)
    out = vertices.clone()
    out[:, :3] = (vertices[:, :3].double() @ A[:3, :3].T + A[:3, 3]).float()
    return out


def prepare_scan(vertices, instance_ids, models, scan_transform, axis_align, aligned=True, n_instances=None):
    """generate() for one scan.  vertices (N,6) f32 xyz + rgb and instance_ids (N,) on the device, `aligned`: the xyz
    are already in the axis-aligned frame (export's output); models / scan_transform / axis_align as cad_boxes
    -> None when no model is inside the class filter (nothing is written then), else
    (boxes: bbox.pkl's list, scan: full_scan.npz's arrays as numpy, mean_sizes)."""
    _lib.need_gpu(vertices, instance_ids)
    if not aligned:
        vertices = align_vertices(vertices, axis_align)
    boxes, mean_sizes = cad_boxes(models, scan_transform, axis_align, vertices.device)
    if not boxes:
        return None
    box3D = np.array([b['box3D'] for b in boxes])
    ids, _, _ = match_instances(box3D, instance_boxes(vertices, instance_ids, n_instances), vertices.device)
    for b, i in zip(boxes, ids):
        b['instance_id'] = int(i)
        b['box_corners'] = box_corners(b['box3D'])
    votes, _ = point_votes(vertices, box3D)
    scan = {'mesh_vertices': vertices.cpu().numpy(), 'point_votes': votes.cpu().numpy(),
            'instance_labels': instance_ids.cpu().numpy().astype(np.uint32)}
    return boxes, scan, mean_sizes


def mean_size_array(mean_sizes_all):
    """the per-scan mean_sizes dictionaries -> (8,3): the class means the reference stores as scannet_means*.npz"""
    out = np.zeros((len(OBJ_CLASS_IDS), 3))
    for k, c in enumerate(OBJ_CLASS_IDS):
        sizes = [s for d in mean_sizes_all if d is not None for s in d[c]]
        out[k] = np.mean(sizes, axis=0) if sizes else np.nan
    return out


# ---- the dataloader's sample -------------------------------------------------------------------------------------------
def percentile_plan(n, q=0.99):
    """numpy's np.percentile(x, q) of n float32 values, method 'linear' -> (lo, hi, gamma): the two order statistics
    it reads and the float32 weight it interpolates with.  numpy divides q by a float32 100 and forms the virtual index
    in the array's own precision."""
    quantile = np.asanyarray(np.true_divide(float(q), np.float32(100)))       # float32: a Python float is weak
    virtual = (n - 1) * quantile
    lo = int(np.floor(virtual))
    gamma = np.asanyarray(virtual - lo, dtype=virtual.dtype)
    lo = min(max(lo, 0), n - 1)
    return lo, min(lo + 1, n - 1), gamma


def lerp(a, b, gamma):
    """numpy's _lerp on scalars of one dtype"""
    d = b - a
    out = a + d * gamma
    if gamma >= 0.5:
        out = b - d * (1 - gamma)
    return out


@torch.no_grad()
def floor_height(z):
    """z (N,) f32 on the device -> np.percentile(z, 0.99) as numpy gives it on float32 (a float32): the two order
    statistics by torch.kthvalue, the interpolation on the host.  One read-back of two values."""
    n = int(z.shape[0])
    lo, hi, gamma = percentile_plan(n)
    pair = torch.stack([torch.kthvalue(z, lo + 1)[0], torch.kthvalue(z, hi + 1)[0]]).cpu().numpy()
    return np.float32(lerp(pair[0], pair[1], gamma[()]))


def draw(rng, n_vertices, num_point, augment):
    """the dataloader's random draws from `rng` (a numpy.random.RandomState), in its order -> (flips, rot_angle,
    choices): in train mode two flips and the angle in [-pi/4, pi/4), then the choice of num_point vertices (with
    replacement iff the scan has fewer)"""
    flips, rot_angle = (False, False), 0.
    if augment:
        flips = (bool(rng.random_sample() > 0.5), bool(rng.random_sample() > 0.5))
        rot_angle = float((rng.random_sample() * np.pi / 2) - np.pi / 4)
    return flips, rot_angle, rng.choice(n_vertices, num_point, replace=n_vertices < num_point)


def augment_boxes(box3D, flips, rot_angle):
    """the flips and the z-rotation of the dataloader on (M,7) boxes, f64, in its order"""
    b = np.array(box3D, np.float64)
    if flips[0]:
        b[:, 0] = -1 * b[:, 0]
        b[:, 6] = np.sign(b[:, 6]) * np.pi - b[:, 6]
    if flips[1]:
        b[:, 1] = -1 * b[:, 1]
        b[:, 6] = -1 * b[:, 6]
    c, s = np.cos(rot_angle), np.sin(rot_angle)
    b[:, 0:3] = np.dot(b[:, 0:3], np.transpose(np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])))
    b[:, 6] += rot_angle
    b[:, 6] = np.mod(b[:, 6] + np.pi, 2 * np.pi) - np.pi
    return b


def box_labels(box3D, classes, instance_ids, dataset_config):
    """the 64-row label arrays of __getitem__ (numpy, the reference's dtypes)"""
    M = len(box3D)
    class_ind = [dataset_config.shapenetid2class[c] for c in classes]
    size_residuals, centres = np.zeros((MAX_NUM_OBJ, 3)), np.zeros((MAX_NUM_OBJ, 6))
    size_classes, mask, sem = np.zeros(MAX_NUM_OBJ), np.zeros(MAX_NUM_OBJ), np.zeros(MAX_NUM_OBJ)
    angle_classes, angle_residuals, inst = np.zeros(MAX_NUM_OBJ), np.zeros(MAX_NUM_OBJ), np.zeros(MAX_NUM_OBJ)
    if M:
        size_classes[:M] = class_ind
        size_residuals[:M] = box3D[:, 3:6] - dataset_config.mean_size_arr[class_ind, :]
        mask[:M] = 1
        centres[:M] = box3D[:, 0:6]
        inst[:M] = instance_ids
        angle_classes[:M], angle_residuals[:M] = dataset_config.angle2class(box3D[:, 6])
        sem[:M] = class_ind
    return {'center_label': centres.astype(np.float32)[:, 0:3],
            'heading_class_label': angle_classes.astype(np.int64),
            'heading_residual_label': angle_residuals.astype(np.float32),
            'size_class_label': size_classes.astype(np.int64),
            'size_residual_label': size_residuals.astype(np.float32),
            'sem_cls_label': sem.astype(np.int64),
            'box_label_mask': mask.astype(np.float32),
            'object_instance_labels': inst.astype(np.float32)}


def subsample_points(points, occ, n, mode, rng):
    """net_utils/transforms.py's SubsamplePoints for an integer n: the first n in test mode, n random rows otherwise"""
    idx = np.arange(0, n) if mode == 'test' else rng.randint(points.shape[0], size=n)
    return points[idx, :], occ[idx]


def completion_labels(boxes, shapenet_path, n_points, mode, rng, unpackbits=True):
    """the completion keys of __getitem__, from the files tools/sample_mesh.py writes under `shapenet_path`:
    point/<catid>/<id>.npz (points, occupancies) and voxel/16/<catid>/<id>.binvox"""
    from . import io
    M = len(boxes)
    pts, occ, vox, pts_all, occ_all = [], [], [], [], []
    for b in boxes:
        d = np.load(os.path.join(shapenet_path, 'point', b['shapenet_catid'], b['shapenet_id'] + '.npz'))
        p = d['points']
        if p.dtype == np.float16 and mode == 'train':
            p = p.astype(np.float32)
            p += 1e-4 * rng.randn(*p.shape)
        else:
            p = p.astype(np.float32)
        o = d['occupancies']
        if unpackbits:
            o = np.unpackbits(o)[:p.shape[0]]
        o = o.astype(np.float32)
        pts_all.append(p)
        occ_all.append(o)
        sp, so = subsample_points(p, o, n_points, mode, rng)
        pts.append(sp)
        occ.append(so)
    for b in boxes:
        grid = io.read_binvox(os.path.join(shapenet_path, 'voxel', '16', b['shapenet_catid'],
                                           b['shapenet_id'] + '.binvox'))[0]
        vox.append(grid.astype(np.float32))

    def padded(rows, shape):
        out = np.zeros((MAX_NUM_OBJ,) + shape)
        if M:
            out[:M] = np.stack(rows)
        return out.astype(np.float32)
    out = {'object_points': padded(pts, (n_points, 3)), 'object_points_occ': padded(occ, (n_points,)),
           'object_voxels': padded(vox, vox[0].shape if M else (16, 16, 16))}
    if mode == 'test':
        n_iou = occ_all[0].shape[-1] if M else 0
        out['object_points_iou'] = padded(pts_all, (n_iou, 3))
        out['object_points_iou_occ'] = padded(occ_all, (n_iou,))
        out['shapenet_catids'] = [b['shapenet_catid'] for b in boxes]
        out['shapenet_ids'] = [b['shapenet_id'] for b in boxes]
    return out


@torch.no_grad()
def make_sample(scan, boxes, cfg, mode, rng=None, choices=None, flips=None, rot_angle=None, shapenet_path=None,
                scan_idx=0, device='cuda', instance_labels=None):
    """ISCNet_ScanNet.__getitem__ for one prepared scan -> its dictionary.  The per-point arrays (point_clouds,
    vote_label, vote_label_mask, point_instance_labels) are tensors on the device, made by one kernel; the 64-row label
    arrays, scan_idx and the completion keys are numpy, with the reference's dtypes.

    scan: full_scan.npz's arrays (numpy or tensors), boxes: bbox.pkl's list, cfg: a Config (data.num_point, no_height,
    use_color_*; dataset_config with mean_size_arr), mode: 'train' augments, anything else does not.
    Randomness: the reference draws from numpy's global state two flips, the angle and then the choice (only the
    choice outside train mode); the same draws are taken here, in that order, from `rng` (a numpy.random.RandomState)
    for whatever is not given explicitly: flips = (bool, bool), rot_angle in radians, choices (num_point,) indices.
    shapenet_path: add the completion keys (data.points_subsample points per object, an integer).  The two instance
    label arrays belong to the completion phase in the reference; instance_labels=True adds them without it."""
    data = cfg.config['data']
    dev = torch.device(device)
    if len(boxes) > MAX_NUM_OBJ:
        raise ValueError("make_sample: %d boxes, the label arrays hold MAX_NUM_OBJ = %d" % (len(boxes), MAX_NUM_OBJ))
    vertices = _lib.as_tensor(scan['mesh_vertices'], dev, torch.float32)
    votes = _lib.as_tensor(scan['point_votes'], dev, torch.float64).contiguous()
    labels = scan['instance_labels']
    labels = (labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels).astype(np.int64)))
    labels = labels.to(dev, torch.int32).contiguous()
    v, stride = _xyz_rows(vertices)
    N = int(v.shape[0])
    if votes.shape != (N, 10) or labels.shape != (N,):
        raise ValueError("make_sample: %d vertices, point_votes %s, instance_labels %s"
                         % (N, tuple(votes.shape), tuple(labels.shape)))
    if N == 0:
        raise ValueError("make_sample: an empty scan")
    use_color = bool(data.get('use_color_detection') or data.get('use_color_completion'))
    use_height = not data.get('no_height', False)
    if use_color and stride < 6:
        raise ValueError("make_sample: colours asked for, the vertices have %d columns" % stride)
    augment = mode == 'train'
    num_point = int(data['num_point'])
    if rng is None and (choices is None or (augment and (flips is None or rot_angle is None))):
        raise ValueError("make_sample: pass rng, or every draw explicitly (choices; in train mode flips and rot_angle)")
    if rng is not None and (choices is None or (augment and (flips is None or rot_angle is None))):
        drawn = draw(rng, N, num_point, augment)
        flips = drawn[0] if flips is None else flips
        rot_angle = drawn[1] if rot_angle is None else rot_angle
        choices = drawn[2] if choices is None else choices
    if not augment:
        flips, rot_angle = (False, False), 0.
    flips = (bool(flips[0]), bool(flips[1]))
    choices = np.asarray(choices, np.int64).reshape(-1)
    if choices.size and (choices.min() < 0 or choices.max() >= N):
        raise ValueError("make_sample: choices outside [0, %d)" % N)
    P = int(choices.size)
    box3D = np.array([b['box3D'] for b in boxes], np.float64).reshape(-1, 7)
    if augment:
        box3D = augment_boxes(box3D, flips, rot_angle)
    n_color = 3 if use_color else 0
    C = 3 + n_color + int(use_height)
    ragged.offsets([P * max(C, 9)])
    floor = floor_height(v[:, 2]) if use_height else np.float32(0)
    d_choices = torch.from_numpy(choices).to(dev)
    points = torch.empty(P, C, dtype=torch.float32, device=dev)
    vote_label = torch.empty(P, 9, dtype=torch.float32, device=dev)
    vote_mask = torch.empty(P, dtype=torch.int64, device=dev)
    instance = torch.empty(P, dtype=torch.float32, device=dev)
    mean = (_lib.C.c_double * 3)(*MEAN_COLOR_RGB)
    _lib.call("rfd_labels_sample", dev, P, N, stride, n_color, int(use_height), int(augment), int(flips[0]),
              int(flips[1]), float(np.cos(rot_angle)), float(np.sin(rot_angle)), float(floor), mean, v.data_ptr(),
              votes.data_ptr(), labels.data_ptr(), d_choices.data_ptr(), points.data_ptr(), vote_label.data_ptr(),
              vote_mask.data_ptr(), instance.data_ptr())
    out = {'point_clouds': points, 'vote_label': vote_label, 'vote_label_mask': vote_mask,
           'scan_idx': np.array(scan_idx).astype(np.int64)}
    out.update(box_labels(box3D, [b['cls_id'] for b in boxes], [b['instance_id'] for b in boxes], cfg.dataset_config))
    if instance_labels is None:
        instance_labels = shapenet_path is not None
    if instance_labels:
        out['point_instance_labels'] = instance
    else:
        del out['object_instance_labels']
    if shapenet_path is not None:
        if mode == 'train' and rng is None:
            raise ValueError("make_sample: the completion keys of train mode draw from rng")
        out.update(completion_labels(boxes, shapenet_path, int(data['points_subsample']), mode, rng,
                                     data.get('points_unpackbits', True)))
    return out
