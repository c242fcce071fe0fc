"""The scan ground truth restated in numpy, independently of rfdnet_amd/scan_labels.py and of the kernels: what the
reference's generate() and ISCNet_ScanNet.__getitem__ compute, step by step in their order and precision (float64 unless
the reference holds a float32 array).  tests/test_scan_labels_cpu.py holds it to the reference's own output
(tests/golden/F_SCAN.npz); tests/test_gpu_scan_labels.py holds the kernels to it.

The bound on a CAD box's sizes (extent_bound).  The kernel measures q = L p with L = A T_lin, every component a
three-term product sum in float64 evaluated left to right: fl(q_i) = sum_j L_ij p_j (1 + d_j) with |d_j| <= 3u
(u = 2^-53: one rounding of the product and at most two of the sums), so |fl(q_i) - q_i| <= 3u S_i with
S_i = sum_j |L_ij| |p_j|.  L itself is a rounded 3x3 product of A (rows normalised in floating point) and T_lin
(itself a rounded product of the annotation's matrices): each entry carries at most 4u of relative error against the
exact product of the same factors, another 4u S_i.  A size is max - min: two such values and one more rounding, so
|size_i - exact_i| <= 2 (3 + 4) u S_i + u |size_i| <= 16 u max_p S_i(p).  The GPU tests allow the kernel these
16 u max S_i against the restatement below and against the reference's box3D; against extents_exact, which evaluates
the SAME rounded L in extended precision, they allow the 3 u S_i of the product sum alone.

The bound between two evaluations of the reference's own route (route_bound).  cad_box below and the reference both
form (T p - c_t) A^T, which carries the translation t through every vertex: fl(T p) is a four-term sum, off by at most
4u R with R = max_p sum_j |T_ij| |p_j| + |t_i| (the largest over the axes); c_t the same; their difference adds a
rounding of at most 2u R: 10u R per component.  A row of A has 1-norm at most sqrt(3), and the three-term sum adds 3u
of its own: below 23u R per coordinate, 46u R per size, and two routes that round differently (the matrices are
composed in another order here) are at most 92u R apart: 96 u R.  Nothing in either bound is measured."""
import numpy as np

U = 2.0 ** -53
MAX_NUM_OBJ = 64
MEAN_COLOR_RGB = np.array([121.87661, 109.73591, 95.61673])
CLASS_IDS = [1, 7, 8, 13, 20, 31, 34, 43]
SYNSETS = {'04379243': 1, '03001627': 7, '02871439': 8, '04256520': 13, '02747177': 20, '02933112': 31, '03211117': 34,
           '02808440': 43}


# ---- instance boxes ------------------------------------------------------------------------------------------------------
def instance_boxes(vertices, ids, n):
    """(n,6) f64: per id 1 .. n the centre and size of the vertices' box, formed on the f32 columns"""
    out = np.zeros((n, 6))
    xyz = np.asarray(vertices)[:, :3]
    for i in range(1, n + 1):
        pc = xyz[np.asarray(ids) == i]
        if len(pc):
            lo, hi = pc.min(0), pc.max(0)
            out[i - 1] = np.concatenate([(lo + hi) / 2, hi - lo])
    return out


# ---- CAD boxes -----------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    w, x, y, z = np.asarray(q, np.float64)
    n = w * w + x * x + y * y + z * z
    return np.eye(3) + (2 / n) * np.array([[-(y * y + z * z), x * y - z * w, x * z + y * w],
                                           [x * y + z * w, -(x * x + z * z), y * z - x * w],
                                           [x * z - y * w, y * z + x * w, -(x * x + y * y)]])


def trs_matrix(t, q, s):
    T, R, S = np.eye(4), np.eye(4), np.eye(4)
    T[:3, 3], R[:3, :3], S[:3, :3] = t, quat_matrix(q), np.diag(s)
    return T @ R @ S


def model_transform(axis_align, scan_trs, model_trs):
    """the 4x4 matrix that takes a CAD vertex into the axis-aligned scan"""
    return (np.asarray(axis_align).reshape(4, 4) @ np.linalg.inv(trs_matrix(*scan_trs))) @ trs_matrix(*model_trs)


def homogeneous(points, T):
    return np.hstack([points, np.ones((len(points), 1))]).dot(T.T)[:, :3]


def cad_box(vertices, T):
    """one model's vertices (V,3) and its 4x4 matrix -> (box3D (7,), order, axes): generate()'s route, the centre first"""
    v = np.asarray(vertices, np.float64)
    centre = (v.max(0) + v.min(0)) / 2.
    probe = homogeneous(np.array([centre, centre - [0, 0, 1], centre - [1, 0, 0], centre + [0, 1, 0]]), T)
    axes = probe[1:] - probe[0]
    axes = axes / np.linalg.norm(axes, axis=1, keepdims=True)
    up = int(np.argmax(axes[:, 2]))
    fwd = 0 if up != 0 else 1
    left = 3 - up - fwd
    f = np.array([axes[fwd, 0], axes[fwd, 1], 0.])
    f = f / np.linalg.norm(f)
    coords = (homogeneous(v, T) - probe[0]).dot(axes.T)
    sizes = coords.max(0) - coords.min(0)
    order = [fwd, left, up]
    return np.hstack([probe[0], sizes[order], [np.arctan2(f[1], f[0])]]), order, axes


def extent_bound(vertices, T, order):
    """(3,) the bound of the module docstring on the three sizes of cad_box, in the box's order"""
    lin = T[:3, :3]
    axes = np.array([-lin[:, 2], -lin[:, 0], lin[:, 1]])
    L = (axes / np.linalg.norm(axes, axis=1, keepdims=True)) @ lin
    S = (np.abs(np.asarray(vertices, np.float64)) @ np.abs(L).T).max(0)
    return 16 * U * S[order]


def route_bound(vertices, T):
    """the second bound of the module docstring: between two float64 evaluations of (T p - c_t) A^T"""
    R = (np.abs(np.asarray(vertices, np.float64)) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max()
    return 96 * U * R


def extents_exact(vertices, L):
    """(12,) min p, max p, min L p, max L p with the product sums in extended precision (64 mantissa bits on x86; exact
    rational arithmetic where long double is no wider than double), rounded to float64 at the end"""
    p = np.asarray(vertices, np.float64)
    if np.finfo(np.longdouble).eps < 1e-18:
        q = (p.astype(np.longdouble) @ np.asarray(L, np.float64).reshape(3, 3).astype(np.longdouble).T).astype(np.float64)
    else:
        from fractions import Fraction
        Lf = [[Fraction(float(x)) for x in row] for row in np.asarray(L, np.float64).reshape(3, 3)]
        q = np.array([[float(sum(l * Fraction(float(x)) for l, x in zip(row, pt))) for row in Lf] for pt in p])
    return np.concatenate([p.min(0), p.max(0), q.min(0), q.max(0)])


def extents_rule(vertices, L):
    """(12,) rule E of include/rfd_labels.h in float64, operation by operation: what the kernel must give bit for bit"""
    p, L = np.asarray(vertices, np.float64), np.asarray(L, np.float64).reshape(3, 3)
    q = np.stack([(L[i, 0] * p[:, 0] + L[i, 1] * p[:, 1]) + L[i, 2] * p[:, 2] for i in range(3)], 1)
    return np.concatenate([p.min(0), p.max(0), q.min(0), q.max(0)])


def class_filter(catids):
    """-> the indices of the models inside the filter and their class ids"""
    keep = [k for k, c in enumerate(catids) if str(c) in SYNSETS]
    return keep, [SYNSETS[str(catids[k])] for k in keep]


# ---- matching ------------------------------------------------------------------------------------------------------------
def polygon_area(p):
    p = np.asarray(p, np.float64).reshape(-1, 2)
    if len(p) < 3:
        return 0.
    return 0.5 * abs(float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])))


def clip_convex(subject, clip):
    """subject, clip: convex polygons, clip counter-clockwise -> their intersection (general half-plane clipping)"""
    out = [np.asarray(p, np.float64) for p in subject]
    for a, b in zip(clip, np.roll(clip, -1, axis=0)):
        n = np.array([-(b - a)[1], (b - a)[0]])                       # inward normal of a counter-clockwise edge
        cur, out = out, []
        for k, p in enumerate(cur):
            q = cur[(k + 1) % len(cur)]
            dp, dq = float(n @ (p - a)), float(n @ (q - a))
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                out.append(p + (q - p) * (dp / (dp - dq)))
        if not out:
            break
    return out


def cuboid_iou(box, inst):
    """box (7,) yawed CAD box, inst (6,) axis-aligned centre + size -> get_iou_cuboid's IoU"""
    c, s = np.cos(box[6]), np.sin(box[6])
    v0, v1 = box[3] / 2 * np.array([c, s]), box[4] / 2 * np.array([-s, c])
    rect = np.array([box[:2] - v0 - v1, box[:2] + v0 - v1, box[:2] + v0 + v1, box[:2] - v0 + v1])
    h = inst[3:6] / 2
    sq = np.array([inst[:2] + [-h[0], -h[1]], inst[:2] + [h[0], -h[1]], inst[:2] + [h[0], h[1]], inst[:2] + [-h[0], h[1]]])
    bz, az = (box[2] - box[5] / 2, box[2] + box[5] / 2), (inst[2] - h[2], inst[2] + h[2])
    inter = polygon_area(clip_convex(rect, sq)) * max(0., min(bz[1], az[1]) - max(bz[0], az[0]))
    vol_b, vol_a = polygon_area(rect) * (bz[1] - bz[0]), polygon_area(sq) * (az[1] - az[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(inter) / (vol_b + vol_a - inter)


def match(boxes, inst_boxes):
    """-> (ids (M,), iou (M, I)): the first instance of the largest positive IoU, 1-based; 0 for none"""
    iou = np.array([[cuboid_iou(b, a[:6]) for a in inst_boxes] for b in boxes]).reshape(len(boxes), len(inst_boxes))
    ids = []
    for row in iou:
        best, best_id = 0., 0
        for i, x in enumerate(row):
            if x > best:
                best, best_id = x, i + 1
        ids.append(best_id)
    return np.array(ids, np.int64), iou


# ---- votes ---------------------------------------------------------------------------------------------------------------
def in_box(xyz, box):
    d = np.asarray(xyz, np.float64) - box[:3]
    c, s = np.cos(box[6]), np.sin(box[6])
    return (np.abs(d[:, 0] * c + d[:, 1] * s) <= abs(box[3] / 2)) & (np.abs(-d[:, 0] * s + d[:, 1] * c) <= abs(box[4] / 2)) \
        & (np.abs(d[:, 2]) <= abs(box[5] / 2))


def point_votes(vertices, boxes):
    """-> (votes (N,10) f64, hits (N,) i32): get_votes box after box, the in-box test as a box test"""
    xyz = np.asarray(vertices)[:, :3].astype(np.float64)
    votes, idx, hits = np.zeros((len(xyz), 10)), np.zeros(len(xyz), np.int64), np.zeros(len(xyz), np.int32)
    for box in np.asarray(boxes, np.float64).reshape(-1, 7):
        hit = in_box(xyz, box)
        votes[hit, 0] = 1
        for slot in range(3):                                         # a first hit fills every slot, later ones their own
            rows = np.nonzero(hit & ((idx == slot) | (idx == 0)))[0]
            votes[rows, 1 + 3 * slot:4 + 3 * slot] = box[:3] - xyz[rows]
        idx[hit] = np.minimum(2, idx[hit] + 1)
        hits[hit] += 1
    return votes, hits


# ---- the dataloader's sample ----------------------------------------------------------------------------------------------
def angle2class(angle, bins=12):
    angle = np.asarray(angle, np.float64) % (2 * np.pi)
    per = 2 * np.pi / bins
    shifted = (angle + per / 2) % (2 * np.pi)
    cls = (shifted / per).astype(np.int16)
    return cls, shifted - (cls * per + per / 2)


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, one rounding back to float64)"""
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def rotate_rows(a, c, s):
    """rows (n,3) f64 times rotz^T as a BLAS kernel with fused accumulation over k forms it (the numpy the fixture was
    made with did): x' = fma(y, -s, x c), y' = fma(y, c, x s), z' = z.  Spelled out so that the restatement does not
    depend on the BLAS of the machine it runs on."""
    out = np.array(a, np.float64)
    out[:, 0] = [fma(y, -s, x * c) for x, y in zip(a[:, 0], a[:, 1])]
    out[:, 1] = [fma(y, c, x * s) for x, y in zip(a[:, 0], a[:, 1])]
    return out


def sample(vertices, votes, labels, box3D, classes, instance_ids, mean_size_arr, choices, augment, flips=(False, False),
           angle=0., use_color=False, use_height=True):
    """__getitem__ in numpy -> its dictionary (detection keys and the two instance label arrays).  The per-point steps
    act on rows independently, so they are taken on the chosen rows only; the floor height is that of the whole cloud."""
    full = np.array(vertices, np.float32)
    pc = full[choices][:, :6 if use_color else 3]
    votes, boxes = np.array(votes, np.float64)[choices], np.array(box3D, np.float64).reshape(-1, 7)
    if use_color:
        pc[:, 3:] = (pc[:, 3:] - MEAN_COLOR_RGB) / 256.0
    if use_height:
        pc = np.concatenate([pc, (pc[:, 2] - np.percentile(full[:, 2], 0.99))[:, None]], 1)
        assert pc.dtype == np.float32
    if augment:
        if flips[0]:
            pc[:, 0], boxes[:, 0] = -pc[:, 0], -boxes[:, 0]
            boxes[:, 6] = np.sign(boxes[:, 6]) * np.pi - boxes[:, 6]
            votes[:, [1, 4, 7]] = -votes[:, [1, 4, 7]]
        if flips[1]:
            pc[:, 1], boxes[:, 1], boxes[:, 6] = -pc[:, 1], -boxes[:, 1], -boxes[:, 6]
            votes[:, [2, 5, 8]] = -votes[:, [2, 5, 8]]
        c, s = np.cos(angle), np.sin(angle)
        ends = [rotate_rows(pc[:, 0:3] + votes[:, 1 + 3 * k:4 + 3 * k], c, s) for k in range(3)]
        pc[:, 0:3] = rotate_rows(pc[:, 0:3].astype(np.float64), c, s)
        boxes[:, 0:3] = rotate_rows(boxes[:, 0:3], c, s)
        boxes[:, 6] = np.mod(boxes[:, 6] + angle + np.pi, 2 * np.pi) - np.pi
        for k in range(3):
            votes[:, 1 + 3 * k:4 + 3 * k] = ends[k] - pc[:, 0:3]
    M = len(boxes)
    ind = [CLASS_IDS.index(c) for c in classes]
    out = {k: np.zeros((MAX_NUM_OBJ,) + shape) for k, shape in (
        ('center_label', (3,)), ('heading_class_label', ()), ('heading_residual_label', ()), ('size_class_label', ()),
        ('size_residual_label', (3,)), ('sem_cls_label', ()), ('box_label_mask', ()), ('object_instance_labels', ()))}
    out['center_label'][:M] = boxes[:, :3]
    out['heading_class_label'][:M], out['heading_residual_label'][:M] = angle2class(boxes[:, 6])
    out['size_class_label'][:M] = out['sem_cls_label'][:M] = ind
    out['size_residual_label'][:M] = boxes[:, 3:6] - np.asarray(mean_size_arr)[ind]
    out['box_label_mask'][:M] = 1
    out['object_instance_labels'][:M] = instance_ids
    out = {k: v.astype(np.int64 if k in ('heading_class_label', 'size_class_label', 'sem_cls_label') else np.float32)
           for k, v in out.items()}
    out['point_clouds'] = pc.astype(np.float32)
    out['vote_label'] = votes[:, 1:].astype(np.float32)
    out['vote_label_mask'] = votes[:, 0].astype(np.int64)
    out['point_instance_labels'] = np.asarray(labels)[choices].astype(np.float32)
    out['scan_idx'] = np.array(0).astype(np.int64)
    return out


SAMPLE_KEYS = ('point_clouds', 'center_label', 'heading_class_label', 'heading_residual_label', 'size_class_label',
               'size_residual_label', 'sem_cls_label', 'box_label_mask', 'vote_label', 'vote_label_mask', 'scan_idx')


def load_fixture(path):
    """F_SCAN.npz -> (arrays, models: the annotation's aligned_models with their vertices, scan_trs)"""
    import os
    fx = dict(np.load(path if path else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F_SCAN.npz")))
    off = np.concatenate([[0], np.cumsum(fx['model_counts'])])
    models = [{'catid_cad': str(fx['model_catid'][k]), 'id_cad': str(fx['model_id'][k]),
               'trs': {'translation': fx['model_translation'][k], 'rotation': fx['model_rotation'][k],
                       'scale': fx['model_scale'][k]},
               'vertices': fx['model_vertices'][off[k]:off[k + 1]]} for k in range(len(fx['model_counts']))]
    scan_trs = {'translation': fx['scan_translation'], 'rotation': fx['scan_rotation'], 'scale': fx['scan_scale']}
    return fx, models, scan_trs


def trs_tuple(trs):
    return trs['translation'], trs['rotation'], trs['scale']


# ---- what the CPU and the GPU tests share -----------------------------------
def ulp32(a):
    """the spacing of float32 at |a| (elementwise)"""
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


def centre_bound(vertices, T):
    """the centre is T (c, 1): a four-term product sum with the translation as its fourth term, 4u per term and route"""
    c = np.abs(vertices).max(0)
    return 8 * U * (np.abs(T[:3, :3]) @ c + np.abs(T[:3, 3]))


def reference_sample(arrays, mode):
    return {k: arrays["%s_%s" % (mode, k)] for k in SAMPLE_KEYS}


def check_sample(got, want, exact):
    """got: a sample as numpy; want: the reference's.  exact: every array equal; else the two rotated arrays within one
    float32 ulp (the routes differ by float64 roundings before the one rounding to float32) and the rest equal"""
    assert set(want) <= set(got)
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape)
        if exact or k not in ('point_clouds', 'vote_label', 'center_label', 'heading_residual_label'):
            assert np.array_equal(g, w), k
        else:
            assert (np.abs(g.astype(np.float64) - w) <= ulp32(w)).all(), k


def check_cad_boxes(fx, restated, boxes, mean_sizes):
    """sl.cad_boxes' output against the fixture and the restatement (shared with the GPU test)"""
    arrays, models, _ = fx
    keep, classes, restated_boxes, Ts = restated
    assert [b['cls_id'] for b in boxes] == list(arrays['cls_id']) == classes
    assert [b['shapenet_catid'] for b in boxes] == list(arrays['shapenet_catid'])
    assert [b['shapenet_id'] for b in boxes] == list(arrays['shapenet_id'])
    for k, b, (box, order, _), T, want in zip(keep, boxes, restated_boxes, Ts, arrays['box3D']):
        v, got = models[k]['vertices'], b['box3D']
        bound = extent_bound(v, T, order)
        ratios = np.abs(got[3:6] - want[3:6]) / bound, np.abs(got[3:6] - box[3:6]) / bound
        print("model %d: size error / bound against the fixture %s, against the restatement %s" % ((k,) + ratios))
        assert (ratios[0] <= 1).all() and (ratios[1] <= 1).all(), (k, ratios)
        assert (np.abs(got[:3] - want[:3]) <= centre_bound(v, T)).all(), (k, got[:3] - want[:3])
        assert abs(got[6] - want[6]) <= 16 * U * np.pi, (k, got[6] - want[6])
    assert sorted(mean_sizes) == sorted(CLASS_IDS)
    flat_cls = [c for c in CLASS_IDS for _ in mean_sizes[c]]
    assert flat_cls == list(arrays['mean_sizes_cls'])
    flat = np.array([s for c in CLASS_IDS for s in mean_sizes[c]])
    assert np.array_equal(flat, np.array([b['box3D'][3:6] for c in CLASS_IDS for b in boxes if b['cls_id'] == c]))


def restate_boxes(fx):
    """the restatement's boxes of the models inside the filter: (keep, classes, [(box3D, order, axes)], [T])"""
    arrays, models, scan_trs = fx
    keep, classes = class_filter([m['catid_cad'] for m in models])
    Ts = [model_transform(arrays['axis_align'], trs_tuple(scan_trs), trs_tuple(models[k]['trs'])) for k in keep]
    return keep, classes, [cad_box(models[k]['vertices'], T) for k, T in zip(keep, Ts)], Ts
