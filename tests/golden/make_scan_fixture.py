"""Writes tests/golden/F_SCAN.npz: what the reference's own ScanNet preparation (utils/scannet/
gen_scannet_w_orientation.py: generate) and its dataloader (models/iscnet/dataloader.py: ISCNet_ScanNet.__getitem__)
make of one small synthetic scan with seven aligned CAD models.

    python tests/golden/make_scan_fixture.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

The reference's Python runs as it lies; no reference text and no binary is kept.  What it cannot import here is
stubbed, and two of the stubs carry arithmetic, so two parts of the fixture rest on this file and not on the
reference's dependencies:
  * `quaternion` (numpy-quaternion): as_rotation_matrix below turns the annotation's quaternions into matrices;
  * `shapely`'s Polygon: the convex polygon clipper below gives get_iou_cuboid its areas, so the fixture's
    `instance_id`s rest on it.  The generator therefore asserts that best and runner-up IoU are at least 1e-9 apart for
    every box, and the match kernel is held to closed forms as well (tests/test_gpu_scan_labels.py).
scipy's Delaunay (the in-box test of get_votes) is the real one.  `export` (the scan's JSON readers) and `read_obj` are
replaced by functions that return the synthetic arrays; the instance boxes export would have made are formed here the way
it forms them.  The meta line, the label map, the split JSON and the configuration are temporary files and objects.

The scene is built so that the generator can assert, on the reference's output:
  * scan points covered by 1, 2, 3 and 4 CAD boxes (the capped third vote slot);
  * one model of a class outside the filter (02818832, a bed), which leaves no trace;
  * no scan point within FACE_MARGIN = 1e-6 m of any plane of a box face (tests/test_predictions_cpu.py's margin, inside
    which Delaunay may decide either way): points that come that close are redrawn before the final run, so the number
    of points excused from the bit-for-bit comparison is zero.
Two samples are stored: test mode (no augmentation, height, no colour) and train mode (both flips, a rotation, colour
and height), with the flips, the angle and the choices the reference drew."""
import argparse
import importlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "F_SCAN.npz")
FACE_MARGIN = 1e-6
IOU_GAP = 1e-9
N_VERTICES, NUM_POINT, SCENE = 5000, 2048, "scene0000_00"


# ---- stubs that carry arithmetic ---------------------------------------------------------------------------------------
def as_rotation_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def signed_area(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


class Polygon(object):
    """a convex polygon: .area and .intersection(other), all this fixture asks of shapely"""

    def __init__(self, points):
        self.points = np.asarray(points, np.float64).reshape(-1, 2)

    @property
    def area(self):
        return abs(signed_area(self.points)) if len(self.points) >= 3 else 0.

    def intersection(self, other):
        clip = other.points if signed_area(other.points) > 0 else other.points[::-1]
        subject = [tuple(p) for p in self.points]
        for a, b in zip(clip, np.roll(clip, -1, axis=0)):
            edge, out = b - a, []
            side = [edge[0] * (p[1] - a[1]) - edge[1] * (p[0] - a[0]) for p in subject]      # > 0: left of a -> b
            for k, p in enumerate(subject):
                q, sp, sq = subject[(k + 1) % len(subject)], side[k], side[(k + 1) % len(subject)]
                if sp >= 0:
                    out.append(p)
                if (sp >= 0) != (sq >= 0):
                    t = sp / (sp - sq)
                    out.append((p[0] + (q[0] - p[0]) * t, p[1] + (q[1] - p[1]) * t))
            subject = out
            if not subject:
                break
        return Polygon(subject) if subject else Polygon(np.zeros((0, 2)))


# ---- the reference, mounted --------------------------------------------------------------------------------------------
def ns(name, path=None, **attrs):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def mount_reference(ref):
    """-> (gen_scannet_w_orientation, dataloader, ScannetConfig) of the checkout at `ref`"""
    import torch  # noqa: F401
    import scipy.spatial  # noqa: F401  (before the aliases: numpy.ma reads np.bool while it loads)
    sys.path.insert(0, ref)
    np.bool, np.int = np.bool_, int                                   # the reference was written for an older numpy
    np.quaternion = lambda w, x, y, z: np.array([w, x, y, z], np.float64)
    ns('quaternion', as_rotation_matrix=as_rotation_matrix)
    ns('shapely')
    ns('shapely.geometry')
    ns('shapely.geometry.polygon', Polygon=Polygon)
    ns('trimesh')
    ns('plyfile', PlyData=None, PlyElement=None)
    ns('matplotlib')
    ns('matplotlib.pyplot', cm=types.SimpleNamespace(jet=None))
    for pkg in ('models', 'models/iscnet', 'external', 'net_utils', 'configs'):
        ns(pkg.replace('/', '.'), os.path.join(ref, pkg))
    ns('external.pointnet2_ops_lib')
    ns('external.pointnet2_ops_lib.pointnet2_ops')
    ns('external.pointnet2_ops_lib.pointnet2_ops.pointnet2_utils', furthest_point_sample=None, gather_operation=None)
    gen = importlib.import_module('utils.scannet.gen_scannet_w_orientation')
    loader = importlib.import_module('models.iscnet.dataloader')
    return gen, loader, importlib.import_module('configs.scannet_config').ScannetConfig


# ---- the scene ---------------------------------------------------------------------------------------------------------
def rotz(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.]])


def rotx(a):
    return np.array([[1., 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def quaternion_of(R):
    """a rotation matrix -> (w, x, y, z)"""
    w = np.sqrt(max(0., 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0., 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0., 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0., 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    q = np.array([w, x, y, z])
    k = int(np.argmax(q))
    sign = [None, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    other = {0: [None, sign[1], sign[2], sign[3]], 1: [sign[1], None, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
             2: [sign[2], R[0, 1] + R[1, 0], None, R[1, 2] + R[2, 1]], 3: [sign[3], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], None]}
    for j in range(4):
        if j != k and other[k][j] < 0:
            q[j] = -q[j]
    return q


# (catid, centre in the aligned frame, yaw, the model's half extents (x, y up, z forward), scale, tilt about x, vertices,
#  lying: the model's forward axis points up)
MODELS = [
    ('04379243', (0.00, 0.00, 0.50), 0.3, (0.50, 0.25, 0.30), (2.0, 2.0, 2.0), 0.00, 300, False),
    ('03001627', (0.30, 0.10, 0.50), -0.5, (0.30, 0.50, 0.40), (2.0, 1.0, 2.0), 0.03, 64, False),
    ('04256520', (-0.20, 0.20, 0.60), 1.0, (0.25, 0.30, 0.25), (2.0, 2.0, 2.0), -0.02, 1000, False),
    ('03001627', (0.10, -0.20, 0.40), 2.0, (0.40, 0.40, 0.40), (1.0, 1.0, 1.0), 0.00, 65, False),
    ('02818832', (2.00, -2.00, 0.30), 0.7, (0.50, 0.30, 1.00), (1.0, 1.0, 1.0), 0.00, 150, False),
    ('02933112', (2.20, 1.50, 0.40), -2.4, (0.30, 0.40, 0.20), (1.5, 1.0, 1.2), 0.01, 500, False),
    ('02871439', (-2.00, -1.80, 0.90), 2.9, (0.40, 0.15, 0.90), (1.0, 1.0, 1.0), 0.02, 200, True),
]


def build_scene(rng):
    axis_align = np.eye(4)
    axis_align[:3, :3], axis_align[:3, 3] = rotz(0.4), (-1.2, 0.7, -0.05)
    scan_trs = {'translation': [0.3, -0.2, 0.1], 'rotation': list(quaternion_of(rotz(-0.25))), 'scale': [1., 1., 1.]}
    Mscan = np.eye(4)
    Mscan[:3, :3], Mscan[:3, 3] = rotz(-0.25), scan_trs['translation']
    G = np.linalg.inv(axis_align.dot(np.linalg.inv(Mscan)))           # aligned frame -> the annotation's world
    models, vertices = [], {}
    for k, (catid, centre, yaw, half, scale, tilt, count, lying) in enumerate(MODELS):
        up = rotx(np.pi) if lying else rotx(np.pi / 2)                # the model's -z (forward) or its y goes up
        Rd = rotz(yaw).dot(rotx(tilt)).dot(up)
        R, t = G[:3, :3].dot(Rd), G[:3, :3].dot(centre) + G[:3, 3]
        id_cad = "model%02d" % k
        models.append({'catid_cad': catid, 'id_cad': id_cad,
                       'trs': {'translation': list(t), 'rotation': list(quaternion_of(R)), 'scale': list(scale)}})
        vertices[(catid, id_cad)] = rng.uniform(-1, 1, (count, 3)) * half
    return axis_align, scan_trs, models, vertices


def draw_points(rng, n):
    """n scan points: half of them in the block where four boxes overlap, the rest over the room"""
    room = rng.uniform((-3.2, -3.2, -0.05), (3.2, 3.2, 2.4), (n, 3))
    core = rng.uniform((-1.6, -1.6, -0.1), (1.6, 1.6, 1.4), (n, 3))
    return np.where((np.arange(n) % 2 == 0)[:, None], core, room).astype(np.float32)


def instance_ids_of(xyz):
    """five clustered instances (ids 1 .. 5), the rest background"""
    ids = np.zeros(len(xyz), np.uint32)
    regions = [((-0.9, -0.5, 0.0), (0.9, 0.5, 1.0)), ((-0.3, -0.7, 0.0), (0.9, 0.9, 1.0)),
               ((1.7, 1.1, 0.0), (2.7, 1.9, 0.8)), ((-2.5, -2.3, 0.0), (-1.5, -1.3, 1.8)),
               ((-3.0, 1.5, 0.0), (-2.0, 3.0, 1.0))]
    for k, (lo, hi) in reversed(list(enumerate(regions))):
        ids[np.all((xyz >= lo) & (xyz <= hi), 1)] = k + 1
    return ids


def instance_bboxes_of(vertices, ids, n):
    """what export() makes of the instances: centre and size per axis from the f32 columns, a label column"""
    out = np.zeros((n, 7))
    for i in range(1, n + 1):
        pc = vertices[ids == i, 0:3]
        if len(pc) == 0:
            continue
        lo, hi = [np.min(pc[:, a]) for a in range(3)], [np.max(pc[:, a]) for a in range(3)]
        out[i - 1] = np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2,
                               hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], np.uint32(1)])
    return out


def face_distance(xyz, box):
    """per point the distance to the nearest of the six planes that carry the faces of `box`"""
    d = xyz.astype(np.float64) - box[:3]
    c, s = np.cos(box[6]), np.sin(box[6])
    local = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
    return np.abs(np.abs(local) - box[3:6] / 2).min(1)


def inside(xyz, box):
    d = xyz.astype(np.float64) - box[:3]
    c, s = np.cos(box[6]), np.sin(box[6])
    local = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
    return np.all(np.abs(local) <= box[3:6] / 2, 1)


def run_generate(gen, tmp, annotation, cad_vertices, mesh_vertices, ids, bboxes):
    out_dir = os.path.join(tmp, "processed")
    os.makedirs(out_dir, exist_ok=True)
    for name in ("bbox.pkl", "full_scan.npz"):
        path = os.path.join(out_dir, SCENE, name)
        if os.path.exists(path):
            os.remove(path)
    gen.export = lambda *a, **k: (mesh_vertices.copy(), None, ids.copy(), bboxes.copy(), None)
    gen.read_obj = lambda path: {'v': cad_vertices[tuple(path.split(os.sep)[-4:-2])].copy()}
    mean_sizes = gen.generate(annotation)
    with open(os.path.join(out_dir, SCENE, "bbox.pkl"), "rb") as f:
        boxes = pickle.load(f)
    return boxes, dict(np.load(os.path.join(out_dir, SCENE, "full_scan.npz"))), mean_sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    rng = np.random.RandomState(2027)
    axis_align, scan_trs, models, cad_vertices = build_scene(rng)
    xyz = draw_points(rng, N_VERTICES)
    rgb = rng.randint(0, 256, (N_VERTICES, 3)).astype(np.float32)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen, loader, RefConfig = mount_reference(ref)
        meta_root = os.path.join(tmp, "meta")
        os.makedirs(os.path.join(meta_root, "scans", SCENE))
        with open(os.path.join(meta_root, "scans", SCENE, SCENE + ".txt"), "w") as f:
            f.write("axisAlignment = " + " ".join(repr(float(x)) for x in axis_align.reshape(-1)) + "\n")
        label_map = os.path.join(tmp, "label_map.pkl")
        with open(label_map, "wb") as f:
            pickle.dump({}, f)
        shapenet = os.path.join(tmp, "shapenet")
        for catid, id_cad in cad_vertices:
            os.makedirs(os.path.join(shapenet, catid, id_cad, "models"))
            open(os.path.join(shapenet, catid, id_cad, "models", "model_normalized.obj"), "w").close()
        os.makedirs(os.path.join(tmp, "processed"))
        gen.ShapeNetv2_path = shapenet
        gen.path_config = types.SimpleNamespace(processed_data_path=os.path.join(tmp, "processed"), metadata_root=meta_root,
                                                raw_label_map_file=label_map, OBJ_CLASS_IDS=gen.OBJ_CLASS_IDS)
        annotation = {'id_scan': SCENE, 'trs': scan_trs, 'aligned_models': models}
        for attempt in range(20):                                     # redraw what comes too close to a face plane
            mesh_vertices = np.concatenate([xyz, rgb], 1).astype(np.float32)
            ids = instance_ids_of(xyz)
            bboxes = instance_bboxes_of(mesh_vertices, ids, 5)
            boxes, scan, mean_sizes = run_generate(gen, tmp, annotation, cad_vertices, mesh_vertices, ids, bboxes)
            near = np.zeros(N_VERTICES, bool)
            for b in boxes:
                near |= face_distance(xyz, b['box3D']) <= FACE_MARGIN
            print("attempt %d: %d points within %g of a face plane" % (attempt, near.sum(), FACE_MARGIN))
            if not near.any():
                break
            xyz[near] = draw_points(rng, int(near.sum()))
        box3D = np.array([b['box3D'] for b in boxes])
        assert np.array_equal(scan['mesh_vertices'], mesh_vertices) and np.array_equal(scan['instance_labels'], ids)

        # ---- what the scene must show
        assert not near.any(), "a scan point lies within FACE_MARGIN of a face plane"
        assert len(boxes) == 6 and all(b['shapenet_catid'] != '02818832' for b in boxes), "the class filter"
        cover = sum(inside(xyz, b).astype(int) for b in box3D)
        assert all((cover == k).any() for k in (1, 2, 3, 4)), np.bincount(cover)
        assert np.array_equal(scan['point_votes'][:, 0], (cover > 0).astype(np.float64)), "Delaunay and the box test differ"
        ious = np.array([[gen.get_iou_cuboid(b['box_corners'], np.array(gen.get_box_corners(
            ib[:3], np.diag(ib[3:6]) / 2.))) for ib in bboxes] for b in boxes])
        ranked = np.sort(ious, 1)
        assert (ranked[:, -1] - ranked[:, -2] >= IOU_GAP).all(), ranked[:, -2:]
        print("coverage:", np.bincount(cover), "instance ids:", [b['instance_id'] for b in boxes])
        print("iou best / runner-up:", ranked[:, -1], ranked[:, -2])

        # ---- the dataloader
        classes = sorted(c for c in mean_sizes if len(mean_sizes[c]))
        mean_size_arr = np.ones((8, 3))
        for k, c in enumerate(gen.OBJ_CLASS_IDS):
            if len(mean_sizes[c]):
                mean_size_arr[k] = np.mean(mean_sizes[c], axis=0)
        dataset_config = RefConfig.__new__(RefConfig)
        dataset_config.num_heading_bin, dataset_config.class_ids = 12, gen.OBJ_CLASS_IDS
        dataset_config.shapenetid2class = {c: i for i, c in enumerate(list(gen.OBJ_CLASS_IDS))}
        dataset_config.mean_size_arr = mean_size_arr
        split_dir = os.path.join(tmp, "split")
        os.makedirs(split_dir)
        scene_dir = os.path.join(tmp, "processed", SCENE)
        for mode in ("train", "test"):
            with open(os.path.join(split_dir, "scannetv2_%s.json" % mode), "w") as f:
                json.dump([{'bbox': os.path.join(scene_dir, "bbox.pkl"), 'scan': os.path.join(scene_dir, "full_scan.npz")}], f)

        def sample(mode, color, seed):
            cfg = types.SimpleNamespace(dataset_config=dataset_config, config={
                'data': {'num_point': NUM_POINT, 'use_color_detection': color, 'use_color_completion': False,
                         'no_height': False, 'shapenet_path': shapenet, 'points_unpackbits': True,
                         'points_subsample': 2048, 'split': split_dir},
                mode: {'phase': 'detection'}})
            np.random.seed(seed)
            return loader.ISCNet_ScanNet(cfg, mode)[0]

        def draws(mode, seed):
            rs = np.random.RandomState(seed)
            flips, angle = (False, False), 0.
            if mode == 'train':
                flips = (rs.random_sample() > 0.5, rs.random_sample() > 0.5)
                angle = (rs.random_sample() * np.pi / 2) - np.pi / 4
            return flips, angle, rs.choice(N_VERTICES, NUM_POINT, replace=False)

        train_seed = next(s for s in range(1000) if all(draws('train', s)[0]))
        for mode, color, seed in (("test", False, 7), ("train", True, train_seed)):
            ret = sample(mode, color, seed)
            flips, angle, choices = draws(mode, seed)
            # the replayed draws are the reference's: the mask column is gathered untouched by any augmentation
            assert np.array_equal(ret['vote_label_mask'], scan['point_votes'][choices, 0].astype(np.int64))
            for key, value in ret.items():
                out["%s_%s" % (mode, key)] = np.asarray(value)
            out[mode + "_flips"], out[mode + "_angle"], out[mode + "_choices"] = np.array(flips), np.float64(angle), choices
            out[mode + "_seed"] = np.int64(seed)
            print(mode, "seed", seed, "flips", flips, "angle", angle, {k: (v.dtype, v.shape) for k, v in ret.items()})
        # the recorded draws are the reference's: the test-mode sample is a plain gather of the chosen rows
        assert np.array_equal(out["test_point_clouds"][:, :3], mesh_vertices[out["test_choices"], :3])

    out.update(vertices=mesh_vertices, instance_labels=ids, instance_bboxes=bboxes, axis_align=axis_align,
               scan_translation=np.array(scan_trs['translation']), scan_rotation=np.array(scan_trs['rotation']),
               scan_scale=np.array(scan_trs['scale']),
               model_catid=np.array([m['catid_cad'] for m in models]), model_id=np.array([m['id_cad'] for m in models]),
               model_translation=np.array([m['trs']['translation'] for m in models]),
               model_rotation=np.array([m['trs']['rotation'] for m in models]),
               model_scale=np.array([m['trs']['scale'] for m in models]),
               model_counts=np.array([len(cad_vertices[(m['catid_cad'], m['id_cad'])]) for m in models]),
               model_vertices=np.concatenate([cad_vertices[(m['catid_cad'], m['id_cad'])] for m in models]),
               box3D=box3D, cls_id=np.array([b['cls_id'] for b in boxes]),
               instance_id=np.array([b['instance_id'] for b in boxes]),
               box_corners=np.array([b['box_corners'] for b in boxes]),
               shapenet_catid=np.array([b['shapenet_catid'] for b in boxes]),
               shapenet_id=np.array([b['shapenet_id'] for b in boxes]),
               point_votes=scan['point_votes'], iou=ious,
               mean_sizes_cls=np.array([c for c in gen.OBJ_CLASS_IDS for _ in mean_sizes[c]]),
               mean_sizes_val=np.array([s for c in gen.OBJ_CLASS_IDS for s in mean_sizes[c]]).reshape(-1, 3),
               mean_size_arr=mean_size_arr, cover=cover.astype(np.int32), num_point=np.int64(NUM_POINT))
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
