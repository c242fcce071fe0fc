"""CPU: the numpy restatement of the scan ground truth (tests/scan_labels_f64.py) against the reference's own output
(tests/golden/F_SCAN.npz), and the host-only parts of rfdnet_amd/scan_labels.py (matrices, rectification, the 64-row
label arrays, the percentile plan, the order of the random draws) against the same fixture.  The bounds are those
derived in scan_labels_f64's docstring; nothing here is measured."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_labels_f64 as ref  # noqa: E402
from rfdnet_amd import scan_labels as sl  # noqa: E402
from rfdnet_amd.iscnet.config import Config  # noqa: E402

U = ref.U


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(None)


@pytest.fixture(scope="module")
def restated(fx):
    return ref.restate_boxes(fx)


def test_fixture_shows_what_it_must(fx):
    arrays = fx[0]
    assert arrays['vertices'].shape == (5000, 6) and arrays['vertices'].dtype == np.float32
    assert len(arrays['model_counts']) == 7 and len(arrays['box3D']) == 6
    assert '02818832' in arrays['model_catid'] and '02818832' not in arrays['shapenet_catid']
    assert all((arrays['cover'] == k).any() for k in (1, 2, 3, 4))
    ranked = np.sort(arrays['iou'], 1)
    assert (ranked[:, -1] - ranked[:, -2] >= 1e-9).all()
    assert arrays['train_flips'].all() and arrays['train_angle'] != 0


def test_instance_boxes_restated(fx):
    arrays = fx[0]
    got = ref.instance_boxes(arrays['vertices'], arrays['instance_labels'], 5)
    assert np.array_equal(got, arrays['instance_bboxes'][:, :6])


def test_cad_boxes_restated(fx, restated):
    arrays, models, _ = fx
    keep, classes, boxes, Ts = restated
    assert [models[k]['catid_cad'] for k in keep] == list(arrays['shapenet_catid'])
    assert classes == list(arrays['cls_id'])
    for k, (box, order, _), T, want in zip(keep, boxes, Ts, arrays['box3D']):
        v = models[k]['vertices']
        assert (np.abs(box[3:6] - want[3:6]) <= ref.route_bound(v, T)).all(), (k, box[3:6] - want[3:6])
        assert (np.abs(box[:3] - want[:3]) <= ref.centre_bound(v, T)).all(), (k, box[:3] - want[:3])
        assert abs(box[6] - want[6]) <= 16 * U * np.pi, (k, box[6] - want[6])
    assert boxes[-1][1] == [1, 2, 0], "the last model lies on its back: its forward axis is the box's z"
    assert all(b[1] == [0, 1, 2] for b in boxes[:-1])


def test_match_restated(fx):
    arrays = fx[0]
    ids, iou = ref.match(arrays['box3D'], arrays['instance_bboxes'])
    assert np.array_equal(ids, arrays['instance_id'])
    assert np.abs(iou - arrays['iou']).max() <= 1e-12          # two clippers, a few dozen roundings each


def test_votes_restated(fx):
    arrays = fx[0]
    votes, hits = ref.point_votes(arrays['vertices'], arrays['box3D'])
    assert np.array_equal(votes, arrays['point_votes'])
    assert np.array_equal(hits, arrays['cover'])
    assert hits.max() == 4


@pytest.mark.parametrize("mode", ["test", "train"])
def test_sample_restated(fx, mode):
    arrays = fx[0]
    train = mode == "train"
    got = ref.sample(arrays['vertices'], arrays['point_votes'], arrays['instance_labels'], arrays['box3D'],
                     arrays['cls_id'], arrays['instance_id'], arrays['mean_size_arr'], arrays[mode + '_choices'], train,
                     arrays[mode + '_flips'], float(arrays[mode + '_angle']), use_color=train)
    ref.check_sample(got, ref.reference_sample(arrays, mode), exact=not train)


# ---- the host side of rfdnet_amd/scan_labels.py --------------------------------------------------------------------------
def test_host_matrices_and_rectification(fx, restated):
    arrays, models, scan_trs = fx
    keep, _, boxes, Ts = restated
    for k, (_, order, axes), T in zip(keep, boxes, Ts):
        mine = np.asarray(arrays['axis_align']).dot(np.linalg.inv(sl.matrix_from_trs(scan_trs))).dot(
            sl.matrix_from_trs(models[k]['trs']))
        assert np.abs(mine - T).max() <= 32 * U * max(1., np.abs(T).max())
        got_order, yaw = sl.rectify(axes)
        assert got_order == order
    assert [sl.class_of(m['catid_cad']) for m in models] == [1, 7, 13, 7, None, 31, 8]
    assert np.array_equal(sl.box_corners(arrays['box3D'][0]), arrays['box_corners'][0])


def test_one_pass_boxes_on_the_host(fx, restated, monkeypatch):
    """cad_boxes with rule E evaluated in numpy in place of the kernel: the one-pass form L (p - c) stays inside the
    bound the kernel is held to, against the reference and against the restatement of its two-pass route"""
    arrays, models, scan_trs = fx
    monkeypatch.setattr(sl, "cad_extents", lambda sets, L, device: np.array(
        [ref.extents_rule(v, l) for v, l in zip(sets, L)]))
    boxes, mean_sizes = sl.cad_boxes(models, scan_trs, arrays['axis_align'], device='cpu')
    ref.check_cad_boxes(fx, restated, boxes, mean_sizes)
    for v, T in zip([models[k]['vertices'] for k in restated[0]], restated[3]):
        L = np.array([sl.unit(-T[:3, 2]), sl.unit(-T[:3, 0]), sl.unit(T[:3, 1])]).dot(T[:3, :3])
        S = np.abs(v) @ np.abs(L).T
        assert (np.abs(ref.extents_rule(v, L) - ref.extents_exact(v, L))[6:] <= 3 * U * np.tile(S.max(0), 2)).all()


@pytest.mark.parametrize("mode", ["test", "train"])
def test_host_label_arrays(fx, mode):
    arrays = fx[0]
    cfg = Config(mean_size_arr=arrays['mean_size_arr'])
    box3D = arrays['box3D']
    if mode == "train":
        box3D = sl.augment_boxes(box3D, arrays['train_flips'], float(arrays['train_angle']))
    got = sl.box_labels(box3D, arrays['cls_id'], arrays['instance_id'], cfg.dataset_config)
    want = {k: v for k, v in ref.reference_sample(arrays, mode).items() if k in got}
    assert len(want) == 7
    ref.check_sample(got, want, exact=mode == "test")
    assert got['object_instance_labels'].dtype == np.float32
    assert np.array_equal(got['object_instance_labels'][:6], arrays['instance_id'])
    assert not got['object_instance_labels'][6:].any()


def test_angle2class():
    cfg = Config(mean_size_arr=np.ones((8, 3))).dataset_config
    angles = np.array([0., np.pi / 12 - 1e-9, np.pi / 12 + 1e-9, -np.pi, np.pi, 3.0, -0.2, 2 * np.pi - 1e-12])
    cls, res = cfg.angle2class(angles)
    assert cls.dtype == np.int16 and list(cls) == [0, 0, 1, 6, 6, 6, 0, 0]
    assert np.abs((cls * (np.pi / 6) + res - angles % (2 * np.pi) + np.pi) % (2 * np.pi) - np.pi).max() < 1e-12
    assert (res >= -np.pi / 12).all() and (res < np.pi / 12).all()
    assert cfg.shapenetid2class == {1: 0, 7: 1, 8: 2, 13: 3, 20: 4, 31: 5, 34: 6, 43: 7}


def test_percentile_plan_is_numpys():
    """floor_height interpolates two order statistics as np.percentile(x, 0.99) does on float32: dtype and bits"""
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 100, 101, 102, 203, 5000, 80000, 150001):
        z = rng.randn(n).astype(np.float32) * 3
        lo, hi, gamma = sl.percentile_plan(n)
        s = np.sort(z)
        assert gamma.dtype == np.float32
        got = sl.lerp(s[lo], s[hi], gamma[()])
        want = np.percentile(z, 0.99)
        assert want.dtype == np.float32 and got == want, (n, got, want)


def test_draws_are_the_dataloaders(fx):
    arrays = fx[0]
    for mode in ("test", "train"):
        flips, angle, choices = sl.draw(np.random.RandomState(int(arrays[mode + '_seed'])), 5000,
                                        int(arrays['num_point']), mode == "train")
        assert list(flips) == list(arrays[mode + '_flips']) and angle == float(arrays[mode + '_angle'])
        assert np.array_equal(choices, arrays[mode + '_choices'])


def test_mean_size_array(fx):
    arrays = fx[0]
    sizes = {c: [s for cc, s in zip(arrays['mean_sizes_cls'], arrays['mean_sizes_val']) if cc == c] for c in sl.OBJ_CLASS_IDS}
    got = sl.mean_size_array([sizes, None])
    have = ~np.isnan(got[:, 0])
    assert list(have) == [True, True, True, True, False, True, False, False]
    assert np.array_equal(got[have], arrays['mean_size_arr'][have])


def test_guards_without_a_gpu(fx):
    import torch
    arrays = fx[0]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        sl.instance_boxes(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        sl.point_votes(torch.zeros(4, 3), np.zeros((1, 7)))
    boxes = [{'box3D': arrays['box3D'][0], 'cls_id': 1, 'instance_id': 0}] * 65
    scan = {'mesh_vertices': arrays['vertices'], 'point_votes': arrays['point_votes'],
            'instance_labels': arrays['instance_labels']}
    with pytest.raises(ValueError, match="MAX_NUM_OBJ = 64"):
        sl.make_sample(scan, boxes, Config(mean_size_arr=np.ones((8, 3))), 'test', choices=np.arange(8))


def test_completion_labels_from_the_sampling_tools_files(tmp_path):
    """the completion keys of __getitem__ from the files tools/sample_mesh.py writes: padded to 64 objects, the first
    n points in test mode (SubsamplePoints), every point for the IoU keys, the voxels as float32"""
    from rfdnet_amd import io
    rng = np.random.RandomState(9)
    boxes, want = [], []
    for k, catid in enumerate(('03001627', '04379243')):
        pts = rng.uniform(-0.55, 0.55, (40, 3))
        occ = rng.rand(40) > 0.5
        vox = rng.rand(16, 16, 16) > 0.7
        for sub in ('point', os.path.join('voxel', '16')):
            os.makedirs(tmp_path / sub / catid, exist_ok=True)
        io.write_points_npz(str(tmp_path / 'point' / catid / ('m%d.npz' % k)), pts, occ, np.zeros(3), 1., float16=True,
                            packbits=True)
        io.write_binvox(str(tmp_path / 'voxel' / '16' / catid / ('m%d.binvox' % k)), vox, [0, 0, 0], 1.)
        boxes.append({'shapenet_catid': catid, 'shapenet_id': 'm%d' % k})
        want.append((pts.astype(np.float16).astype(np.float32), occ.astype(np.float32), vox.astype(np.float32)))
    got = sl.completion_labels(boxes, str(tmp_path), 8, 'test', None)
    assert sorted(got) == ['object_points', 'object_points_iou', 'object_points_iou_occ', 'object_points_occ',
                           'object_voxels', 'shapenet_catids', 'shapenet_ids']
    assert got['object_points'].shape == (64, 8, 3) and got['object_points_iou'].shape == (64, 40, 3)
    assert got['object_voxels'].shape == (64, 16, 16, 16) and got['object_points_occ'].shape == (64, 8)
    assert all(got[k].dtype == np.float32 for k in got if k.startswith('object'))
    for k, (pts, occ, vox) in enumerate(want):
        assert np.array_equal(got['object_points'][k], pts[:8]) and np.array_equal(got['object_points_occ'][k], occ[:8])
        assert np.array_equal(got['object_points_iou'][k], pts) and np.array_equal(got['object_points_iou_occ'][k], occ)
        assert np.array_equal(got['object_voxels'][k], vox)
    assert not got['object_points'][2:].any() and not got['object_voxels'][2:].any()
    assert got['shapenet_catids'] == ['03001627', '04379243'] and got['shapenet_ids'] == ['m0', 'm1']
    train = sl.completion_labels(boxes, str(tmp_path), 8, 'train', np.random.RandomState(1))
    assert 'object_points_iou' not in train and train['object_points'].shape == (64, 8, 3)
    rs = np.random.RandomState(1)
    noisy = want[0][0] + 1e-4 * rs.randn(40, 3)          # float16 points in train mode: the symmetry breaker, then the draw
    assert np.array_equal(train['object_points'][0], noisy.astype(np.float32)[rs.randint(40, size=8)])


def test_read_scan_ply(tmp_path):
    """a scanner's PLY (float xyz, uchar rgba, faces after the vertices), binary and ascii -> (N,6) float32"""
    from rfdnet_amd import io
    rng = np.random.RandomState(2)
    xyz, rgba = rng.randn(5, 3).astype(np.float32), rng.randint(0, 256, (5, 4)).astype(np.uint8)
    head = ("ply\nformat %s 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    rec = np.empty(5, dtype=[('p', '<f4', (3,)), ('c', 'u1', (4,))])
    rec['p'], rec['c'] = xyz, rgba
    with open(tmp_path / "b.ply", "wb") as f:
        f.write((head % "binary_little_endian").encode() + rec.tobytes() + bytes([3]) + np.array([0, 1, 2], '<i4').tobytes())
    with open(tmp_path / "a.ply", "w") as f:
        f.write(head % "ascii")
        for p, c in zip(xyz, rgba):
            f.write(" ".join(repr(float(t)) for t in p) + " " + " ".join(str(int(t)) for t in c) + "\n")
        f.write("3 0 1 2\n")
    want = np.concatenate([xyz, rgba[:, :3].astype(np.float32)], 1)
    for name in ("b.ply", "a.ply"):
        got = io.read_scan_ply(str(tmp_path / name))
        assert got.dtype == np.float32 and np.array_equal(got, want), name
