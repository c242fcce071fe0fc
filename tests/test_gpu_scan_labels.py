"""GPU: rfdnet_amd.scan_labels (csrc/scan_labels.hip, the rules of include/rfd_labels.h) against numpy, against the
restatement tests/scan_labels_f64.py and against the reference's own output tests/golden/F_SCAN.npz, which
tests/test_scan_labels_cpu.py holds the restatement to.  Equality wherever the rule fixes the bits (instance boxes, rule
E, votes, the unaugmented sample); the derived bounds of scan_labels_f64's docstring elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_labels_f64 as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.U


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(None)


@pytest.fixture(scope="module")
def restated(fx):
    return ref.restate_boxes(fx)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda() if dtype is None else t.to("cuda", dtype)


# ---- instance boxes ------------------------------------------------------------------------------------------------------
def check_instance_boxes(xyz, ids, n):
    from rfdnet_amd.scan_labels import instance_boxes
    got = instance_boxes(dev(xyz), dev(ids.astype(np.int64)), n)
    assert got.dtype == np.float64 and got.shape == (n, 6)
    np.testing.assert_array_equal(got, ref.instance_boxes(xyz, ids, n))
    return got


def test_instance_aabb_several_workgroups_one_id_absent():
    """N = 3000: two workgroups of 2048 vertices, no multiple of 256; ids 0 .. 5 in runs (whole waves of one id) and
    shuffled (mixed waves), id 4 absent; six columns, so the stride is not 3"""
    rng = np.random.RandomState(11)
    v = (rng.randn(3000, 6) * [3, 3, 1, 50, 50, 50]).astype(np.float32)
    ids = np.sort(rng.choice([0, 1, 2, 3, 5], 3000))
    for order in (np.arange(3000), rng.permutation(3000)):
        got = check_instance_boxes(v[order], ids[order], 5)
        assert not got[3].any() and got[[0, 1, 2, 4]].any(1).all()
    assert np.array_equal(check_instance_boxes(v, ids, 7)[5:], np.zeros((2, 6)))        # ids above the largest present


def test_instance_aabb_many_instances_and_one_vertex():
    """I = 300: ids beyond the 256 rows a workgroup keeps in LDS go to memory directly; N = 1; negative coordinates"""
    rng = np.random.RandomState(12)
    v = (rng.randn(3000, 3) * 4).astype(np.float32)
    check_instance_boxes(v, rng.randint(0, 301, 3000), 300)
    check_instance_boxes(v, np.repeat(np.arange(300, 0, -1), 10), 300)
    got = check_instance_boxes(np.array([[-1.5, 2.25, -0.0]], np.float32), np.array([1]), 1)
    np.testing.assert_array_equal(got, [[-1.5, 2.25, 0, 0, 0, 0]])
    check_instance_boxes(v[:1], np.array([0]), 3)


def test_instance_boxes_of_the_fixture(fx):
    arrays = fx[0]
    got = check_instance_boxes(arrays['vertices'], arrays['instance_labels'], 5)
    np.testing.assert_array_equal(got, arrays['instance_bboxes'][:, :6])


# ---- CAD extents and boxes -----------------------------------------------------------------------------------------------
def test_cad_extents_ragged():
    """models of 1, 63, 64, 65, 500 and 5 000 vertices (the last one three runs of 2048): bit for bit rule E, and within
    3u S of the same L evaluated in extended precision; the one-vertex model has size 0"""
    from rfdnet_amd.scan_labels import cad_extents
    rng = np.random.RandomState(13)
    counts = [1, 63, 64, 65, 500, 5000]
    sets = [rng.randn(n, 3) * rng.uniform(0.1, 2, 3) for n in counts]
    L = rng.randn(len(counts), 3, 3)
    got = cad_extents(sets, L, 'cuda')
    assert got.shape == (6, 12) and got.dtype == np.float64
    for g, v, l in zip(got, sets, L):
        np.testing.assert_array_equal(g, ref.extents_rule(v, l))
        S = (np.abs(v) @ np.abs(l).T).max(0)
        err = np.abs(g - ref.extents_exact(v, l))
        print("%5d vertices: |L p - exact| / (3u S) = %s" % (len(v), err[6:] / (3 * U * np.tile(S, 2))))
        assert not err[:6].any() and (err[6:] <= 3 * U * np.tile(S, 2)).all()
    assert not (got[0, 3:6] - got[0, 0:3]).any() and not (got[0, 9:12] - got[0, 6:9]).any()
    with pytest.raises(ValueError, match="no vertex"):
        cad_extents([sets[0], np.zeros((0, 3))], L[:2], 'cuda')


def test_cad_boxes_of_the_fixture(fx, restated):
    """box3D, the class filter and mean_sizes: sizes within 16u S of the reference and of the restatement"""
    from rfdnet_amd.scan_labels import cad_boxes
    arrays, models, scan_trs = fx
    boxes, mean_sizes = cad_boxes(models, scan_trs, arrays['axis_align'])
    ref.check_cad_boxes(fx, restated, boxes, mean_sizes)
    only_bed = [m for m in models if m['catid_cad'] == '02818832']
    assert cad_boxes(only_bed, scan_trs, arrays['axis_align'])[0] == []


# ---- matching ------------------------------------------------------------------------------------------------------------
IOU_TOL = 1e-13      # the clip and the shoelace sum are a few dozen float64 operations on numbers of order 1: 100u ~ 1e-14


def test_match_closed_forms():
    from rfdnet_amd.scan_labels import match_instances
    unit = [0., 0., 0., 1., 1., 1.]
    cad = np.array([unit + [0.],                                  # identical to instance 1
                    [5., 5., 5., 1., 1., 1., 0.3],                # disjoint from everything
                    [0.5, 0., 0., 1., 1., 1., 0.],                # shifted by half: 0.5 / 1.5
                    [3., 0., 0., 1., 1., 1., np.pi / 4],          # unit square at 45 degrees inside a 2 x 2 square
                    [10., 0., 0., 1., 1., 1., 0.]])               # halfway between two equal instances
    inst = np.array([unit, [3., 0., 0., 2., 2., 1.], [9.5, 0., 0., 1., 1., 1.], [10.5, 0., 0., 1., 1., 1.],
                     [0., 0., 0., 0., 0., 0.]])                   # an empty instance's row of zeros
    ids, best, second = match_instances(cad, inst)
    assert list(ids) == [1, 0, 1, 2, 3]
    np.testing.assert_allclose(best, [1., 0., 1. / 3, 1. / 4, 1. / 3], rtol=0, atol=IOU_TOL)
    np.testing.assert_allclose(second, [0., 0., 0., 0., 1. / 3], rtol=0, atol=IOU_TOL)
    assert best[4] == second[4], "equal candidates: the first wins, the other is the runner-up"
    ids, best, second = match_instances(cad, np.zeros((0, 6)))
    assert not ids.any() and not best.any() and not second.any()


def test_match_many_instances_against_the_restatement():
    """130 instances: every lane of the wave holds several candidates; the winner and both IoUs are the restatement's"""
    from rfdnet_amd.scan_labels import match_instances
    rng = np.random.RandomState(14)
    cad = np.hstack([rng.uniform(-2, 2, (9, 3)), rng.uniform(0.5, 2, (9, 3)), rng.uniform(-np.pi, np.pi, (9, 1))])
    inst = np.hstack([rng.uniform(-2, 2, (130, 3)), rng.uniform(0.3, 2, (130, 3))])
    ids, best, second = match_instances(cad, inst)
    want_ids, iou = ref.match(cad, inst)
    ranked = np.sort(iou, 1)
    assert (ranked[:, -1] - ranked[:, -2] > 1e-9).all()
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_allclose(best, ranked[:, -1], rtol=0, atol=IOU_TOL)
    np.testing.assert_allclose(second, ranked[:, -2], rtol=0, atol=IOU_TOL)


def test_match_of_the_fixture(fx):
    from rfdnet_amd.scan_labels import match_instances
    arrays = fx[0]
    ids, best, second = match_instances(arrays['box3D'], arrays['instance_bboxes'])
    np.testing.assert_array_equal(ids, arrays['instance_id'])
    ranked = np.sort(arrays['iou'], 1)
    np.testing.assert_allclose(best, ranked[:, -1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(second, ranked[:, -2], rtol=0, atol=1e-12)


# ---- votes ---------------------------------------------------------------------------------------------------------------
def device_votes(vertices, boxes):
    from rfdnet_amd.scan_labels import point_votes
    votes, hits = point_votes(dev(vertices), boxes)
    assert votes.dtype == torch.float64 and hits.dtype == torch.int32
    return votes.cpu().numpy(), hits.cpu().numpy()


def test_votes_of_the_fixture(fx):
    """every point, bit for bit: the generator keeps every scan point more than 1e-6 m from every face plane"""
    arrays = fx[0]
    votes, hits = device_votes(arrays['vertices'], arrays['box3D'])
    np.testing.assert_array_equal(votes, arrays['point_votes'])
    np.testing.assert_array_equal(hits, arrays['cover'])


def test_votes_no_box_many_boxes_odd_sizes():
    rng = np.random.RandomState(15)
    xyz = rng.uniform(-1, 1, (257, 3)).astype(np.float32)             # 257: a second workgroup with one vertex
    votes, hits = device_votes(xyz, np.zeros((0, 7)))
    assert votes.shape == (257, 10) and not votes.any() and not hits.any()
    # 70 boxes (two rounds of 64), the first and the last five around the origin: 5- and 10-deep overlaps
    boxes = np.hstack([rng.uniform(-1, 1, (70, 3)), rng.uniform(0.2, 0.6, (70, 3)), rng.uniform(-3, 3, (70, 1))])
    boxes[:5, :3] = boxes[-5:, :3] = rng.uniform(-0.05, 0.05, (5, 3))
    boxes[:5, 3:6] = boxes[-5:, 3:6] = 1.5
    want, want_hits = ref.point_votes(xyz, boxes)
    near = np.zeros(len(xyz), bool)
    for b in boxes:
        d = xyz.astype(np.float64) - b[:3]
        c, s = np.cos(b[6]), np.sin(b[6])
        local = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
        near |= np.abs(np.abs(local) - b[3:6] / 2).min(1) <= 1e-9      # cos / sin may differ in the last bit
    assert not near.any() and want_hits.max() >= 10
    votes, hits = device_votes(xyz, boxes)
    np.testing.assert_array_equal(hits, want_hits)
    np.testing.assert_array_equal(votes, want)
    one, one_hits = device_votes(xyz[:1], boxes)
    np.testing.assert_array_equal(one, want[:1])


# ---- the sample ----------------------------------------------------------------------------------------------------------
def fixture_scan(arrays):
    boxes = [{'box3D': b, 'cls_id': int(c), 'instance_id': int(i), 'shapenet_catid': str(cat), 'shapenet_id': str(sid)}
             for b, c, i, cat, sid in zip(arrays['box3D'], arrays['cls_id'], arrays['instance_id'],
                                          arrays['shapenet_catid'], arrays['shapenet_id'])]
    scan = {'mesh_vertices': arrays['vertices'], 'point_votes': arrays['point_votes'],
            'instance_labels': arrays['instance_labels']}
    return scan, boxes


def make_fixture_sample(arrays, mode, **kw):
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.scan_labels import make_sample
    cfg = Config({'data': {'num_point': int(arrays['num_point']), 'use_color_detection': mode == 'train'}},
                 mean_size_arr=arrays['mean_size_arr'])
    scan, boxes = fixture_scan(arrays)
    out = make_sample(scan, boxes, cfg, mode, **kw)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def test_sample_test_mode_is_the_references(fx):
    """a gather, the height column and casts: every array bit for bit, the draws taken from the RandomState"""
    arrays = fx[0]
    got = make_fixture_sample(arrays, 'test', rng=np.random.RandomState(int(arrays['test_seed'])))
    assert set(got) == set(ref.SAMPLE_KEYS)
    ref.check_sample(got, ref.reference_sample(arrays, 'test'), exact=True)
    again = make_fixture_sample(arrays, 'test', choices=arrays['test_choices'], instance_labels=True)
    ref.check_sample(again, ref.reference_sample(arrays, 'test'), exact=True)
    assert np.array_equal(again['point_instance_labels'],
                          arrays['instance_labels'][arrays['test_choices']].astype(np.float32))


def test_sample_train_mode_within_one_ulp(fx):
    """both flips, the rotation, colour and height: the rotated arrays within one float32 ulp per element (the routes
    differ by float64 roundings before the one rounding to float32), index and mask arrays equal; and the float64
    restatement of the same steps agrees with the kernel to the same ulp"""
    arrays = fx[0]
    want = ref.reference_sample(arrays, 'train')
    got = make_fixture_sample(arrays, 'train', rng=np.random.RandomState(int(arrays['train_seed'])))
    for k in ('point_clouds', 'vote_label'):
        err = np.abs(got[k].astype(np.float64) - want[k]) / ref.ulp32(want[k])
        print("%s: largest error %.3g ulp, %d of %d elements differ" % (k, err.max(), (err > 0).sum(), err.size))
    ref.check_sample(got, want, exact=False)
    np.testing.assert_array_equal(got['point_clouds'][:, 3:], want['point_clouds'][:, 3:])      # colour and height: exact
    explicit = make_fixture_sample(arrays, 'train', choices=arrays['train_choices'], flips=arrays['train_flips'],
                                   rot_angle=float(arrays['train_angle']))
    for k in got:
        np.testing.assert_array_equal(explicit[k], got[k])


def test_sample_rejects_what_it_cannot_hold(fx):
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.scan_labels import make_sample
    arrays = fx[0]
    scan, boxes = fixture_scan(arrays)
    cfg = Config({'data': {'num_point': 16}}, mean_size_arr=arrays['mean_size_arr'])
    with pytest.raises(ValueError, match="MAX_NUM_OBJ = 64"):
        make_sample(scan, boxes * 11, cfg, 'test', choices=np.arange(16))
    with pytest.raises(ValueError, match="choices outside"):
        make_sample(scan, boxes, cfg, 'test', choices=np.array([0, 5000]))
    with pytest.raises(ValueError, match="pass rng"):
        make_sample(scan, boxes, cfg, 'train', choices=np.arange(16))


# ---- the whole way -------------------------------------------------------------------------------------------------------
def test_prepare_scan_is_the_references(fx, restated):
    from rfdnet_amd.scan_labels import prepare_scan
    arrays, models, scan_trs = fx
    boxes, scan, mean_sizes = prepare_scan(dev(arrays['vertices']), dev(arrays['instance_labels'].astype(np.int64)), models,
                                           scan_trs, arrays['axis_align'])
    ref.check_cad_boxes(fx, restated, boxes, mean_sizes)
    assert [b['instance_id'] for b in boxes] == list(arrays['instance_id'])
    assert np.abs(np.array([b['box_corners'] for b in boxes]) - arrays['box_corners']).max() < 1e-14
    np.testing.assert_array_equal(scan['mesh_vertices'], arrays['vertices'])
    np.testing.assert_array_equal(scan['instance_labels'], arrays['instance_labels'])
    assert scan['instance_labels'].dtype == np.uint32 and scan['point_votes'].dtype == np.float64
    # the boxes differ from the reference's in the last bits, so a vote may: the mask must not, the votes by 1e-14
    np.testing.assert_array_equal(scan['point_votes'][:, 0], arrays['point_votes'][:, 0])
    assert np.abs(scan['point_votes'] - arrays['point_votes']).max() < 1e-14
    only_bed = [m for m in models if m['catid_cad'] == '02818832']
    assert prepare_scan(dev(arrays['vertices']), dev(arrays['instance_labels'].astype(np.int64)), only_bed, scan_trs,
                        arrays['axis_align']) is None


def test_round_trip_to_the_vote_loss(fx, tmp_path):
    """tools/make_scan_labels.py's file, read the way demo.py --gt reads it, feeds the existing vote loss: finite, and
    equal to the loss from the reference's own arrays"""
    import pickle
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scan_labels
    from rfdnet_amd.iscnet.loss import compute_vote_loss
    arrays = fx[0]
    scan, boxes = fixture_scan(arrays)
    np.savez(tmp_path / "full_scan.npz", **scan)
    with open(tmp_path / "bbox.pkl", "wb") as f:
        pickle.dump(boxes, f)
    np.savez(tmp_path / "means.npz", arr_0=arrays['mean_size_arr'])
    out = tmp_path / "scan_labels.npz"
    make_scan_labels.main(["--scan", str(tmp_path / "full_scan.npz"), "--bbox", str(tmp_path / "bbox.pkl"),
                           "--mean_size_npz", str(tmp_path / "means.npz"), "--num_point", "2048", "--seed", "7",
                           "--out", str(out)])
    gt = np.load(out)
    for k in ref.SAMPLE_KEYS + ('point_instance_labels', 'object_instance_labels'):
        assert k in gt.files, k
    np.testing.assert_array_equal(gt['vote_label'], arrays['test_vote_label'])           # seed 7, 2048 points: the fixture's
    np.testing.assert_array_equal(gt['vote_label_mask'], arrays['test_vote_label_mask'])
    np.testing.assert_array_equal(gt['point_clouds'], arrays['test_point_clouds'])

    def as_demo_reads(source, k, prefix=""):                                             # demo.py: one scan gets a batch axis
        a = np.asarray(source[prefix + k])
        per_scan = 2 if k == 'vote_label' else 1
        return torch.from_numpy(a[None] if a.ndim == per_scan else a).cuda()
    gen = torch.Generator().manual_seed(3)
    S = 256
    inds = torch.randperm(2048, generator=gen)[:S].to(torch.int32)
    seed_xyz = torch.from_numpy(arrays['test_point_clouds'][:, :3])[inds.long()]
    est = {'seed_xyz': seed_xyz[None].cuda(), 'seed_inds': inds[None].cuda(),
           'vote_xyz': (seed_xyz + 0.1 * torch.randn(S, 3, generator=gen))[None].cuda()}
    mine = compute_vote_loss(est, {k: as_demo_reads(gt, k) for k in ('vote_label', 'vote_label_mask')})
    theirs = compute_vote_loss(est, {k: as_demo_reads(arrays, k, 'test_') for k in ('vote_label', 'vote_label_mask')})
    assert torch.isfinite(mine) and float(mine) > 0 and float(mine) == float(theirs)


def test_prepare_scan_tool_from_files(fx, tmp_path):
    """tools/prepare_scan.py from a .npz scan, an id array, an annotation JSON, a meta file and .obj models: the files
    the reference writes.  The tool aligns the vertices itself, so the scan goes in un-aligned (the inverse alignment
    applied in float64) and comes back within float32 rounding of the fixture's; boxes, ids and the vote mask of every
    point more than 1e-5 m from a face plane are the fixture's.  A scan whose models are all outside the filter writes
    nothing."""
    import json
    import pickle
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prepare_scan
    arrays, models, scan_trs = fx
    inv = np.linalg.inv(arrays['axis_align'])
    raw = arrays['vertices'].copy()
    raw[:, :3] = (arrays['vertices'][:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    np.savez(tmp_path / "scan.npz", vertices=raw)
    np.save(tmp_path / "ids.npy", arrays['instance_labels'])
    with open(tmp_path / "meta.txt", "w") as f:
        f.write("axisAlignment = " + " ".join(repr(float(x)) for x in arrays['axis_align'].reshape(-1)) + "\n")
    entry = {'id_scan': 'scene', 'trs': {k: list(map(float, v)) for k, v in scan_trs.items()}, 'aligned_models': []}
    for m in models:
        d = tmp_path / "shapenet" / m['catid_cad'] / m['id_cad'] / "models"
        os.makedirs(d)
        with open(d / "model_normalized.obj", "w") as f:
            f.writelines("v %r %r %r\n" % tuple(float(t) for t in p) for p in m['vertices'])
        entry['aligned_models'].append({'catid_cad': m['catid_cad'], 'id_cad': m['id_cad'],
                                        'trs': {k: list(map(float, v)) for k, v in m['trs'].items()}})
    with open(tmp_path / "annotation.json", "w") as f:
        json.dump([{'id_scan': 'other', 'trs': entry['trs'], 'aligned_models': []}, entry], f)
    common = ["--scan", str(tmp_path / "scan.npz"), "--instance_ids", str(tmp_path / "ids.npy"),
              "--meta", str(tmp_path / "meta.txt"), "--shapenet", str(tmp_path / "shapenet")]
    out_dir = tmp_path / "out"
    assert prepare_scan.main(common + ["--annotation", str(tmp_path / "annotation.json"), "--id_scan", "scene",
                                       "--out_dir", str(out_dir)]) == str(out_dir)
    with open(out_dir / "bbox.pkl", "rb") as f:
        boxes = pickle.load(f)
    scan = np.load(out_dir / "full_scan.npz")
    assert [b['shapenet_id'] for b in boxes] == list(arrays['shapenet_id'])
    assert np.abs(np.array([b['box3D'] for b in boxes]) - arrays['box3D']).max() < 1e-12      # .obj text keeps the bits
    assert [b['instance_id'] for b in boxes] == list(arrays['instance_id'])
    assert np.abs(scan['mesh_vertices'][:, :3] - arrays['vertices'][:, :3]).max() < 2e-6       # two f32 roundings at < 4 m
    np.testing.assert_array_equal(scan['mesh_vertices'][:, 3:], arrays['vertices'][:, 3:])
    np.testing.assert_array_equal(scan['instance_labels'], arrays['instance_labels'])
    clear = np.ones(len(raw), bool)
    for b in arrays['box3D']:
        d = arrays['vertices'][:, :3].astype(np.float64) - b[:3]
        c, s = np.cos(b[6]), np.sin(b[6])
        local = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
        clear &= np.abs(np.abs(local) - b[3:6] / 2).min(1) > 1e-5
    assert clear.sum() > 4900
    np.testing.assert_array_equal(scan['point_votes'][clear, 0], arrays['point_votes'][clear, 0])
    sizes = np.load(out_dir / "mean_sizes.npz")
    assert list(sizes['cls_id']) == list(arrays['mean_sizes_cls']) and sizes['size'].shape == (6, 3)
    entry['aligned_models'] = [m for m in entry['aligned_models'] if m['catid_cad'] == '02818832']
    with open(tmp_path / "bed.json", "w") as f:
        json.dump(entry, f)
    assert prepare_scan.main(common + ["--annotation", str(tmp_path / "bed.json"), "--out_dir", str(tmp_path / "none")]) is None
    assert not os.path.exists(tmp_path / "none")
