"""GPU (-m gpu): rfd_objgrid_pack / rfd_mesh_iou_counts / rfd_mesh_iou_finalize (csrc/mesh_iou.hip) and
rfdnet_amd.iscnet.mesh_eval against the reference's own results (tests/golden/F_MIOU.npz) and the restatement
tests/mesh_iou_f64.py.

No tolerance anywhere: the lookup counts are integers, and the IoU is five correctly rounded float64 operations on
them in the order of rule M5 -- the kernel, the restatement and the reference must agree to the bit.  The voxel grids of
voxelize_objects are held, bit for bit, to the restatement built on tests/mesh_sample_ref.py, as the voxelisers
themselves are (tests/test_gpu_mesh_sample.py)."""
import os

import numpy as np
import pytest
import torch

import eval_det_f64 as E
import mesh_iou_f64 as M

pytestmark = pytest.mark.gpu
THR = (0.25, 0.5)
SETTINGS = (("pcp1", True), ("pcp0", False))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "F_MIOU.npz"))


@pytest.fixture(scope="module")
def objs(fx):
    return M.fixture_objects(fx)


@pytest.fixture(scope="module")
def all_pairs(objs):
    """every fixture object, and one without a grid, against every other: the restatement, computed once"""
    everything = objs + [M.Obj()]
    return everything, M.iou_matrix(everything, everything)


def as_entries(objects):
    return [None if o.U is None else (o.S, o.I, o.lo, o.cell) for o in objects]


def test_pack_counts_finalize_equal_the_reference(hip, fx, objs):
    from rfdnet_amd.iscnet import mesh_eval
    for s in range(fx['pred_obj'].shape[0]):
        pi, gi = fx['pred_obj'][s], fx['gt_obj'][s]
        pi, gi = pi[pi >= 0], gi[gi >= 0]
        pg = mesh_eval.pack_grids(as_entries([objs[i] for i in pi]), "cuda")
        gg = mesh_eval.pack_grids(as_entries([objs[i] for i in gi]), "cuda")
        iou, counts = mesh_eval.mesh_iou(pg, gg)
        P, G = len(pi), len(gi)
        print("scene %d: %d x %d pairs, D %s x %s" % (s, P, G, pg.dims.tolist(), gg.dims.tolist()))
        np.testing.assert_array_equal(counts.cpu().numpy(), fx['counts'][s, :P, :G])
        assert iou.cpu().numpy().tobytes() == np.ascontiguousarray(fx['mesh_iou'][s, :P, :G]).tobytes()
    assert hip.stream_status_bits() == 0


def test_packed_words_and_counts(hip, objs):
    from rfdnet_amd.iscnet import mesh_eval
    grids = mesh_eval.pack_grids(as_entries(objs), "cuda")
    words = grids.words.cpu().numpy().view(np.uint64)
    off = grids.off.cpu().numpy()
    cnt = grids.cnt.cpu().numpy()
    assert {2, 63, 64, 65, 130} <= set(grids.dims.tolist())                  # the word boundary, three words per row
    for i, o in enumerate(objs):
        want = M.pack_words(o.U)
        np.testing.assert_array_equal(words[off[i]:off[i] + len(want)], want)
        assert tuple(cnt[i]) == (int(o.U.sum()), int(o.S.sum()))
    assert grids.n_words == sum(len(M.pack_words(o.U)) for o in objs)


def test_every_object_against_every_other(hip, all_pairs):
    """self pairs (exactly 1), disjoint cubes (the early-out), nested, incommensurate, ties, empty S / I, no grid"""
    from rfdnet_amd.iscnet import mesh_eval
    everything, (want_iou, want_cnt) = all_pairs
    grids = mesh_eval.pack_grids(as_entries(everything), "cuda")
    iou, counts = mesh_eval.mesh_iou(grids, grids)
    iou, counts = iou.cpu().numpy(), counts.cpu().numpy()
    np.testing.assert_array_equal(counts, want_cnt)
    assert iou.tobytes() == want_iou.tobytes()
    n = len(everything)
    has_surface = np.array([o.U is not None and o.S.any() for o in everything])
    assert (np.diag(iou)[has_surface] == 1.0).all() and (np.diag(iou)[~has_surface] == 0.0).all()
    assert (iou[-1] == 0).all() and (iou[:, -1] == 0).all() and (counts[-1] == 0).all()       # the object without grid
    assert (counts[:, :, 0] == counts[:, :, 1].T).all() and (want_iou > 0).sum() > n          # a_AB of (p, g) is a_BA of (g, p)
    # scattered into a larger matrix: rows and columns permuted, one row out of range; the rest stays untouched
    K, G = n + 3, n + 2
    rows = np.random.default_rng(3).permutation(K)[:n].astype(np.int32)
    cols = np.random.default_rng(4).permutation(G)[:n].astype(np.int32)
    rows[2] = K                                                                # skipped
    out = torch.full((K, G), -7.0, dtype=torch.float64, device="cuda")
    mesh_eval.scatter_iou(grids, grids, torch.from_numpy(counts).cuda(), out, rows, cols)
    want = np.full((K, G), -7.0)
    keep = rows < K
    want[np.ix_(rows[keep], cols)] = want_iou[keep]
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_no_predictions_or_no_ground_truths(hip, objs):
    from rfdnet_amd.iscnet import mesh_eval
    some = mesh_eval.pack_grids(as_entries(objs[:3]), "cuda")
    none = mesh_eval.pack_grids([], "cuda")
    for a, b in ((none, some), (some, none), (none, none)):
        iou, counts = mesh_eval.mesh_iou(a, b)
        assert tuple(iou.shape) == (len(a), len(b)) and tuple(counts.shape) == (len(a), len(b), 2)
    assert hip.stream_status_bits() == 0


def test_refusals_launch_nothing(hip, objs):
    """hipErrorInvalidValue before anything is queued: the buffers are never touched (they hold a sentinel)"""
    from rfdnet_amd.iscnet import mesh_eval
    dev = torch.device("cuda")
    S = torch.ones(2, 2, 2, dtype=torch.uint8, device=dev)
    words = torch.full((64,), 5, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), 9, dtype=torch.int32, device=dev)
    for D, off, n_words in ((1, 0, 64), (257, 0, 64), (0, 0, 64), (-3, 0, 64), (2, -1, 64), (2, 61, 64), (2, 0, 3), (2, 0, -1)):
        with pytest.raises(hip.RfdHipError):
            hip.call("rfd_objgrid_pack", dev, D, S.data_ptr(), S.data_ptr(), words.data_ptr(), off, n_words, cnt.data_ptr())
    g = mesh_eval.pack_grids(as_entries(objs[:2]), dev)
    counts = torch.full((4,), 9, dtype=torch.int32, device=dev)
    args = lambda P, G: (P, G, g.frame.data_ptr(), g.dim.data_ptr(), g.off.data_ptr(), g.words.data_ptr(), g.n_words,
                         g.frame.data_ptr(), g.dim.data_ptr(), g.off.data_ptr(), g.words.data_ptr(), g.n_words,
                         counts.data_ptr())
    iou = torch.full((4,), 9.0, dtype=torch.float64, device=dev)
    for P, G in ((1025, 1), (1, 257), (-1, 1), (1, -1)):
        with pytest.raises(hip.RfdHipError):
            hip.call("rfd_mesh_iou_counts", dev, *args(P, G))
        with pytest.raises(hip.RfdHipError):
            hip.call("rfd_mesh_iou_finalize", dev, P, G, counts.data_ptr(), g.cnt.data_ptr(), g.cnt.data_ptr(), None, None,
                     1, 1, iou.data_ptr())
    with pytest.raises(ValueError):                                           # the host refuses D > 256 before any launch
        mesh_eval.pack_grids([(np.zeros((257,) * 3, bool), np.zeros((257,) * 3, bool), np.zeros(3), 0.1)], dev)
    torch.cuda.synchronize()
    assert (words == 5).all() and (cnt == 9).all() and (counts == 9).all() and (iou == 9).all()
    # a table row that is out of range is an object without grid, not a read outside the buffer
    bad = mesh_eval.pack_grids(as_entries(objs[:2]), dev)
    bad.dim[0] = 300
    bad.off[1] = bad.n_words
    _, c = mesh_eval.mesh_iou(bad, g)
    assert (c == 0).all()
    # the stream is still usable
    iou2, _ = mesh_eval.mesh_iou(g, g)
    assert float(iou2[0, 0]) == 1.0 and hip.stream_status_bits() == 0


# ------------------------------------------------------------------------------------------------ voxelize_objects
CUBE_V = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]])
TETRA_V = np.array([[0., 0., 0.], [0.8, 0.1, 0.05], [0.2, 0.7, 0.1], [0.3, 0.25, 0.6]])
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def ragged_scene():
    """a cube (stretched, moved), a tetrahedron, an empty mesh, an object of zero extent (NaN after the placement)"""
    from rfdnet_amd.iscnet.scene import SceneMesh
    parts_v = [CUBE_V * [1.0, 0.7, 0.4] + [0.3, -1.2, 2.0], TETRA_V + [0.6, -1.0, 2.1], np.zeros((0, 3)),
               np.full((3, 3), np.nan)]
    parts_f = [CUBE_F, TETRA_F, np.zeros((0, 3), np.int64), np.array([[0, 1, 2]])]
    obj_off = np.concatenate([[0], np.cumsum([len(v) for v in parts_v])])
    face_off = np.concatenate([[0], np.cumsum([len(f) for f in parts_f])])
    v = np.concatenate(parts_v).astype(np.float32)
    f = np.concatenate([f + o for f, o in zip(parts_f, obj_off)]).astype(np.int32)
    face_obj = np.repeat(np.arange(4), np.diff(face_off)).astype(np.int32)
    t = lambda a: torch.from_numpy(a).cuda()
    mesh = SceneMesh(vertices=t(v), faces=t(f), face_obj=t(face_obj), obj_off=t(obj_off.astype(np.int32)),
                     face_off=t(face_off.astype(np.int32)), obj_class=torch.zeros(4, dtype=torch.int32, device="cuda"),
                     normals=None)
    return mesh, [(v[a:b].astype(np.float64), pf) for a, b, pf in zip(obj_off[:-1], obj_off[1:], parts_f)]


@pytest.mark.parametrize("voxel_size,cube_d", [(0.5, 2), (1.0 / 7.5, 7), (1.0 / 65.5, 65)])
def test_voxelize_objects_equals_the_restatement(hip, voxel_size, cube_d):
    from rfdnet_amd.iscnet import mesh_eval
    mesh, parts = ragged_scene()
    grids = mesh_eval.voxelize_objects(mesh, voxel_size)
    want = [M.voxelize(v, f, voxel_size) if len(v) else M.Obj() for v, f in parts]
    assert want[0].S.shape[0] == cube_d and want[0].I.any() and want[2].U is None and want[3].U is None
    dims = [0 if o.U is None else o.S.shape[0] for o in want]
    assert grids.dims.tolist() == dims and grids.dim.cpu().tolist() == dims
    frame, words, off, cnt = (t.cpu().numpy() for t in (grids.frame, grids.words, grids.off, grids.cnt))
    words = words.view(np.uint64)
    for i, o in enumerate(want):
        if o.U is None:
            assert tuple(cnt[i]) == (0, 0)
            continue
        assert (frame[i, :3] == o.lo).all() and frame[i, 3] == o.cell          # equal in float64
        packed = M.pack_words(o.U)
        np.testing.assert_array_equal(words[off[i]:off[i] + len(packed)], packed)
        assert tuple(cnt[i]) == (int(o.U.sum()), int(o.S.sum())) and o.S.any()
    iou, _ = mesh_eval.mesh_iou(grids, grids)
    assert iou.cpu().numpy().tobytes() == M.iou_matrix(want, want)[0].tobytes()
    assert float(iou[0, 0]) == 1.0 and float(iou[1, 1]) == 1.0 and float(iou[2, 2]) == 0.0 and float(iou[3, 3]) == 0.0
    with pytest.raises(ValueError):
        mesh_eval.voxelize_objects(mesh, 1.0 / 300)                           # D > 256


# ------------------------------------------------------------------------------------------------ scene_records
def fixture_inputs(fx):
    c = lambda k: torch.from_numpy(fx[k]).cuda()
    parsed = {'pred_corners_3d_upright_camera': c('corners'), 'sem_cls_probs': c('sem_cls_probs'),
              'obj_prob': c('obj_prob'), 'pred_sem_cls': c('pred_sem_cls')}
    gts = {'gt_corners_3d_upright_camera': c('gt_corners'), 'sem_cls_label': c('gt_sem_cls_label'),
           'box_label_mask': c('gt_box_label_mask')}
    return {'pred_mask': c('pred_mask')}, parsed, gts


@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_mesh_flags_equal_the_reference(hip, fx, objs, tag, pcp):
    from rfdnet_amd.iscnet import evaluation, mesh_eval
    eval_dict, parsed, gts = fixture_inputs(fx)
    B, K = fx['pred_obj'].shape
    G = fx['gt_obj'].shape[1]
    miou = torch.zeros(B, K, G, dtype=torch.float64, device="cuda")          # from the kernels, scene by scene
    for s in range(B):
        pi, gi = fx['pred_obj'][s], fx['gt_obj'][s]
        pg = mesh_eval.pack_grids(as_entries([objs[i] for i in pi[pi >= 0]]), "cuda")
        gg = mesh_eval.pack_grids(as_entries([objs[i] for i in gi[gi >= 0]]), "cuda")
        mesh_eval.scatter_iou(pg, gg, mesh_eval.mesh_iou_counts(pg, gg), miou[s], np.nonzero(pi >= 0)[0], np.nonzero(gi >= 0)[0])
    assert miou.cpu().numpy().tobytes() == fx['mesh_iou'].tobytes()
    cfg = {'per_class_proposal': pcp}
    rec = evaluation.scene_records(eval_dict, parsed, gts, cfg, THR, mesh_iou=miou)
    plain = evaluation.scene_records(eval_dict, parsed, gts, cfg, THR)
    got, base = rec.compact(), plain.compact()
    assert set(base) == {'cls', 'score', 'tp', 'npos', 'thr'} and plain.tp_mesh is None
    assert set(got) == set(base) | {'tp_mesh'}
    for k in ('cls', 'score', 'tp', 'npos'):                                 # the box half is what it is without meshes
        np.testing.assert_array_equal(got[k], base[k])
    assert rec.buf[:plain.buf.numel()].numpy().tobytes() == plain.buf.numpy().tobytes()
    want, want_tp = E.scene_records(fx['corners'], fx['obj_prob'], fx['sem_cls_probs'], fx['pred_sem_cls'], fx['pred_mask'],
                                    fx['gt_corners'], fx['gt_sem_cls_label'], fx['gt_box_label_mask'] == 1, thr=THR,
                                    conf_thresh=float(fx['conf_thresh']), per_class_proposal=pcp, iou3d=fx['mesh_iou'])
    np.testing.assert_array_equal(rec.tp_mesh.numpy(), want_tp)
    np.testing.assert_array_equal(got['tp_mesh'], want['tp'])
    assert (got['tp_mesh'] != got['tp']).any()
    calc = mesh_eval.MeshAPCalculator(THR)
    calc.step(rec)
    metrics = calc.compute_metrics()
    for ti, t in enumerate(THR):
        key = "%s_%g" % (tag, t)
        for flags, sfx in (('tp', ''), ('tp_mesh', '_mesh')):                 # the reference's flags, in its score order
            cur = E.class_curves([dict(got, tp=got[flags])], ti)
            for c in cur:
                np.testing.assert_array_equal(cur[c][3], fx['%s_tp%s_%d' % (key, sfx, c)])
        keys = list(fx[key + '_metric_keys'])
        assert list(metrics[ti].keys()) == keys
        np.testing.assert_allclose(np.array([metrics[ti][k] for k in keys], np.float64), fx[key + '_metric_values'],
                                   rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        evaluation.scene_records(eval_dict, parsed, gts, cfg, THR, mesh_iou=miou[:, :, :2])


# ------------------------------------------------------------------------------------------------------ end to end
def test_evaluate_with_meshes_end_to_end(hip, golden_dir, monkeypatch):
    """ISCNet.evaluate(mesh=True) on the scene of tests/test_gpu_evaluation.py::test_evaluate_end_to_end"""
    from test_gpu_evaluation import labels_from_proposals
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet import evaluation, mesh_eval
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
    labels, n_gt = labels_from_proposals(end_points['parsed_predictions'], end_points['pred_mask'], fnms['mean_size_arr'])
    assert n_gt > 5 and len(meshes) > 0
    data = dict(labels, point_clouds=pc)

    # unit-cube ground-truth meshes: the box half is bit for bit what it is without meshes
    cube = (CUBE_V, CUBE_F)
    _, _, _, plain = net.evaluate(data, fit=False)
    ep, ids2, meshes2, rec = net.evaluate(dict(data, gt_meshes=[cube] * n_gt), fit=False, mesh=True)
    got, base = rec.compact(), plain.compact()
    for k in ('cls', 'score', 'tp', 'npos'):
        assert got[k].tobytes() == base[k].tobytes()
    assert rec.buf[:plain.buf.numel()].numpy().tobytes() == plain.buf.numpy().tobytes()
    miou = ep['mesh_iou']
    assert tuple(miou.shape) == (1, 256, 64) and miou.dtype == torch.float64
    m = miou.cpu().numpy()
    assert np.isfinite(m).all() and m.min() >= 0 and m.max() <= 1 and (m > 0).any()
    assert (m[0, :, n_gt:] == 0).all()                                       # masked ground-truth rows
    with_mesh = np.zeros(256, bool)
    with_mesh[ids[0, :, 0].cpu().numpy()] = True
    assert (m[0, ~with_mesh] == 0).all()                                     # proposals without a generated mesh
    calc = mesh_eval.MeshAPCalculator(THR)
    calc.step(rec)
    out = calc.compute_metrics()
    assert np.isfinite(out[0]['mAP_mesh']) and np.isfinite(out[1]['mAP_mesh'])
    # a class with predictions and no ground truth has recall 0 / 0 = NaN, as in the reference: the mesh half has its
    # NaN exactly where the box half has them (the ground-truth counts are the same), and the same keys in the same order
    box_keys = [k for k in out[0] if not k.endswith('_mesh')]
    assert [k + '_mesh' for k in box_keys] == [k for k in out[0] if k.endswith('_mesh')]
    for o in out:
        assert all(np.isnan(o[k]) == np.isnan(o[k + '_mesh']) for k in box_keys)
        assert all(0 <= o[k + '_mesh'] <= 1 for k in box_keys if not np.isnan(o[k + '_mesh']))
    with pytest.raises(ValueError):
        net.evaluate(dict(data, gt_meshes=[cube] * (n_gt - 1)), fit=False, mesh=True)

    # the generated meshes themselves as ground truth, each in the box of its own proposal: those pairs are exactly 1.
    # The ground-truth corners decoded from labels cannot reproduce a predicted box to the bit, so the parsed ground
    # truths are given the scored corners directly.
    n_self = min(len(meshes), n_gt)
    rows = ids[0, :n_self, 0]
    parse = evaluation.parse_groundtruths

    def parse_with_predicted_boxes(gt_data, dataset_config):
        out = parse(gt_data, dataset_config)
        c = out['gt_corners_3d_upright_camera'].clone()
        c[0, :n_self] = end_points['parsed_predictions']['pred_corners_3d_upright_camera'][0, rows].double()
        return dict(out, gt_corners_3d_upright_camera=c)
    monkeypatch.setattr(evaluation, "parse_groundtruths", parse_with_predicted_boxes)
    gt_meshes = [meshes[j] for j in range(n_self)] + [None] * (n_gt - n_self)
    ep, _, _, rec = net.evaluate(dict(data, gt_meshes=gt_meshes), fit=False, mesh=True)
    m = ep['mesh_iou'][0].cpu().numpy()
    own = m[rows.cpu().numpy(), np.arange(n_self)]
    has_faces = np.array([int(meshes[j].faces.shape[0]) > 0 for j in range(n_self)])
    print("self pairs: %d of %d meshes have faces; IoU %s" % (has_faces.sum(), n_self, own))
    assert has_faces.any() and (own[has_faces] == 1.0).all() and (own[~has_faces] == 0.0).all()
    assert (m[:, n_self:n_gt] == 0).all()                                    # ground truths without a mesh
    assert hip.stream_status_bits() == 0
