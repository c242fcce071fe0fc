"""GPU: the completion loss of the test mode (csrc/encoder_latent.hip, include/rfd_latent.h) -- the latent encoder against
float64 (the fixture F_LAT's float64 run of the reference modules; tests/latent_f64.py on ragged shapes), its bit-identity
across batch, point order and runs, the BCE row sums, the voxel IoU counts, ONet.compute_loss against the reference's
recorded call and ISCNet.evaluate(completion=True).

Bounds.  Encoder outputs and KL: 8 x `ref32_dev`, the reference fp32 run's own largest deviation from float64 on the same
quantity (both sides are fp32 evaluations in another summation order of 128-term dot products through three layers; the
maximum over 96 outputs is a noisy statistic, hence 8 and not 2).  BCE per proposal: T * 1e-4, the project's logit contract
times BCE's Lipschitz constant 1 in the logit."""
import os

import numpy as np
import pytest
import torch

from rfdnet_amd import synthetic
from rfdnet_amd.iscnet.config import Config

from latent_f64 import bce_rowsum_f64, compute_iou, encoder_f64, kl_f64
from seeded import onet_arrays, seeded_onet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "F_LAT.npz")), np.load(os.path.join(golden_dir, "F_GEN.npz"))


@pytest.fixture(scope="module")
def encoder(hip, fx):
    """the fixture's encoder (seed-202 ONet weights in the reference's key order) on the device + its weights as numpy"""
    from rfdnet_amd.iscnet.encoder_latent import Encoder_Latent
    sd = {k[len("encoder_latent."):]: v for k, v in onet_arrays(fx[1]).items() if k.startswith("encoder_latent.")}
    enc = Encoder_Latent(z_dim=32, c_dim=512)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return enc.cuda().eval(), sd


def make_onet(fgen, threshold=0.5):
    return seeded_onet(fgen, generation={'upsampling_steps': 0}, data={'threshold': threshold, 'latent_encoder': True})


def count_calls(hip, monkeypatch):
    names = []
    call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


def test_encoder_on_the_fixture(hip, fx, encoder, monkeypatch):
    """K = 3, T = 2048: |mean - f64| and |logstd - f64| <= 8 x ref32_dev; at most 6 launches.  Measured on the MI355X: mean
    1.27e-8, logstd 1.49e-8 (the reference's fp32 run: 4.94e-8, 3.51e-8)."""
    flat, fgen = fx
    enc, _ = encoder
    p, o, c = (torch.from_numpy(a).cuda() for a in (flat["points"], flat["occ"], fgen["codes"]))
    names = count_calls(hip, monkeypatch)
    mean, logstd = enc(p, o, c)
    assert names == ["rfd_latent_prep"] + ["rfd_latent_stage"] * 3 + ["rfd_latent_head"] and len(names) <= 6
    dm = np.abs(mean.cpu().numpy().astype(np.float64) - flat["mean64"]).max()
    dl = np.abs(logstd.cpu().numpy().astype(np.float64) - flat["logstd64"]).max()
    print("encoder vs f64: mean %.3e (reference fp32 %.3e), logstd %.3e (reference fp32 %.3e)"
          % (dm, flat["ref32_dev"][0], dl, flat["ref32_dev"][1]))
    assert dm <= 8 * flat["ref32_dev"][0] and dl <= 8 * flat["ref32_dev"][1]
    assert mean.shape == logstd.shape == (3, 32) and mean.dtype == torch.float32


@pytest.mark.parametrize("T", [1, 31, 33, 257])
def test_encoder_ragged_shapes(hip, fx, encoder, T):
    """K = 5, T no multiple of the 32-point wave or the 128-point workgroup; T = 1: a padded row that reached the pool
    could not hide behind a larger live one"""
    flat, _ = fx
    enc, sd = encoder
    rng = np.random.default_rng(100 + T)
    p = rng.uniform(-0.55, 0.55, (5, T, 3)).astype(np.float32)
    o = (rng.random((5, T)) < 0.4).astype(np.float32)
    c = rng.normal(0, 1, (5, 512)).astype(np.float32)
    mean, logstd = enc(torch.from_numpy(p).cuda(), torch.from_numpy(o).cuda(), torch.from_numpy(c).cuda())
    rm, rl = encoder_f64(sd, p, o, c)
    dm, dl = np.abs(mean.cpu().numpy() - rm).max(), np.abs(logstd.cpu().numpy() - rl).max()
    print("T = %d: mean %.3e logstd %.3e" % (T, dm, dl))
    assert dm <= 8 * flat["ref32_dev"][0] and dl <= 8 * flat["ref32_dev"][1]


def test_encoder_bit_identity(hip, encoder):
    """a proposal alone == itself in a batch of 5; permuting its points changes nothing; two runs are equal"""
    enc, _ = encoder
    rng = np.random.default_rng(7)
    T = 257
    p = torch.from_numpy(rng.uniform(-0.55, 0.55, (5, T, 3)).astype(np.float32)).cuda()
    o = torch.from_numpy((rng.random((5, T)) < 0.4).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.normal(0, 1, (5, 512)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.normal(0, 1, (5, 32)).astype(np.float32)).cuda()
    batch = enc.posterior(p, o, c, eps)
    again = enc.posterior(p, o, c, eps)
    alone = enc.posterior(p[2:3], o[2:3], c[2:3], eps[2:3])
    perm = torch.from_numpy(rng.permutation(T)).cuda()
    shuffled = enc.posterior(p[2:3][:, perm], o[2:3][:, perm], c[2:3], eps[2:3])
    for a, b, s, n in zip(batch, again, alone, shuffled):
        assert torch.equal(a, b) and torch.equal(a[2:3], s) and torch.equal(s, n)
    assert torch.isfinite(batch[3]).all() and float(batch[3].min()) >= 0.0          # a KL divergence


@pytest.mark.parametrize("T", [1, 2047, 2048, 2049])
def test_bce_rowsum(hip, T):
    from rfdnet_amd.iscnet.occupancy_net import bce_logits_rowsum
    rng = np.random.default_rng(T)
    special = np.array([0, 1e-3, -1e-3, 30, -30, 90, -90], np.float32)
    x = rng.normal(0, 3, (3, T)).astype(np.float32)
    y = np.empty((3, T), np.float32)
    for k in range(3):
        n = min(T, special.size)
        pos = rng.permutation(T)[:n]
        x[k, pos] = np.roll(special, k)[:n]
        y[k] = (0.0, 1.0, 0.3)[k]
    if T > 1:
        y[0, ::2] = 1.0                                                     # a row of mixed targets
    ref = bce_rowsum_f64(x, y)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    out = bce_logits_rowsum(xd, yd)
    rel = np.abs(out.cpu().numpy().astype(np.float64) - ref) / ref
    print("T = %d: relative error %s" % (T, rel))
    assert torch.isfinite(out).all() and rel.max() <= 1e-6
    assert torch.equal(out, bce_logits_rowsum(xd, yd))
    # a view with a row stride (the decoder's padded logits) is read in place
    wide = torch.full((3, T + 5), 1e4, device="cuda")
    wide[:, :T] = xd
    assert torch.equal(out, bce_logits_rowsum(wide[:, :T], yd))


@pytest.mark.parametrize("V", [4096, 4097])
def test_voxel_iou(hip, V):
    from rfdnet_amd.iscnet import evaluation
    rng = np.random.default_rng(V)
    logits = rng.normal(0, 1, (4, V)).astype(np.float32)
    gt = (rng.random((4, V)) < 0.3).astype(np.float32)
    thr = float(np.log(0.2) - np.log(0.8))
    logits[1] = thr - 1.0                                                    # an all-empty pair: 0 / 0
    gt[1] = 0
    logits[2, :7] = np.float32(thr)                                          # exactly at the threshold: set
    gt[3] = rng.random(V).astype(np.float32)                                 # any float: >= 0.5 is the bit
    iou, inter, union = evaluation.voxel_iou(torch.from_numpy(logits).cuda(), thr, torch.from_numpy(gt).cuda(),
                                             return_counts=True)
    pred = logits >= np.float32(thr)
    g = gt >= 0.5
    np.testing.assert_array_equal(inter.cpu().numpy(), (pred & g).sum(1))
    np.testing.assert_array_equal(union.cpu().numpy(), (pred | g).sum(1))
    assert inter.dtype == union.dtype == torch.int32
    want = compute_iou(pred, gt)
    got = iou.cpu().numpy()
    assert np.isnan(got[1]) and np.isnan(want[1])
    np.testing.assert_array_equal(got.view(np.uint32)[[0, 2, 3]], want.view(np.uint32)[[0, 2, 3]])


@pytest.mark.parametrize("thr", [0.5, 0.2])
def test_compute_loss_on_the_fixture(hip, fx, thr):
    """ONet.compute_loss with the fixture's eps against the float64 run of the reference's modules.  Measured on the MI355X
    (the reference's own fp32 run in brackets): KL 1.0e-8 (1.46e-7), BCE per proposal 5.5e-5 / 2.5e-4 / 9.8e-5 (5.5e-5 /
    3.6e-4 / 9.8e-5) against the bound T * 1e-4 = 0.205, loss 1857.1750 (1857.1753); 4 lattice points excluded at threshold
    0.5 and none at 0.2, none of them different from the reference's voxels."""
    flat, fgen = fx
    onet = make_onet(fgen, thr)
    p, o, c, eps = (torch.from_numpy(a).cuda() for a in (flat["points"], flat["occ"], fgen["codes"], flat["eps"]))
    loss, voxels, terms = onet.compute_loss(c, p, o, None, export_shape=True, eps=eps, return_terms=True)
    T = p.shape[1]
    kl, bce = terms['kl'].cpu().numpy().astype(np.float64), terms['bce'].cpu().numpy().astype(np.float64)
    dk, db = np.abs(kl - flat["kl64"]).max(), np.abs(bce - flat["bce64"])
    print("threshold %g: kl vs f64 %.3e (reference fp32 %.3e), bce vs f64 %s (reference fp32 %s), loss %.4f (reference "
          "%.4f), z vs reference fp32 %.3e" % (thr, dk, flat["ref32_dev"][2], db, np.abs(flat["bce32"] - flat["bce64"]),
                                               float(loss), float(flat["loss32"]),
                                               np.abs(terms['z'].cpu().numpy() - flat["z32"]).max()))
    assert dk <= 8 * flat["ref32_dev"][2]
    assert db.max() <= T * 1e-4
    assert abs(float(loss) - (kl.mean() + bce.mean())) <= 1e-3 and loss.shape == ()
    # the head's KL is the f64 formula on ITS fp32 mean / logstd, rounded once: numpy's, to the last fp32 place (the device's
    # exp and its summation tree differ from numpy's in the last f64 place, which moves the rounding almost never)
    head = kl_f64(terms['mean'].cpu().numpy(), terms['logstd'].cpu().numpy()).astype(np.float32)
    assert np.abs(terms['kl'].cpu().numpy() - head).max() <= np.spacing(head).max()
    lt = np.log(thr) - np.log(1. - thr)
    near = np.abs(flat["voxel_logits64"] - lt) <= 1e-4
    assert near.mean() <= 0.005
    ref = flat["voxels_out_" + ("%g" % thr).replace(".", "")]
    assert voxels.shape == (3, 16, 16, 16) and voxels.dtype == torch.bool
    got = voxels.cpu().numpy().reshape(3, -1)
    print("threshold %g: %d lattice points excluded, %d of them differ" % (thr, near.sum(), (got != ref.reshape(3, -1))[near].sum()))
    np.testing.assert_array_equal(got[~near], ref.reshape(3, -1)[~near])
    # without return_terms / export_shape: the reference's return shape
    loss2, none = onet.compute_loss(c, p, o, None, eps=eps)
    assert none is None and torch.equal(loss2, loss)
    # eps=None draws on the device: another loss, the same KL (it does not depend on the draw)
    _, _, drawn = onet.compute_loss(c, p, o, None, return_terms=True)
    assert torch.equal(drawn['kl'], terms['kl']) and not torch.equal(drawn['z'], terms['z'])
    assert hip.stream_status_bits() == 0


def test_compute_loss_without_a_latent_code_and_with_class_codes(hip):
    """z_dim == 0 works without the encoder (loss = BCE alone); use_cls_for_completion concatenates the class codes"""
    from rfdnet_amd.iscnet.occupancy_net import ONet, bce_logits_rowsum
    rng = np.random.default_rng(3)
    p = torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 130, 3)).astype(np.float32)).cuda()
    o = torch.from_numpy((rng.random((2, 130)) < 0.5).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.normal(0, 1, (2, 512)).astype(np.float32)).cuda()
    cls = torch.eye(8)[[1, 5]].cuda()
    onet = ONet(Config({'data': {'z_dim': 0}, 'generation': {'resolution_0': 16}}))
    synthetic.load_seeded(onet, 5)
    onet = onet.cuda().eval()
    loss, vox = onet.compute_loss(c, p, o, cls)
    assert vox is None and torch.equal(loss, bce_logits_rowsum(onet(p, c, cls).logits.contiguous(), o).mean())
    onet = ONet(Config({'data': {'use_cls_for_completion': True, 'latent_encoder': True}, 'generation': {'resolution_0': 16}}))
    assert onet.encoder_latent.fc_c.weight.shape == (128, 520)
    synthetic.load_seeded(onet, 5)
    onet = onet.cuda().eval()
    eps = torch.zeros(2, 32, device="cuda")
    _, _, terms = onet.compute_loss(c, p, o, cls, eps=eps, return_terms=True)
    sd = {k[len("encoder_latent."):]: v.cpu().numpy() for k, v in onet.state_dict().items() if k.startswith("encoder_latent.")}
    rm, _ = encoder_f64(sd, p.cpu().numpy(), o.cpu().numpy(), torch.cat([c, cls], 1).cpu().numpy())
    # a wiring check (are the class codes in the encoder's input?): fp32 is ~1e-7 off, a missing code ~1e-1
    assert np.abs(terms['mean'].cpu().numpy() - rm).max() < 1e-5 and torch.equal(terms['z'], terms['mean'])


def completion_scene():
    """a 4096-point synthetic scene with its twelve cuboids as ground truth in every second label row"""
    pc, boxes, cls = synthetic.synthetic_scene(seed=3, n_raw=5000, n_points=4096, return_boxes=True)
    G, T = 32, 200
    pts, occ, vox = synthetic.object_occupancy(boxes, n_points=T, seed=9)
    data = {'center_label': np.zeros((1, G, 3), np.float32), 'heading_class_label': np.zeros((1, G), np.int64),
            'heading_residual_label': np.zeros((1, G), np.float32), 'size_class_label': np.zeros((1, G), np.int64),
            'size_residual_label': np.zeros((1, G, 3), np.float32), 'sem_cls_label': np.zeros((1, G), np.int64),
            'box_label_mask': np.zeros((1, G), np.float32), 'object_points': np.zeros((1, G, T, 3), np.float32),
            'object_points_occ': np.zeros((1, G, T), np.float32), 'object_voxels': np.zeros((1, G, 16, 16, 16), np.float32)}
    rows = 2 * np.arange(12) + 1                                             # masked-out rows in between and in front
    data['center_label'][0, rows] = boxes[:, :3]
    data['size_residual_label'][0, rows] = boxes[:, 3:6] - 0.8
    data['sem_cls_label'][0, rows] = cls
    data['box_label_mask'][0, rows] = 1
    data['object_points'][0, rows], data['object_points_occ'][0, rows], data['object_voxels'][0, rows] = pts, occ, vox
    data = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
    data['point_clouds'] = torch.from_numpy(pc[None]).cuda()
    return data


def test_evaluate_with_completion(hip, monkeypatch):
    from rfdnet_amd.iscnet.network import ISCNet
    cfg = Config({'data': {'latent_encoder': True}, 'generation': {'resolution_0': 8, 'upsampling_steps': 0}},
                 mean_size_arr=np.full((8, 3), 0.8))
    cfg.eval_overrides = dict(getattr(cfg, 'eval_overrides', None) or {}, remove_empty_box=False)
    net = ISCNet(cfg)
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    detect = net.detect

    def every_proposal_is_an_object(point_clouds):
        ep, pf = detect(point_clouds)
        ep['objectness_scores'] = torch.tensor([0.0, 4.0], device="cuda").expand_as(ep['objectness_scores']).contiguous()
        return ep, pf
    net.detect = every_proposal_is_an_object
    data = completion_scene()

    # ---- completion=False: the parent's evaluate, call for call (after one pass that packs the weights, once per network)
    net.generate(data, selection='nms')
    names = count_calls(hip, monkeypatch)
    ep0, ids0, meshes0, rec0 = net.evaluate(data, fit=False)
    plain = list(names)
    del names[:]
    from rfdnet_amd.iscnet import evaluation
    ep1, ids1, meshes1 = net.generate(data, selection='nms')                 # the parent's evaluate, restated
    rec1 = evaluation.scene_records({'pred_mask': ep1['pred_mask']}, ep1['parsed_predictions'],
                                    evaluation.parse_groundtruths(data, cfg.dataset_config),
                                    getattr(cfg, 'eval_overrides', None), (0.25, 0.5))
    assert plain == names and not any(n.startswith(("rfd_latent", "rfd_bce", "rfd_voxel")) for n in plain)
    assert torch.equal(ids0, ids1) and len(meshes0) == len(meshes1) == ids0.shape[1] >= 1
    for a, b in zip(meshes0, meshes1):
        assert torch.equal(torch.as_tensor(a.vertices), torch.as_tensor(b.vertices))
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(rec0.compact()[k], rec1.compact()[k])
    assert not {'completion_loss', 'proposal_to_gt', 'iou_stats'} & set(ep0)

    # ---- completion=True
    seen = {}
    compute_loss = net.completion.compute_loss

    def recording(*a, **k):
        seen['args'], seen['kwargs'] = a, k
        seen['out'] = compute_loss(*a, **k)
        return seen['out']
    monkeypatch.setattr(net.completion, "compute_loss", recording)
    Kp = ids0.shape[1]
    eps = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (Kp, 32)).astype(np.float32)).cuda()
    del names[:]
    ep, ids, meshes, rec = net.evaluate(data, fit=False, completion=True, completion_eps=eps)
    assert names[:len(plain) - 2] == plain[:-2] and names[-2:] == plain[-2:]                  # the box records come last
    assert names.count("rfd_latent_stage") == 3 and names.count("rfd_bce_logits_rowsum") == names.count("rfd_voxel_iou") == 1
    assert torch.equal(ids, ids0) and len(meshes) == Kp
    np.testing.assert_array_equal(rec.compact()['tp'], rec0.compact()['tp'])
    pairs = ep['proposal_to_gt'].cpu()
    assert pairs.shape == (1, Kp, 3) and pairs.dtype == torch.int64
    # proposal_to_gt against torch on the CPU: the nearest centroid among the masked rows, lowest index on a tie
    centers = ep['center'][0].cpu().double()
    rows = torch.nonzero(data['box_label_mask'][0].cpu()).squeeze(1)
    d = ((centers[:, None, :] - data['center_label'][0].cpu().double()[rows][None]) ** 2).sum(-1)
    assign = rows[torch.argmin(d, dim=1)]
    want = torch.stack([ids[0, :, 0].cpu(), assign[ids[0, :, 0].cpu()],
                        data['sem_cls_label'][0].cpu()[assign[ids[0, :, 0].cpu()]]], dim=-1)
    assert torch.equal(pairs[0], want)
    assert len(set(pairs[0, :, 1].tolist())) >= 1 and set(pairs[0, :, 1].tolist()) <= set(rows.tolist())
    # prepare_data: the gathered samples are those rows
    codes, points, occ, cls = seen['args']
    assert torch.equal(points, data['object_points'][0][pairs[0, :, 1].cuda()])
    assert torch.equal(occ, data['object_points_occ'][0][pairs[0, :, 1].cuda()])
    assert seen['kwargs']['export_shape'] is True and codes.shape == (Kp, 512)
    # the loss is compute_loss called by hand on the same inputs and eps, bit for bit
    loss, voxels, terms = compute_loss(codes, points, occ, cls, export_shape=True, eps=eps, return_terms=True)
    assert torch.equal(ep['completion_loss'], loss) and torch.isfinite(loss) and loss.dim() == 0
    stats = ep['iou_stats']
    np.testing.assert_array_equal(stats['cls'], pairs[0, :, 2].numpy())
    want_iou = compute_iou(voxels.cpu().numpy(), data['object_voxels'][0][pairs[0, :, 1].cuda()].cpu().numpy())
    np.testing.assert_array_equal(stats['iou'].view(np.uint32), want_iou.view(np.uint32))
    print("K' = %d proposals, completion loss %.3f, mean voxel IoU %.4f" % (Kp, float(loss), np.nanmean(stats['iou'])))
    # without object_voxels: no shape example, no IoU
    ep2, _, _, _ = net.evaluate({k: v for k, v in data.items() if k != 'object_voxels'}, fit=False, completion=True,
                                completion_eps=eps)
    assert ep2['iou_stats'] is None and seen['kwargs']['export_shape'] is False
    assert torch.equal(ep2['completion_loss'], loss)
    assert hip.stream_status_bits() == 0
