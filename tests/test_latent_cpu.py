"""CPU: the host side of the completion loss -- the latent encoder's state_dict keys against the reference ONet's full
list (F_GEN), the float64 restatement (tests/latent_f64.py) against the fixture's float64 run of the reference
modules (F_LAT, tests/golden/make_latent_fixture.py), and the errors of the entry points."""
import os

import numpy as np
import pytest

from rfdnet_amd import synthetic
from rfdnet_amd.iscnet.config import Config

from latent_f64 import bce_rowsum_f64, compute_iou, encoder_f64, kl_f64
from seeded import decoder_arrays, onet_arrays
from test_modules_cpu import my_keys, ref_keys


@pytest.fixture(scope="module")
def flat(golden_dir):
    return np.load(os.path.join(golden_dir, "F_LAT.npz"))


@pytest.fixture(scope="module")
def fgen(golden_dir):
    return np.load(os.path.join(golden_dir, "F_GEN.npz"))


def test_onet_with_latent_encoder_has_the_reference_keys_in_order(fgen):
    from rfdnet_amd.iscnet.occupancy_net import ONet
    onet = ONet(Config())
    assert onet.encoder_latent is None and not any(k.startswith("encoder_latent.") for k, _ in my_keys(onet))
    assert onet.enable_latent_encoder() is onet
    assert my_keys(onet) == ref_keys(fgen, "onet")
    assert [n for n, _ in onet.named_children()][:2] == ["encoder_latent", "decoder"]
    onet.enable_latent_encoder()                                         # idempotent
    assert my_keys(onet) == ref_keys(fgen, "onet")
    # the config switch calls it; z_dim == 0 has no encoder, as in the reference
    assert my_keys(ONet(Config({'data': {'latent_encoder': True}}))) == ref_keys(fgen, "onet")
    assert ONet(Config({'data': {'z_dim': 0}})).enable_latent_encoder().encoder_latent is None


def test_a_reference_checkpoint_keeps_its_latent_encoder_tensors(fgen):
    """load_weight drops keys the network does not own: with the encoder enabled completion.encoder_latent.* stay"""
    import torch
    from rfdnet_amd.iscnet.network import ISCNet
    sd = {"module.completion." + k: torch.from_numpy(v) for k, v in onet_arrays(fgen).items()}
    plain = ISCNet(Config())
    plain.load_weight(sd)
    assert plain.completion.encoder_latent is None
    net = ISCNet(Config({'data': {'latent_encoder': True}}))
    net.load_weight(sd)
    got = net.completion.encoder_latent.fc_3.weight.detach().numpy()
    np.testing.assert_array_equal(got, sd["module.completion.encoder_latent.fc_3.weight"].numpy())
    view = net.worker_view()                                             # shared, not copied
    assert view.completion.encoder_latent is net.completion.encoder_latent


def test_restatement_agrees_with_the_float64_run_of_the_reference_modules(flat, fgen):
    sd = {k[len("encoder_latent."):]: v for k, v in onet_arrays(fgen).items() if k.startswith("encoder_latent.")}
    mean, logstd = encoder_f64(sd, flat["points"], flat["occ"], fgen["codes"])
    assert np.abs(mean - flat["mean64"]).max() <= 1e-12
    assert np.abs(logstd - flat["logstd64"]).max() <= 1e-12
    assert np.abs(kl_f64(mean, logstd) - flat["kl64"]).max() <= 1e-12
    z = mean + flat["eps"].astype(np.float64) * np.exp(logstd)
    assert np.abs(z - flat["z64"]).max() <= 1e-12
    # the decoder's restatement (tests/dec_f64.py) closes the loop: BCE at that z, and the lattice logits
    from dec_f64 import decoder_f64
    dsd = decoder_arrays(fgen)
    bce = bce_rowsum_f64(decoder_f64(dsd, flat["points"], z, fgen["codes"]), flat["occ"])
    assert np.abs(bce - flat["bce64"]).max() <= 1e-12 * flat["bce64"].max()
    # the fixture is self-consistent: fp32 records within their own stated deviation, the loss is the two means
    assert np.abs(flat["mean32"] - flat["mean64"]).max() == flat["ref32_dev"][0]
    assert np.abs(flat["logstd32"] - flat["logstd64"]).max() == flat["ref32_dev"][1]
    assert np.abs(flat["kl32"] - flat["kl64"]).max() == flat["ref32_dev"][2]
    assert abs(float(flat["loss32"]) - (flat["kl64"].mean() + flat["bce64"].mean())) < 1e-3
    for tag, thr in (("05", 0.5), ("02", 0.2)):
        lt = np.log(thr) - np.log(1 - thr)
        near = np.abs(flat["voxel_logits64"] - lt) <= 1e-4
        assert near.mean() <= 0.005
        np.testing.assert_array_equal(flat["voxels_out_" + tag].reshape(3, -1)[~near], (flat["voxel_logits64"] >= lt)[~near])


def test_compute_iou_restatement_on_edge_cases():
    a = np.zeros((3, 2, 2, 2), np.float32)
    b = np.zeros((3, 2, 2, 2), np.float32)
    a[1, 0] = 1
    b[1, :, 0] = 0.5
    a[2], b[2] = 1, 0.7
    iou = compute_iou(a, b)
    assert np.isnan(iou[0]) and iou[1] == np.float32(2) / np.float32(6) and iou[2] == 1 and iou.dtype == np.float32


def test_synthetic_object_occupancy():
    _, boxes, _ = synthetic.synthetic_scene(seed=3, n_raw=3000, n_points=1024, return_boxes=True)
    p, occ, vox = synthetic.object_occupancy(boxes, n_points=300, seed=4)
    p2, occ2, vox2 = synthetic.object_occupancy(boxes, n_points=300, seed=4)
    assert np.array_equal(p, p2) and np.array_equal(occ, occ2) and np.array_equal(vox, vox2)
    assert p.shape == (12, 300, 3) and occ.shape == (12, 300) and vox.shape == (12, 16, 16, 16)
    assert p.dtype == occ.dtype == vox.dtype == np.float32 and np.abs(p).max() <= 0.5
    assert set(np.unique(occ)) == {0.0, 1.0} and set(np.unique(vox)) == {0.0, 1.0}
    # the ellipsoid fills pi/6 * prod(axes ratios) * 0.9^3 of the cube: both samplings see about that share
    axes = 0.45 * boxes[:, 3:6] / boxes[:, 3:6].max(1, keepdims=True)
    share = 4 / 3 * np.pi * axes.prod(1)
    assert np.abs(vox.mean(axis=(1, 2, 3)) - share).max() < 0.02
    assert np.abs(occ.mean(1) - share).max() < 0.1
    # the longest axis reaches 0.45: the voxel centre nearest to it along that axis is inside, the cube's corner is not
    assert vox[:, 0, 0, 0].max() == 0


def test_compute_loss_without_the_encoder_names_the_switch():
    import torch
    from rfdnet_amd.iscnet.occupancy_net import ONet
    onet = ONet(Config())

    with pytest.raises(RuntimeError, match="enable_latent_encoder"):
        onet.compute_loss(torch.zeros(2, 512), torch.zeros(2, 4, 3), torch.zeros(2, 4), None)
    onet.enable_latent_encoder()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        onet.compute_loss(torch.zeros(2, 512), torch.zeros(2, 4, 3), torch.zeros(2, 4), None)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        onet.encoder_latent(torch.zeros(2, 4, 3), torch.zeros(2, 4), torch.zeros(2, 512))


def test_leaky_encoder_is_not_built():
    from rfdnet_amd.iscnet.encoder_latent import Encoder_Latent
    with pytest.raises(NotImplementedError, match="leaky"):
        Encoder_Latent(leaky=True)
    enc = Encoder_Latent(z_dim=32, c_dim=0)
    assert "fc_c.weight" not in enc.state_dict() and enc.fc_2.weight.shape == (128, 256)


def test_latent_abi_entries_take_a_trailing_stream():
    from rfdnet_amd import _lib
    for name, n in (("rfd_latent_prep", 8), ("rfd_latent_stage", 12), ("rfd_latent_head", 11),
                    ("rfd_bce_logits_rowsum", 8), ("rfd_voxel_iou", 9)):
        assert len(_lib.SIGNATURES[name]) == n and _lib.SIGNATURES[name][-1] is _lib._f
