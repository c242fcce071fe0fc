"""Generate tests/golden/F_LAT.npz (DEV CONTAINER ONLY): the reference's ONet.compute_loss (occupancy_net.py:59-109, torch
CPU fp32) -- latent encoder, rsample, KL, BCE and the 16^3 voxel example -- on F_GEN's three codes.

Same recipe as make_refine_fixture.py: the reference ONet with seed-202 weights (synthetic.load_seeded seeds
encoder_latent.* too) and F_GEN's codes.  Inputs: T = 2048 points uniform in [-0.55, 0.55]^3 (numpy PCG64, POINT_SEED) with the
occupancy of a sphere of radius 0.35.  The standard-normal draw of rsample() and the z that reaches decode() are captured by
wrapping torch.distributions' _standard_normal and ONet.decode.

Beside the reference's fp32 results the file holds a float64 run of the same modules (mean, logstd, per-proposal KL and BCE,
the 4096 lattice logits at the prior mean), `ref32_dev`: the fp32 run's own largest deviation from that float64 run on mean,
logstd and KL -- the unit of the device tests' bounds -- and a synthetic ground-truth voxel grid for the IoU.

Usage:  python tests/golden/make_latent_fixture.py
"""
import copy
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
from make_fixtures import mount_reference, ns  # noqa: E402

POINT_SEED, EPS_SEED, T, RADIUS = 31, 5, 2048, 0.35
THRESHOLDS = (0.5, 0.2)
BAND, BAND_CAP = 1e-4, 0.005


def main():
    import torch
    import torch.distributions as dist
    import torch.nn.functional as F
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.config import Config
    from latent_f64 import bce_rowsum_f64, compute_iou, encoder_f64, kl_f64
    mount_reference()
    ns('external.libmise').MISE = None
    ns('models.registers')
    reg = importlib.import_module('net_utils.registry')
    sys.modules['models.registers'].MODULES = reg.Registry('module')
    sys.modules['models.registers'].METHODS = reg.Registry('method')
    sys.modules['models.registers'].LOSSES = reg.Registry('loss')
    onet_mod = importlib.import_module('models.iscnet.modules.occupancy_net')
    gen = np.load(os.path.join(HERE, "F_GEN.npz"))
    codes = gen["codes"]
    K = codes.shape[0]
    onet = onet_mod.ONet(Config({'generation': {'resolution_0': 16, 'upsampling_steps': 1}}))
    synthetic.load_seeded(onet, 202)
    onet.eval()
    onet64 = copy.deepcopy(onet).double()

    rng = np.random.default_rng(POINT_SEED)
    points = rng.uniform(-0.55, 0.55, (K, T, 3)).astype(np.float32)
    occ = ((points.astype(np.float64) ** 2).sum(-1) <= RADIUS ** 2).astype(np.float32)
    p, o, c = torch.from_numpy(points), torch.from_numpy(occ), torch.from_numpy(codes)

    # ---- the reference call, with the draw and the decoded z captured
    seen = {}
    normal_mod = importlib.import_module('torch.distributions.normal')
    draw = normal_mod._standard_normal

    def recording_draw(*a, **k):
        seen['eps'] = draw(*a, **k)
        return seen['eps']
    decode = onet.decode

    def recording_decode(pts, z, feat, **k):
        seen.setdefault('z', z.detach().clone())            # the first decode is the loss's (the second: the prior mean)
        return decode(pts, z, feat, **k)
    out = {"points": points, "occ": occ, "point_seed": POINT_SEED, "eps_seed": EPS_SEED, "radius": RADIUS,
           "thresholds": np.array(THRESHOLDS)}
    with torch.no_grad():
        for thr in THRESHOLDS:
            seen.clear()
            onet.threshold = thr
            normal_mod._standard_normal, onet.decode = recording_draw, recording_decode
            torch.manual_seed(EPS_SEED)
            try:
                loss, voxels = onet.compute_loss(c, p, o, None, export_shape=True)
            finally:
                normal_mod._standard_normal = draw
                del onet.decode
            tag = ("%g" % thr).replace(".", "")
            out["voxels_out_" + tag] = voxels.numpy()
            if "eps" in out:
                assert np.array_equal(out["eps"], seen['eps'].numpy()) and float(loss) == float(out["loss32"])
            out["eps"], out["z32"], out["loss32"] = seen['eps'].numpy(), seen['z'].numpy(), np.float32(loss)
        eps = torch.from_numpy(out["eps"])
        mean32, logstd32 = onet.encoder_latent(p, o, c)
        q = dist.Normal(mean32, torch.exp(logstd32))
        kl32 = dist.kl_divergence(q, onet.get_prior_z(onet.z_dim, 'cpu')).sum(-1)
        assert torch.equal(mean32 + eps * torch.exp(logstd32), seen['z'])
        bce32 = F.binary_cross_entropy_with_logits(onet.decode(p, seen['z'], c).logits, o, reduction='none').sum(-1)
        assert abs(float(kl32.mean() + bce32.mean()) - float(out["loss32"])) < 1e-3
        # ---- the same modules in float64
        p64, o64, c64 = p.double(), o.double(), c.double()
        mean64, logstd64 = onet64.encoder_latent(p64, o64, c64)
        q64 = dist.Normal(mean64, torch.exp(logstd64))
        kl64 = dist.kl_divergence(q64, dist.Normal(torch.zeros(onet.z_dim).double(), torch.ones(onet.z_dim).double())).sum(-1)
        z64 = mean64 + eps.double() * torch.exp(logstd64)
        logits64 = onet64.decode(p64, z64, c64).logits
        bce64 = F.binary_cross_entropy_with_logits(logits64, o64, reduction='none').sum(-1)
        grid = onet_mod.make_3d_grid([-0.5 + 1 / 32] * 3, [0.5 - 1 / 32] * 3, (16, 16, 16))
        z0 = torch.zeros(K, onet.z_dim).double()
        vlogits64 = onet64.decode(grid.double().expand(K, *grid.size()), z0, c64).logits
    sd = {k: v.numpy() for k, v in onet.encoder_latent.state_dict().items()}
    rm, rl = encoder_f64(sd, points, occ, codes)
    print("restatement vs torch float64: mean %.1e logstd %.1e, kl %.1e, bce %.1e"
          % (np.abs(rm - mean64.numpy()).max(), np.abs(rl - logstd64.numpy()).max(),
             np.abs(kl_f64(rm, rl) - kl64.numpy()).max(),
             np.abs(bce_rowsum_f64(logits64.numpy(), occ) - bce64.numpy()).max()))
    dev = np.array([np.abs(mean32.numpy() - mean64.numpy()).max(), np.abs(logstd32.numpy() - logstd64.numpy()).max(),
                    np.abs(kl32.numpy() - kl64.numpy()).max()])
    out.update(mean32=mean32.numpy(), logstd32=logstd32.numpy(), kl32=kl32.numpy(), bce32=bce32.numpy(),
               mean64=mean64.numpy(), logstd64=logstd64.numpy(), kl64=kl64.numpy(), bce64=bce64.numpy(),
               z64=z64.numpy(), voxel_logits64=vlogits64.numpy(), ref32_dev=dev)
    lattice = grid.numpy().astype(np.float64)
    out["gt_voxels"] = ((lattice ** 2).sum(-1) <= RADIUS ** 2).reshape(16, 16, 16)[None].repeat(K, 0).astype(np.float32)
    print("ref32_dev: mean %.2e logstd %.2e kl %.2e; logits in [%.3f, %.3f]; loss %.4f; kl %s; bce %s"
          % (dev[0], dev[1], dev[2], logits64.min(), logits64.max(), float(out["loss32"]), kl64.numpy(), bce64.numpy()))
    print("fp32 bce vs f64: %s (bound T * 1e-4 = %.3f)" % (np.abs(bce32.numpy() - bce64.numpy()), T * 1e-4))
    for thr in THRESHOLDS:
        tag = ("%g" % thr).replace(".", "")
        lt = np.log(thr) - np.log(1. - thr)
        near = np.abs(vlogits64.numpy() - lt) <= BAND
        ref = out["voxels_out_" + tag].reshape(K, -1)
        assert near.mean() <= BAND_CAP, near.mean()                       # the reference alone stays inside the cap
        assert np.array_equal(ref[~near], (vlogits64.numpy() >= lt)[~near])
        print("threshold %g: %.3f %% of the lattice within %g of it, %d of %d voxels set, IoU vs gt_voxels %s"
              % (thr, 100 * near.mean(), BAND, ref.sum(), ref.size, compute_iou(ref, out["gt_voxels"])))
    path = os.path.join(HERE, "F_LAT.npz")
    np.savez_compressed(path, **out)
    print("F_LAT.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    assert mf.REF
    main()
