"""Occupancy network wrapper (models/iscnet/modules/occupancy_net.py:12-189): holds the decoder under the reference's
attribute name (`decoder` => state_dict keys completion.decoder.*), the prior over z, the mesh generator and -- once
enable_latent_encoder() is called -- the latent encoder q(z | p, occ, c) with the completion loss of the test mode
(compute_loss: KL + BCE + the 16^3 voxel example)."""
import torch
import torch.distributions as dist
import torch.nn as nn

from .. import _lib
from .generator import Generator3D
from .occ_decoder import DecoderCBatchNorm, logit_threshold
from .registers import MODULES


@MODULES.register_module
class ONet(nn.Module):
    def __init__(self, cfg, optim_spec=None):
        super().__init__()
        self.optim_spec = optim_spec
        data = cfg.config['data']
        self.z_dim = data['z_dim']
        self.use_cls_for_completion = data['use_cls_for_completion']
        base = data['c_dim'] if data['skip_propagate'] else 128
        c_dim = self.use_cls_for_completion * cfg.dataset_config.num_class + base
        self.threshold = data['threshold']
        # the latent encoder q(z|p,occ,c) (encoder_latent.py) serves compute_loss only -- the ground-truth-dependent
        # completion loss of the reference's training AND test mode (network.py:140, testing.py:64); generation uses the
        # prior mean (occupancy_net.py:138-143).  Opt-in (enable_latent_encoder / data.latent_encoder): the default
        # state_dict is the decoder's alone.
        self.c_dim = c_dim
        self.encoder_latent = None
        self.decoder = DecoderCBatchNorm(dim=3, z_dim=self.z_dim, c_dim=c_dim)
        if data.get('latent_encoder'):
            self.enable_latent_encoder()
        gen = cfg.config.get('generation')
        if gen and gen['generate_mesh']:
            self.generator = Generator3D(
                self, threshold=data['threshold'], resolution0=gen['resolution_0'],
                upsampling_steps=gen['upsampling_steps'], sample=gen['use_sampling'],
                refinement_step=0, simplify_nfaces=gen['simplify_nfaces'],
                with_normals=gen.get('with_normals', False),
                preprocessor=None)
            if gen['refinement_step']:
                self.generator.set_refinement(gen['refinement_step'])
            if gen.get('decimate_cells'):       # not a key of the reference's config files: absent = off
                self.generator.set_decimation(gen['decimate_cells'])
            if gen.get('simplify_faces'):       # nor is this one (the reference's simplify_nfaces still raises)
                self.generator.set_simplification(gen['simplify_faces'])
            if gen.get('keep_components'):      # nor this one: 'largest' or a fraction (Generator3D.set_components)
                self.generator.set_components(gen['keep_components'])

    def enable_latent_encoder(self):
        """Attach the latent encoder (z_dim > 0; occupancy_net.py:40-43) in front of the decoder, so that state_dict()
        is the reference ONet's full key list in its order and load_weight() keeps a checkpoint's
        completion.encoder_latent.* tensors.  New parameters are initialised like nn.Linear's and live on the decoder's
        device.  Call it before the network is shared (worker_view)."""
        if self.z_dim == 0 or self.encoder_latent is not None:
            return self
        from .encoder_latent import Encoder_Latent
        enc = Encoder_Latent(dim=3, z_dim=self.z_dim, c_dim=self.c_dim).to(self.decoder.fc_p.weight.device)
        enc.train(self.training)
        rest = dict(self._modules)
        self.__dict__.pop('encoder_latent', None)
        self._modules.clear()
        self._modules['encoder_latent'] = enc
        self._modules.update(rest)
        return self

    def infer_z(self, p, occ, c, device, **kwargs):
        """-> q(z | p, occ, c) = Normal(mean, exp(logstd))  (occupancy_net.py:158-175)"""
        if self.encoder_latent is not None:
            mean_z, logstd_z = self.encoder_latent(p, occ, c, **kwargs)
        else:
            mean_z = torch.empty(p.size(0), 0, device=device)
            logstd_z = torch.empty(p.size(0), 0, device=device)
        return dist.Normal(mean_z, torch.exp(logstd_z))

    def voxel_grid_points(self, device):
        """the 16^3 lattice of compute_loss's shape example: make_3d_grid([-0.5 + 1/32] * 3, [0.5 - 1/32] * 3, (16,) * 3)
        (external/common.py:157-176), x slowest"""
        lin = torch.linspace(-0.5 + 1 / 32, 0.5 - 1 / 32, 16)
        return torch.stack(torch.meshgrid(lin, lin, lin, indexing='ij'), dim=-1).view(-1, 3).to(device)

    def logit_threshold(self):
        return logit_threshold(self.threshold)

    @torch.no_grad()
    def compute_loss(self, input_features_for_completion, input_points_for_completion,
                     input_points_occ_for_completion, cls_codes_for_completion, export_shape=False, eps=None,
                     return_terms=False):
        """The completion loss of occupancy_net.py:59-109 as an evaluation quantity (no gradient):
        features (K,D), points (K,T,3), occupancies (K,T), class codes (K,C) -> (loss, voxels_out):
        loss = mean_k KL(q(z|p,occ,c) || N(0,1)) + mean_k sum_t BCE-with-logits(decode(p, z, c), occ), z = q.rsample();
        voxels_out (K,16,16,16) bool with export_shape (the decoder at the prior mean on the 16^3 lattice, thresholded),
        else None.
        eps (K, z_dim): the standard-normal draw of rsample (z = mean + exp(logstd) eps).  None draws torch.randn on the
        device: the reference's distribution, but another stream than its CPU draw -- pass eps to reproduce a run.
        return_terms: a third value {'kl','bce' (K,), 'mean','logstd','z' (K,z_dim), 'voxel_logits' (K,4096) or None}.
        Launches: 5 (encoder) + the decoder's forward + 1 (BCE row sums) + a few elementwise torch ops."""
        feat, p, occ = input_features_for_completion, input_points_for_completion, input_points_occ_for_completion
        if self.z_dim > 0 and self.encoder_latent is None:
            raise RuntimeError("ONet.compute_loss needs the latent encoder (z_dim = %d): call enable_latent_encoder() "
                               "(or set data.latent_encoder) and load its weights" % self.z_dim)
        _lib.need_gpu(feat, p, occ)
        device = feat.device
        K = feat.size(0)
        if self.use_cls_for_completion:
            feat = torch.cat([feat, cls_codes_for_completion.to(device).float()], dim=-1)
        feat = feat.float()
        occ = occ.contiguous().float()
        terms = {'kl': None, 'mean': None, 'logstd': None, 'voxel_logits': None}
        if self.z_dim > 0:
            if eps is None:
                eps = torch.randn(K, self.z_dim, device=device)
            mean, logstd, z, kl = self.encoder_latent.posterior(p, occ, feat, eps.to(device))
            loss = kl.mean()
            terms.update(kl=kl, mean=mean, logstd=logstd)
        else:
            z = torch.empty(K, 0, device=device)
            loss = 0.
        logits = self.decode(p, z, feat).logits
        bce = bce_logits_rowsum(logits, occ)
        loss = loss + bce.mean()
        terms.update(bce=bce, z=z)
        voxels_out = None
        if export_shape:
            grid = self.voxel_grid_points(device)
            z0 = self.get_z_from_prior((K,), device, sample=False)
            vlogits = self.decode(grid.expand(K, *grid.size()), z0, feat).logits
            voxels_out = (vlogits >= self.logit_threshold()).view(K, 16, 16, 16)
            terms['voxel_logits'] = vlogits
        return (loss, voxels_out, terms) if return_terms else (loss, voxels_out)

    def get_prior_z(self, z_dim, device):
        return dist.Normal(torch.zeros(z_dim, device=device), torch.ones(z_dim, device=device))

    def get_z_from_prior(self, size=torch.Size([]), device='cuda', sample=False):
        p0_z = self.get_prior_z(self.z_dim, device)
        if sample:
            return p0_z.sample(size)
        z = p0_z.mean
        return z.expand(*size, *z.size())

    def decode(self, input_points_for_completion, z, features, **kwargs):
        """-> Bernoulli over occupancy, logits (B,T)  (occupancy_net.py:147-156)"""
        logits = self.decoder(input_points_for_completion, z, features, **kwargs)
        return dist.Bernoulli(logits=logits)

    def forward(self, input_points_for_completion, input_features_for_completion,
                cls_codes_for_completion, sample=False, **kwargs):
        device = input_features_for_completion.device
        if self.use_cls_for_completion:
            input_features_for_completion = torch.cat(
                [input_features_for_completion, cls_codes_for_completion.to(device).float()], dim=-1)
        z = self.get_z_from_prior((input_points_for_completion.size(0),), device, sample=sample)
        return self.decode(input_points_for_completion, z, input_features_for_completion, **kwargs)


def bce_logits_rowsum(logits, target):
    """(K,T) f32 device tensors (unit stride along T) -> (K,) f32: sum_t binary_cross_entropy_with_logits, one
    rfd_bce_logits_rowsum launch (f64 row sums in a fixed order: deterministic)"""
    _lib.need_gpu(logits, target)
    K, T = logits.shape
    assert target.shape == (K, T) and logits.dtype == torch.float32 and target.dtype == torch.float32
    (logits, ld_l), (target, ld_t) = _lib.rows(logits), _lib.rows(target)
    out = torch.empty(K, dtype=torch.float32, device=logits.device)
    _lib.call("rfd_bce_logits_rowsum", logits.device, K, T, logits.data_ptr(), ld_l, target.data_ptr(), ld_t,
              out.data_ptr())
    return out
