"""Latent encoder q(z | p, occ, c) with the reference's constructor, parameter names and forward signature
(models/iscnet/modules/encoder_latent.py:12-73), evaluated by csrc/encoder_latent.hip in five launches: one per-proposal
prologue (fc_c(c) and the -inf fill of the pooled rows), three stage kernels -- stage s recomputes stages 1 .. s-1 from the
16-byte input of a point and pools its own layer into a (K, 128) row -- and the head (fc_mean, fc_logstd and, when the
caller passes eps, z = mean + exp(logstd) eps and KL(q || N(0, 1))).  Nothing of width (K, T, *) is stored.

state_dict keys: fc_pos.{weight (128,3), bias}, fc_c.{weight (128,C), bias} (c_dim != 0), fc_0.{weight (128,1), bias},
fc_1.{weight (128,128), bias}, fc_2 / fc_3.{weight (128,256), bias}, fc_mean / fc_logstd.{weight (Z,128), bias}."""
import torch
import torch.nn as nn

from .. import _lib
from ..sa_fused import korder_next, pack_layer

HIDDEN = 128
LAUNCHES = 5                  # of forward() / posterior(): prep, three stages, head


class Encoder_Latent(nn.Module):
    def __init__(self, z_dim=128, c_dim=128, dim=3, leaky=False):
        super().__init__()
        if leaky:
            raise NotImplementedError("Encoder_Latent: leaky=True (leaky ReLU + mean pooling) is never instantiated by "
                                      "RfD-Net (occupancy_net.py:41) and has no kernel")
        if dim != 3:
            raise NotImplementedError("Encoder_Latent: the HIP encoder is built for dim=3")
        if not 1 <= z_dim <= 512:
            raise NotImplementedError("Encoder_Latent: 1 <= z_dim <= 512")
        self.z_dim = z_dim
        self.c_dim = c_dim
        self.fc_pos = nn.Linear(dim, HIDDEN)
        if c_dim != 0:
            self.fc_c = nn.Linear(c_dim, HIDDEN)
        self.fc_0 = nn.Linear(1, HIDDEN)
        self.fc_1 = nn.Linear(HIDDEN, HIDDEN)
        self.fc_2 = nn.Linear(2 * HIDDEN, HIDDEN)
        self.fc_3 = nn.Linear(2 * HIDDEN, HIDDEN)
        self.fc_mean = nn.Linear(HIDDEN, z_dim)
        self.fc_logstd = nn.Linear(HIDDEN, z_dim)

    def _packed(self):
        """the kernels' constant operands (include/rfd_latent.h), rebuilt only when a parameter changes"""
        params = list(self.parameters())
        key = _lib.tensor_key(*params)

        def build():
            sd = {k: v.detach().float() for k, v in self.state_dict().items()}
            dev = sd['fc_1.weight'].device
            korder = korder_next(HIDDEN // 2).to(dev)
            order = korder.reshape(-1)                                     # lane order: position 2j + h -> channel
            l0 = torch.cat([sd['fc_pos.weight'], sd['fc_0.weight']], dim=1)[order].contiguous()
            b0 = sd['fc_pos.bias'] + sd['fc_0.bias']
            wcT = None
            if self.c_dim != 0:
                b0 = b0 + sd['fc_c.bias']
                wcT = sd['fc_c.weight'][order].t().contiguous()
            wa = torch.stack([pack_layer(w, korder) for w in
                              (sd['fc_1.weight'], sd['fc_2.weight'][:, :HIDDEN], sd['fc_3.weight'][:, :HIDDEN])])
            wbT = torch.stack([sd['fc_2.weight'][:, HIDDEN:].t(), sd['fc_3.weight'][:, HIDDEN:].t()]).contiguous()
            b123 = torch.stack([sd['fc_1.bias'], sd['fc_2.bias'], sd['fc_3.bias']]).contiguous()
            whT = torch.cat([sd['fc_mean.weight'], sd['fc_logstd.weight']], dim=0).t().contiguous()
            bh = torch.cat([sd['fc_mean.bias'], sd['fc_logstd.bias']]).contiguous()
            return l0, b0[order].contiguous(), wcT, wa.contiguous(), wbT, b123, whT, bh
        return _lib.build_once(self.__dict__, '_rfd_latent_packed', key, build, params[0].device)

    def posterior(self, p, x, c=None, eps=None):
        """p (K,T,3), x (K,T) occupancies, c (K,c_dim) -> (mean, logstd, z, kl); z = mean + exp(logstd) eps and
        kl (K,) = KL(q || N(0,1)) summed over z_dim come out of the head kernel when eps (K,z_dim) is given, else None."""
        _lib.need_gpu(p)
        K, T, _ = p.shape
        dev = p.device
        p = p.detach().contiguous().float()
        x = x.detach().contiguous().float()
        assert x.shape == (K, T)
        l0, b0, wcT, wa, wbT, b123, whT, bh = self._packed()
        if self.c_dim != 0:
            c = c.detach().contiguous().float()
            assert c.shape == (K, self.c_dim)
        else:
            c = None
        Z = self.z_dim
        mean = torch.empty(K, Z, dtype=torch.float32, device=dev)
        logstd = torch.empty(K, Z, dtype=torch.float32, device=dev)
        z = kl = None
        if eps is not None:
            eps = eps.detach().contiguous().float()
            assert eps.shape == (K, Z) and eps.device == dev
            z, kl = torch.empty_like(mean), torch.empty(K, dtype=torch.float32, device=dev)
        if K == 0:
            return mean, logstd, z, kl
        if T == 0:
            raise ValueError("Encoder_Latent: the max over no points is undefined (T == 0)")
        bias0 = torch.empty(K, HIDDEN, dtype=torch.float32, device=dev)
        pool = torch.empty(3, K, HIDDEN, dtype=torch.float32, device=dev)
        _lib.call("rfd_latent_prep", dev, K, self.c_dim, _lib.ptr(c), _lib.ptr(wcT), b0.data_ptr(), bias0.data_ptr(),
                  pool.data_ptr())
        for stage in (1, 2, 3):
            _lib.call("rfd_latent_stage", dev, stage, K, T, p.data_ptr(), x.data_ptr(), l0.data_ptr(), bias0.data_ptr(),
                      wa.data_ptr(), wbT.data_ptr(), b123.data_ptr(), pool.data_ptr())
        _lib.call("rfd_latent_head", dev, K, Z, pool[2].data_ptr(), whT.data_ptr(), bh.data_ptr(), _lib.ptr(eps),
                  mean.data_ptr(), logstd.data_ptr(), _lib.ptr(z), _lib.ptr(kl))
        return mean, logstd, z, kl

    def forward(self, p, x, c=None, **kwargs):
        """-> (mean, logstd), each (K, z_dim)  (encoder_latent.py:49-73).  Inference only: no gradient."""
        mean, logstd, _, _ = self.posterior(p, x, c)
        return mean, logstd
