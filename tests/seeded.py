"""Seeded networks of the tests, built once here: the F_GEN ONet in the reference's key order (encoder_latent.* first, as
the reference's ONet has it: the seed's stream is consumed in that order whether or not the network under test owns the
encoder), the stand-alone decoder, and the Dirichlet draws of the reference's refine_mesh.  A plain helper module, imported
the way normals_f64.py is."""
from collections import OrderedDict

import numpy as np

from rfdnet_amd import synthetic


def _placed(module):
    import torch
    return (module.cuda() if torch.cuda.is_available() else module).eval()


def onet_shapes(fx_gen):
    """ordered {name: shape} of the reference ONet's state_dict (F_GEN's onet_names / onet_shapes)"""
    return OrderedDict((str(n), tuple(int(x) for x in str(s).split(",")) if str(s) else ())
                       for n, s in zip(fx_gen["onet_names"], fx_gen["onet_shapes"]))


def onet_arrays(fx_gen, seed=202):
    """the F_GEN ONet's parameters as numpy, ordered, under the ONet's key names"""
    return synthetic.seeded_state_dict(onet_shapes(fx_gen), seed)


def decoder_arrays(fx_gen, seed=202):
    """the same ONet's decoder parameters under the decoder's own key names"""
    return OrderedDict((k[len("decoder."):], v) for k, v in onet_arrays(fx_gen, seed).items() if k.startswith("decoder."))


def seeded_onet(fx_gen, seed=202, generation=None, data=None):
    """ONet(Config({'generation': ..., 'data': ...})) holding the keys it owns of onet_arrays(fx_gen, seed): eval mode, on the
    GPU where there is one.  generation defaults to resolution_0 = 16, upsampling_steps = 1."""
    import torch
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.occupancy_net import ONet
    cfg = {'generation': dict({'resolution_0': 16, 'upsampling_steps': 1}, **(generation or {}))}
    if data is not None:
        cfg['data'] = data
    onet = ONet(Config(cfg))
    sd = onet_arrays(fx_gen, seed)
    onet.load_state_dict({k: torch.from_numpy(sd[k]) for k in onet.state_dict()})
    return _placed(onet)


def seeded_decoder(seed=1234):
    """the stand-alone DecoderCBatchNorm of the kernel tests, seeded in its own key order: eval mode, on the GPU where there
    is one"""
    from rfdnet_amd.iscnet.occ_decoder import DecoderCBatchNorm
    dec = DecoderCBatchNorm(dim=3, z_dim=32, c_dim=512, hidden_size=256)
    synthetic.load_seeded(dec, seed)
    return _placed(dec)


def reference_draws(n_faces, steps, seed):
    """what generator.py:259 draws in `steps` steps of one mesh after np.random.seed(seed)"""
    np.random.seed(seed)
    return np.stack([np.random.dirichlet((0.5, 0.5, 0.5), size=n_faces) for _ in range(steps)]).astype(np.float32)
