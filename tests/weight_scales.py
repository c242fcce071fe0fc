"""Weights whose per-layer power-of-two exponents differ (occ_fold.choose_kw), for the split-f16 kernels' tests.

Every matrix kernel multiplies a layer's weights by 2^kw before the f16 hi/lo split and undoes the exponent elsewhere
(the decoder's table rows and pack kernels, the normals kernel's e0 / e1, the chain's os1..os3, the head's osa..osc).
Synthetic weights (synthetic.seeded_tensor: uniform +-1/sqrt(fan_in)) give every layer of one fan-in the same exponent,
so a mixed-up exponent goes unnoticed.  The helpers here return networks with the same structure whose exponents are
pairwise distinct, and assert that premise themselves.  Plain module (like dec_f64.py), CPU only, numpy / torch."""
from collections import OrderedDict

import numpy as np
import torch

from rfdnet_amd import occ_fold

BN_EPS = 1e-5

# per block: fc_0 scale (cancelled through bn_1's running statistics) and fc_1 scale (not cancelled)
FC0_SCALE = (0.3, 0.55, 0.045, 13.0, 1.9)
FC1_SCALE = (0.7, 0.2, 0.3, 1.2, 1.0)
OUTLIER_BLOCK = 1          # fc_0: max |w| from ONE weight 8x the rest of the block
POW2_BLOCK = 3             # fc_0: max |w| exactly a power of two: |w| * 2^kw == 16384, choose_kw's boundary
GAUSS_BLOCK = 4            # fc_1: drawn from N(0, s) instead of uniform: many small weights, a long tail


def _np(sd):
    return OrderedDict((k, np.array(v.detach().cpu().numpy() if torch.is_tensor(v) else v)) for k, v in sd.items())


def decoder_exponents(sd):
    """(kw0, kw1, kb0, kb1) exactly as DecoderCBatchNorm.packed_weights() / packed_weights_bwd() compute them"""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    fc0, fc1 = occ_fold.stacked_fc_weights(t)
    kw0 = [occ_fold.choose_kw([fc0[i]]) for i in range(5)]
    kw1 = occ_fold.choose_kw([fc1])
    b0 = fc1.flip(0).transpose(1, 2).contiguous()
    b1 = fc0.flip(0).transpose(1, 2).contiguous()
    kb0 = [occ_fold.choose_kw([b0[j]]) for j in range(5)]
    kb1 = occ_fold.choose_kw([b1])
    return kw0, kw1, kb0, kb1


def _scale_cancelled(sd, layer, bn, a):
    """layer's weight and bias * a (a > 0), undone by the BatchNorm that normalises its output: running_mean * a and
    running_var chosen so that running_var + eps == a^2 (var + eps) -- the same function up to fp32 rounding"""
    sd[layer + ".weight"] = (sd[layer + ".weight"].astype(np.float64) * a).astype(np.float32)
    sd[layer + ".bias"] = (sd[layer + ".bias"].astype(np.float64) * a).astype(np.float32)
    sd[bn + ".running_mean"] = (sd[bn + ".running_mean"].astype(np.float64) * a).astype(np.float32)
    v = sd[bn + ".running_var"].astype(np.float64)
    sd[bn + ".running_var"] = (a * a * (v + BN_EPS) - BN_EPS).astype(np.float32)


def spread_decoder(sd, seed=0, fc0_scale=FC0_SCALE, fc1_scale=FC1_SCALE, p=None, z=None, c=None, check_band=True):
    """sd: DecoderCBatchNorm state dict (torch or numpy) -> (sd' (numpy, a copy), kw0, kw1, kb0, kb1).

    Block i: fc_0 * fc0_scale[i], cancelled through bn_1's running statistics; fc_1 * fc1_scale[i], NOT cancelled (the
    float64 reference sees the changed network).  On top: block OUTLIER_BLOCK's fc_0 gets one weight 8x the block's
    max |w|, block POW2_BLOCK's fc_0 is rescaled so that its max |w| is exactly a power of two (the scale cancelled like
    the others), block GAUSS_BLOCK's fc_1 is redrawn from a Gaussian of the uniform draw's variance.

    Asserts the premise: kw0 pairwise distinct and kw1 none of them, kb0 pairwise distinct, neither kw0 nor kb0 equal
    to its own reverse, kb1 != kw1; with p, z, c given and check_band, also that the activations stay inside the f16
    range at the default scale (amax * 2^ka < 65504, tests/dec_f64.py)."""
    sd = _np(sd)
    rng = np.random.default_rng(seed)
    for i in range(5):
        b = "blocks.%d." % i
        a = float(fc0_scale[i])
        if i == POW2_BLOCK:
            m = float(np.abs(sd[b + "fc_0.weight"]).max()) * a
            a *= 2.0 ** np.round(np.log2(m)) / m                     # max |w| * a == 2^e (up to fp32 rounding, fixed below)
        _scale_cancelled(sd, b + "fc_0", b + "bn_1.bn", a)
        w = sd[b + "fc_0.weight"]
        if i == OUTLIER_BLOCK:
            flat = w.reshape(-1)
            j = int(rng.integers(flat.size))
            flat[j] = np.float32(8.0 * np.abs(flat).max() * (1 if flat[j] >= 0 else -1))
        if i == POW2_BLOCK:
            flat = w.reshape(-1)
            j = int(np.abs(flat).argmax())
            e = np.round(np.log2(abs(float(flat[j]))))
            np.clip(flat, -(2.0 ** e), 2.0 ** e, out=flat)
            flat[j] = np.float32(np.copysign(2.0 ** e, flat[j]))
            assert float(np.abs(flat).max()) == 2.0 ** e
        w1 = sd[b + "fc_1.weight"].astype(np.float64)
        if i == GAUSS_BLOCK:
            bound = np.abs(w1).max()
            w1 = rng.normal(0.0, bound / np.sqrt(3.0), w1.shape)
        sd[b + "fc_1.weight"] = (w1 * fc1_scale[i]).astype(np.float32)
        sd[b + "fc_1.bias"] = (sd[b + "fc_1.bias"].astype(np.float64) * fc1_scale[i]).astype(np.float32)
    kw0, kw1, kb0, kb1 = decoder_exponents(sd)
    assert len(set(kw0)) == 5 and kw1 not in kw0, (kw0, kw1)
    assert len(set(kb0)) == 5, kb0
    assert kw0 != kw0[::-1] and kb0 != kb0[::-1], (kw0, kb0)
    assert kb1 != kw1, (kb1, kw1)
    w = sd["blocks.%d.fc_0.weight" % POW2_BLOCK]
    assert float(np.abs(w).max()) * 2.0 ** kw0[POW2_BLOCK] == 16384.0          # exactly at choose_kw's boundary
    if p is not None and check_band:
        from dec_f64 import decoder_f64
        _, amax = decoder_f64(sd, p, z, c, return_amax=True)
        assert amax * 2.0 ** occ_fold.KA < 65504.0, amax
    return sd, kw0, kw1, kb0, kb1


def spread_layers(layers, scales, packed):
    """layers: a chain [(W (N,K), b (N,)), ...] in which every layer but the last is followed by a ReLU (or a max over
    points); scales: one positive factor per layer but the last.  Layer i's output is multiplied by scales[i] and the
    next layer's weight divided by it (W_i * s_i / s_(i-1), b_i * s_i; the ReLU is positively homogeneous), so the
    chain computes the same function with other weight exponents.  packed: indices of the layers whose exponent a
    kernel uses -- their choose_kw values must be pairwise distinct (asserted).  -> (new layers, [exponent of each
    packed layer])"""
    assert len(scales) == len(layers) - 1 and all(s > 0 for s in scales)
    s = list(scales) + [1.0]
    out = []
    prev = 1.0
    for (W, b), si in zip(layers, s):
        out.append(((W.double() * (si / prev)).float(), None if b is None else (b.double() * si).float()))
        prev = si
    sw = [occ_fold.choose_kw([out[i][0]]) for i in packed]
    assert len(set(sw)) == len(sw), sw
    return out, sw


def _pointseg_pairs(seg):
    """(layer, BatchNorm, [(consumer layer, input column slice)]) of PointSeg's BN-followed layers: the layer's BN output
    goes through a ReLU (or a max over points) into the consumers' input columns"""
    enc = seg.feat
    every = slice(None)
    pairs = []
    for t in (enc.stn, enc.fstn):
        pairs += [(t.conv1, t.bn1, [(t.conv2, every)]), (t.conv2, t.bn2, [(t.conv3, every)]),
                  (t.conv3, t.bn3, [(t.fc1, every)]), (t.fc1, t.bn4, [(t.fc2, every)]), (t.fc2, t.bn5, [(t.fc3, every)])]
    # the encoder's first layer feeds the feature STN and (through the bmm with its output) conv2 and the head's
    # point-feature columns; conv3 (no ReLU, but a max: positively homogeneous as well) the head's global columns
    pairs += [(enc.conv1, enc.bn1, [(enc.fstn.conv1, every), (enc.conv2, every), (seg.conv1, slice(1024, None))]),
              (enc.conv2, enc.bn2, [(enc.conv3, every)]),
              (enc.conv3, enc.bn3, [(seg.conv1, slice(0, 1024))]),
              (seg.conv1, seg.bn1, [(seg.conv2, every)]), (seg.conv2, seg.bn2, [(seg.conv3, every)]),
              (seg.conv3, seg.bn3, [(seg.conv4, every)])]
    return pairs


def spread_module(module, seed):
    """PointSeg (in place, eval mode): every Conv1d / Linear followed by a BatchNorm gets its own power-of-two-free scale
    a in [1/8, 8].  Scaling the layer and cancelling it in the BatchNorm's running statistics alone would leave the
    FOLDED weight (fold_bn.folded: W * gamma / sqrt(var + eps)) -- the only one the fused kernels see -- unchanged, so
    the scale is carried through the BatchNorm's affine output instead (weight, bias * a) and undone in the input
    columns of the layers that consume it; the layer's own weight and bias are scaled by a as well, cancelled through
    the running statistics as in spread_decoder.  Same function up to fp32 rounding.  Asserts that the exponents of
    each fused launch differ (chain: the packed layers of STN3d (mode 1), STNkd (mode 2), the encoder (mode 0); the
    head: Wa, Wb, Wc).  Returns {launch: exponents}."""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer, bn, consumers in _pointseg_pairs(module):
            a = float(2.0 ** rng.uniform(-3.0, 3.0))
            u = float(2.0 ** rng.uniform(-1.0, 1.0))
            layer.weight.mul_(u)
            layer.bias.mul_(u)
            bn.running_mean.mul_(u)
            bn.running_var.copy_(((bn.running_var.double() + bn.eps) * u * u - bn.eps).float())
            bn.weight.mul_(a)
            bn.bias.mul_(a)
            for cons, cols in consumers:
                cons.weight[:, cols].div_(a)
    enc = module.feat

    def fw(layer, bn):                                     # fold_bn.folded's weight, without touching its cache
        W = layer.weight.detach().reshape(layer.weight.shape[0], -1)
        return W * (torch.rsqrt(bn.running_var + bn.eps) * bn.weight.detach())[:, None]
    exps = {
        "stn (mode 1)": [occ_fold.choose_kw([fw(enc.stn.conv2, enc.stn.bn2)]), occ_fold.choose_kw([fw(enc.stn.conv3, enc.stn.bn3)])],
        "fstn (mode 2)": [occ_fold.choose_kw([fw(t, b)]) for t, b in ((enc.fstn.conv1, enc.fstn.bn1),
                                                                     (enc.fstn.conv2, enc.fstn.bn2),
                                                                     (enc.fstn.conv3, enc.fstn.bn3))],
        "encoder (mode 0)": [occ_fold.choose_kw([fw(enc.conv2, enc.bn2)]), occ_fold.choose_kw([fw(enc.conv3, enc.bn3)])],
        "head": [occ_fold.choose_kw([fw(module.conv1, module.bn1)[:, 1024:]]),
                 occ_fold.choose_kw([fw(module.conv2, module.bn2)]), occ_fold.choose_kw([fw(module.conv3, module.bn3)])],
    }
    for k, v in exps.items():
        assert len(set(v)) == len(v), (k, v)
    return exps
