"""float64 restatement of Encoder_Latent.forward (encoder_latent.py:49-73) and of the two loss terms of
ONet.compute_loss (occupancy_net.py:78-93) in numpy: the ground truth the device encoder is held to (an fp32 evaluation
of the module in another summation order is no closer to it than the reference's own fp32 run is)."""
import numpy as np


def encoder_f64(sd, p, occ, c, return_pools=False):
    """sd: encoder_latent state_dict (numpy arrays, reference key names); p (K,T,3), occ (K,T), c (K,C) or None
    -> mean, logstd (K,Z) float64"""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    p, occ = np.asarray(p, dtype=np.float64), np.asarray(occ, dtype=np.float64)
    lin = lambda name, x: x @ g(name + ".weight").T + g(name + ".bias")
    relu = lambda x: np.maximum(x, 0)
    net = lin("fc_0", occ[..., None]) + lin("fc_pos", p)
    if "fc_c.weight" in sd:
        net = net + lin("fc_c", np.asarray(c, dtype=np.float64))[:, None, :]
    net = lin("fc_1", relu(net))
    pools = []
    for name in ("fc_2", "fc_3"):
        pooled = net.max(axis=1, keepdims=True)
        pools.append(pooled[:, 0])
        net = lin(name, relu(np.concatenate([net, np.broadcast_to(pooled, net.shape)], axis=2)))
    pooled = net.max(axis=1)
    pools.append(pooled)
    out = lin("fc_mean", pooled), lin("fc_logstd", pooled)
    return out + (pools,) if return_pools else out


def kl_f64(mean, logstd):
    """KL(N(mean, exp(logstd)) || N(0, 1)) summed over the last axis (torch.distributions.kl._kl_normal_normal)"""
    mean, logstd = np.asarray(mean, dtype=np.float64), np.asarray(logstd, dtype=np.float64)
    return (0.5 * (np.exp(2 * logstd) + mean ** 2 - 1) - logstd).sum(-1)


def bce_rowsum_f64(logits, target):
    """sum over the last axis of binary_cross_entropy_with_logits: max(x, 0) - x y + log1p(exp(-|x|))"""
    x, y = np.asarray(logits, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum(-1)


def compute_iou(occ1, occ2):
    """What the reference's compute_iou (external/common.py:7-35) gives for two batches (K, ...) of occupancy arrays:
    both thresholded at 0.5, the counts as float32 (exact up to 2^24 cells), their float32 quotient; 0 / 0 = NaN"""
    a = np.asarray(occ1).reshape(len(occ1), -1) >= 0.5
    b = np.asarray(occ2).reshape(len(occ2), -1) >= 0.5
    inter = np.count_nonzero(a & b, axis=1).astype(np.float32)
    union = np.count_nonzero(a | b, axis=1).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / union
