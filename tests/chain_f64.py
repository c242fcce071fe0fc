"""float64 restatement of the fused PointNet chains and of PointSeg's per-point head (csrc/pointseg_chain.hip), in numpy:
    chain:  x (M, d) -> [d -> 64, ReLU] -> 64 -> 128, ReLU -> 128 -> c3 [, ReLU] -> max over each proposal's P rows
    head:   x (M, 64) -> 512 (+ gbias[proposal], ReLU) -> 256 (ReLU) -> 128 (ReLU) -> n_cls scores
A layer is (W (N, K), b (N,)) with the BatchNorm folded in; layer1 is None where x already is the 64-wide feature
(mode 0).  Arguments may be numpy arrays or torch tensors on any device; everything is computed in float64 on the host
and returned as numpy float64.  Unlike the kernel, chain_rows() keeps the rows BEFORE the pool, so a test can tell which
row decides a channel and by how much."""
import numpy as np


def f64(a):
    """numpy float64 of a numpy array or a torch tensor (any device)"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _lin(h, layer):
    return h @ f64(layer[0]).T + f64(layer[1])


def chain_rows(x, layer1, layer2, layer3, relu3):
    """(M, c3): every row's output of the chain, before the pool"""
    h = f64(x)
    if layer1 is not None:
        h = np.maximum(_lin(h, layer1), 0.)
    h = np.maximum(_lin(h, layer2), 0.)
    h = _lin(h, layer3)
    return np.maximum(h, 0.) if relu3 else h


def pool(rows, P):
    """(M, c3) rows -> (M / P, c3): the max over each proposal's P rows"""
    M, c3 = rows.shape
    assert M % P == 0
    return rows.reshape(M // P, P, c3).max(axis=1)


def chain_pool(x, layer1, layer2, layer3, P, relu3):
    return pool(chain_rows(x, layer1, layer2, layer3, relu3), P)


def head_hidden(x, P, Wa, gbias, layer_b, layer_c):
    """(M, 128): the head's last hidden layer (it does not depend on the class count)"""
    h = np.maximum(f64(x) @ f64(Wa).T + np.repeat(f64(gbias), P, axis=0), 0.)
    h = np.maximum(_lin(h, layer_b), 0.)
    return np.maximum(_lin(h, layer_c), 0.)


def head_scores(x, P, Wa, gbias, layer_b, layer_c, Wd, bd):
    """(M, n_cls) raw class scores"""
    return _lin(head_hidden(x, P, Wa, gbias, layer_b, layer_c), (Wd, bd))


def tolerance(ref):
    """the bound of tests/test_gpu_chain.py: max |out - ref| < 2e-5 max(1, max |ref|)"""
    return 2e-5 * max(1., float(np.abs(ref).max()))


def decisive(ref):
    """A candidate decides a channel when it beats the other by at least this much: 100 x the tolerance, so no
    admissible rounding of either can change the winner."""
    return 100. * tolerance(ref)
