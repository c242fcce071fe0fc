"""CPU: the host side of the exact-fp32 matrix-core kernels (csrc/f32_wave32.h) -- sa_fused.pack_layer against the layout's
definition, element by element, and fold_bn.folded on a Conv2d + BatchNorm2d against the closed form."""
import numpy as np
import pytest
import torch

from rfdnet_amd import fold_bn, sa_fused


@pytest.mark.parametrize("C,K,first", [(32, 6, True), (64, 64, False)])
def test_pack_layer_against_its_definition(C, K, first):
    """element (b, j4, lane, e) = w[32b + (lane & 31), korder[4 j4 + e, lane >> 5]], zero where korder points past K.
    C = 32, K = 6: a first layer whose 8 padded input positions reach past the 6 real ones."""
    w = torch.from_numpy(np.random.default_rng(C + K).normal(size=(C, K)).astype(np.float32))
    korder = sa_fused.korder_first(((K + 7) // 8) * 4) if first else sa_fused.korder_next(K // 2)
    kj = korder.shape[0]
    assert korder.shape == (kj, 2)
    # the k order visits every input position once (and, in a first layer, the padding behind them)
    assert sorted(korder.reshape(-1).tolist()) == list(range(2 * kj)) and 2 * kj >= K
    packed = sa_fused.pack_layer(w, korder)
    assert packed.shape == (C // 32, kj // 4, 64, 4) and packed.is_contiguous() and packed.dtype == torch.float32
    past = 0
    for b in range(C // 32):
        for j4 in range(kj // 4):
            for lane in range(64):
                for e in range(4):
                    k = int(korder[4 * j4 + e, lane >> 5])
                    want = float(w[32 * b + (lane & 31), k]) if k < K else 0.0
                    past += k >= K
                    assert float(packed[b, j4, lane, e]) == want, (b, j4, lane, e)
    assert past == (C * (2 * kj - K))              # (32, 6): two padded positions per output channel


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_folded_conv2d_batchnorm2d_equals_the_closed_form(bias, affine):
    """W' = W s, b' = (b - mean) s + beta with s = gamma / sqrt(var + eps), against float64.  Bounds from the fp32 operations
    (u = 2^-24): var + eps, 1 / sqrt, * gamma, * W round 0.5 + 1.5 + 0.5 + 0.5 = 3 u into W' (4 u asked); b' adds the
    subtraction and the final sum: 5 u of |b - mean| |s| + |beta|."""
    g = torch.Generator().manual_seed(7 + 2 * bias + affine)
    conv = torch.nn.Conv2d(6, 32, 1, bias=bias)
    bn = torch.nn.BatchNorm2d(32, affine=affine)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        bn.running_mean.copy_(torch.randn(32, generator=g))
        bn.running_var.copy_(torch.rand(32, generator=g) * 2 + 0.1)
        if bias:
            conv.bias.copy_(torch.randn(32, generator=g))
        if affine:
            bn.weight.copy_(torch.randn(32, generator=g))
            bn.bias.copy_(torch.randn(32, generator=g))
    W, b = fold_bn.folded(conv, bn)
    assert W.shape == (32, 6) and b.shape == (32,) and W.is_contiguous() and b.is_contiguous()
    s = 1.0 / np.sqrt(bn.running_var.double().numpy() + bn.eps)
    beta = np.zeros(32)
    if affine:
        s, beta = s * bn.weight.detach().double().numpy(), bn.bias.detach().double().numpy()
    b0 = conv.bias.detach().double().numpy() if bias else np.zeros(32)
    W64 = conv.weight.detach().double().numpy().reshape(32, 6) * s[:, None]
    centred = (b0 - bn.running_mean.double().numpy()) * s
    u = 2.0 ** -24
    assert (np.abs(W.numpy() - W64) <= 4 * u * np.abs(W64)).all()
    assert (np.abs(b.numpy() - (centred + beta)) <= 5 * u * (np.abs(centred) + np.abs(beta))).all()
