"""GPU (-m gpu): the split-f16 kernels on weights whose per-layer exponents differ (tests/weight_scales.py).

Every matrix kernel scales a layer's weights by 2^kw before the f16 split and undoes kw elsewhere; with the synthetic
weights every layer of one fan-in has the same kw, so a swapped, reversed or shared exponent passes the rest of the suite.
Here the decoder's kw0 are five different values and kw1 none of them (and kb0 / kb1 of the normals kernel's backward
stream likewise), the chain's sw1..sw3 and the head's swa..swc are pairwise distinct.  Contracts: those of the logit-band
tests (tests/test_gpu_decoder.py), of the normals tests (tests/test_gpu_normals.py) and of the chain tests
(tests/test_gpu_chain.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from rfdnet_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dec_f64 import decoder_f64  # noqa: E402
from normals_f64 import normals_of  # noqa: E402
from weight_scales import spread_decoder, spread_layers, spread_module  # noqa: E402

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-4
CHAIN_TOL = 2e-5


@pytest.fixture(autouse=True)
def main_kernel_only(request, hip):
    """as in tests/test_gpu_decoder.py: launches stay on the main kernel unless the test is marked `tail`"""
    if request.node.get_closest_marker("tail"):
        yield
        return
    old = hip.lib().rfd_occ_set_tail_tiles(0)
    try:
        yield
    finally:
        hip.lib().rfd_occ_set_tail_tiles(old)


def _codes(K=4, T=2000, cs=1.0, seed=0):
    rng = np.random.default_rng(seed)
    p = ((rng.random((K, T, 3)) - 0.5) * 1.1).astype(np.float32)
    z = rng.normal(0, 1, (K, 32)).astype(np.float32)
    c = (rng.normal(0, 1, (K, 512)) * cs).astype(np.float32)
    return p, z, c


def spread_dec(p, z, c, kernel="w8", seed=1234, check_band=True):
    """a FRESH decoder (ka is lowered for good once it falls back) with weight_scales.spread_decoder's weights"""
    from rfdnet_amd.iscnet.occ_decoder import DecoderCBatchNorm
    dec = DecoderCBatchNorm(dim=3, z_dim=32, c_dim=512, hidden_size=256)
    synthetic.load_seeded(dec, seed)
    sd, kw0, kw1, kb0, kb1 = spread_decoder(dec.state_dict(), p=p, z=z, c=c, check_band=check_band)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    dec = dec.cuda().eval()
    dec.kernel = kernel
    _, pk0, pk1 = dec.packed_weights()
    assert (pk0, pk1) == (kw0, kw1)                  # the kernel is handed the distinct exponents
    return dec, sd, (kw0, kw1, kb0, kb1)


def _run(dec, p, z, c):
    with torch.no_grad():
        return dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())


def _band_contract(name, o, exact, ref32):
    e_hip, e_or = np.abs(o - exact).max(), np.abs(ref32 - exact).max()
    print("%s: |logit| max %.2f, |HIP-f64| %.2e, |oracle32-f64| %.2e" % (name, np.abs(exact).max(), e_hip, e_or))
    assert e_hip <= LOGIT_TOL, (name, e_hip)
    assert e_hip <= 1.25 * e_or + 2e-6, (name, e_hip, e_or)


@pytest.mark.parametrize("kern", ["w8", "w4"])
def test_decoder_with_distinct_weight_exponents(hip, oracle, kern):
    """K = 4 proposals x 2000 points (T not a multiple of the 128-point tile), non-zero z: the main w8 kernel and the w4
    kernel against the float64 module, under the logit-band contract"""
    p, z, c = _codes()
    dec, sd, kws = spread_dec(p, z, c, kernel=kern)
    exact = decoder_f64(sd, p, z, c)
    ref32 = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
    out = _run(dec, p, z, c)
    hip.device_status()
    assert dec.ka == 6
    _band_contract("%s, kw0 %s kw1 %d" % (kern, kws[0], kws[1]), out.cpu().numpy().astype(np.float64), exact, ref32)


@pytest.mark.tail
def test_tail_decoder_with_distinct_weight_exponents(hip, oracle):
    """the tail route (csrc/occ_decoder_tail.hip) on the same launch: bit-identical to the main kernel, and in contract"""
    lib = hip.lib()
    p, z, c = _codes()
    dec, sd, _ = spread_dec(p, z, c)
    n_tiles = p.shape[0] * ((p.shape[1] + 127) // 128)
    default = lib.rfd_occ_set_tail_tiles(-1)
    try:
        lib.rfd_occ_set_tail_tiles(0)
        ref = _run(dec, p, z, c)
        lib.rfd_occ_set_tail_tiles(n_tiles)
        got = _run(dec, p, z, c)
    finally:
        lib.rfd_occ_set_tail_tiles(default)
    hip.device_status()
    assert dec.ka == 6
    assert torch.equal(got, ref)
    exact = decoder_f64(sd, p, z, c)
    ref32 = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
    _band_contract("tail", got.cpu().numpy().astype(np.float64), exact, ref32)


def _ragged_tiles(K=6, seed=4, skip_every=5):
    """tiles per proposal 1..6, every skip_every-th tile skipped (tile_prop < 0)"""
    rng = np.random.default_rng(seed)
    tile_prop = np.repeat(np.arange(K, dtype=np.int32), rng.integers(1, 7, K))
    tile_prop[::skip_every] = -1
    pts = ((rng.random((tile_prop.shape[0] * 128, 3)) - 0.5) * 1.1).astype(np.float32)
    return tile_prop, pts


@pytest.mark.tail
def test_decode_tiles_and_fused_scatter_with_distinct_weight_exponents(hip):
    """decode_tiles with a ragged tile count per proposal and skipped tiles, plain and through the fused MISE scatter
    (rfd_occ_decode_scatter_w8, the path generate_grids takes), main and tail route: every route bit-identical to the
    main kernel's plain logits, which are within 1e-4 of the float64 module"""
    lib = hip.lib()
    K = 6
    tile_prop, pts = _ragged_tiles(K)
    _, z, c = _codes(K=K, T=1, seed=9)
    dec, sd, _ = spread_dec(pts.reshape(1, -1, 3)[:, :2048].repeat(K, 0), z, c)
    n_tiles = tile_prop.shape[0]
    tp = torch.from_numpy(tile_prop).cuda()
    pt = torch.from_numpy(pts).cuda()
    keep = np.repeat(tile_prop >= 0, 128)
    # the scatter's slots: a tile's position among its proposal's unskipped tiles, a few padding slots
    rank = np.zeros(n_tiles, dtype=np.int64)
    seen = {}
    for t, k in enumerate(tile_prop):
        if k >= 0:
            rank[t] = seen.get(int(k), 0)
            seen[int(k)] = rank[t] + 1
    lin_h = np.repeat(rank, 128) * 128 + np.arange(n_tiles * 128) % 128
    lin_h[~keep] = -1
    lin_h[::37] = -1
    lin = torch.from_numpy(lin_h.astype(np.int32)).cuda()
    n_per = 128 * max(seen.values())
    default = lib.rfd_occ_set_tail_tiles(-1)
    plain, scat = [], []
    try:
        with torch.no_grad():
            table, fcp = dec.fold(torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
            for tail in (0, n_tiles):
                lib.rfd_occ_set_tail_tiles(tail)
                plain.append(dec.decode_tiles(pt, tp, table, fcp))
                values = torch.full((K, n_per), float("nan"), device="cuda")
                pstate = torch.ones(K, n_per, dtype=torch.uint8, device="cuda")
                dec.decode_tiles(pt, tp, table, fcp, scatter=(lin, values, pstate))
                scat.append((values, pstate))
    finally:
        lib.rfd_occ_set_tail_tiles(default)
    hip.device_status()
    ref = plain[0].cpu().numpy()
    assert np.array_equal(plain[1].cpu().numpy()[keep], ref[keep])
    real = lin_h >= 0
    prop = np.repeat(tile_prop, 128)
    for values, pstate in scat:
        known = pstate.cpu().numpy() == 2
        assert int(known.sum()) == int(real.sum())
        assert np.array_equal(values.cpu().numpy()[prop[real], lin_h[real]], ref[real])
    worst = 0.0
    for k in range(K):
        m = prop == k
        exact = decoder_f64(sd, pts[m][None], z[k:k + 1], c[k:k + 1])[0]
        worst = max(worst, float(np.abs(ref[m] - exact).max()))
    print("ragged tiles, %d tiles (%d skipped): max |HIP - f64| = %.2e" % (n_tiles, int((tile_prop < 0).sum()), worst))
    assert worst <= LOGIT_TOL


@pytest.mark.parametrize("kern", ["w8", "w4"])
def test_decoder_fallback_scale_with_distinct_weight_exponents(hip, oracle, kern):
    """codes x10 on the spread weights: activations up to ~2240 (x 2^6 beyond the f16 range, x 2^3 inside) -- the launch
    is answered by the fallback scale 2^3 and the logits stay fp32-class relative to max |logit| (~570), as in
    test_decoder_logit_band_beyond_the_default_scale.  (Codes x7, that test's factor, keeps these weights' activations
    below 300: the spread's fc_1 scales shrink the residual stream, so the band is reached at x10.)  Measured on MI355X:
    |HIP - f64| 1.03e-3 (w8) and 1.27e-3 (w4), 1.8e-6 and 2.2e-6 of max |logit|; the fp32 oracle 1.15e-3."""
    p, z, c = _codes(T=2048, cs=10.0)
    z[:] = 0.0
    dec, sd, _ = spread_dec(p, z, c, kernel=kern, check_band=False)
    exact, amax = decoder_f64(sd, p, z, c, return_amax=True)
    assert amax * 64 > 65504 > amax * 8
    ref32 = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
    with pytest.warns(RuntimeWarning, match="f16 range"):
        out = _run(dec, p, z, c)
    hip.device_status()
    assert dec.ka == 3
    o = out.cpu().numpy().astype(np.float64)
    m = np.abs(exact).max()
    e_hip, e_or = np.abs(o - exact).max(), np.abs(ref32 - exact).max()
    print("codes x10 %s: |logit| max %.1f, act max %.0f: |HIP-f64| %.2e (%.1e relative), |oracle32-f64| %.2e"
          % (kern, m, amax, e_hip, e_hip / m, e_or))
    assert e_hip / m < 4e-6
    assert e_hip <= 1.25 * e_or + 2e-6


def test_normals_with_distinct_weight_exponents(hip):
    """test_normals_ragged_meshes_against_float64 on the spread decoder: the normals kernel combines kw0 / kw1 with the
    backward stream's kb0 / kb1 (e1[j] = kw[4-j] - kw[6+j], e0 = kw[5] - kw[11]), here all different.  Measured on
    MI355X: 15 218 vertices, 125 in the exception set (0.8 %, nearly all near a ReLU kink), raw gradient 5.4e-5 relative"""
    from test_gpu_normals import check, f64_and_f32, kernel_normals, ragged_case
    verts, vend, z, c = ragged_case()
    dec, sd, (kw0, kw1, kb0, kb1) = spread_dec(np.asarray(verts[:2048], np.float32)[None].repeat(4, 0), z[:4], c[:4])
    _, pb0, pb1 = dec.packed_weights_bwd()
    assert (pb0, pb1) == (kb0, kb1)
    kn, kg = kernel_normals(dec, verts, vend, z, c, return_grad=True)
    hip.device_status()
    g64, g32, mg = f64_and_f32(sd, verts, vend, z, c)
    check("spread exponents kw0 %s kw1 %d kb0 %s kb1 %d" % (kw0, kw1, kb0, kb1), kn, kg, normals_of(g32), g64, mg)


def test_autograd_input_gradient_with_distinct_weight_exponents(hip):
    from test_gpu_normals import ragged_case
    verts, vend, z, c = ragged_case(K=9, seed=4)
    k = 6                                                           # 2500 vertices
    v = np.asarray(verts[vend[k]:vend[k + 1]], np.float32)
    dec, _, _ = spread_dec(v[None, :2048], z[k:k + 1], c[k:k + 1])
    vi = torch.from_numpy(v).cuda()[None].requires_grad_()
    zz, cc = torch.from_numpy(z[k:k + 1]).cuda(), torch.from_numpy(c[k:k + 1]).cuda()
    dec(vi, zz, cc).sum().backward()
    with torch.no_grad():
        table, fcp = dec.fold(zz, cc)
        _, g = dec.normals(vi.detach()[0].double().contiguous(), [0, vi.shape[1]], table, fcp, return_grad=True)
    hip.device_status()
    assert dec.ka == 6
    assert torch.equal(vi.grad[0], g)


# ------------------------------------------------------------------ chain and head ----
CHAIN_SCALES = {0: (0.15,), 1: (6.0, 0.3), 2: (6.0, 0.3)}


@pytest.mark.parametrize("relu3", [True, False])
@pytest.mark.parametrize("c3", [1024, 256])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_chain_with_distinct_weight_exponents(hip, mode, c3, relu3):
    """chain_pool against tests/test_gpu_chain.py's fp64 composition with sw1 / sw2 / sw3 pairwise distinct (mode 1's
    first layer is not packed: sw2 != sw3 there)"""
    from rfdnet_amd import chain
    from test_gpu_chain import layers, reference
    d = {0: 0, 1: 4, 2: 64}[mode]
    B, P = 2, 1024
    g = torch.Generator(device="cuda").manual_seed(100 + 10 * mode + c3 // 64 + int(relu3))
    l1, l2, l3 = layers(g, d, c3)
    if not relu3:
        l3 = (l3[0], l3[1] - 3.0)
    chain_layers = [l2, l3] if mode == 0 else [l1, l2, l3]
    spread, sw = spread_layers(chain_layers, CHAIN_SCALES[mode], {0: (0, 1), 1: (1, 2), 2: (0, 1, 2)}[mode])
    if mode == 0:
        l1, (l2, l3) = None, spread
    else:
        l1, l2, l3 = spread
    din = d if mode else 64
    x = torch.randn(B * P, din, device="cuda", generator=g) * 1.5
    out = chain.chain_pool(x, l1, l2, l3, P, relu3)
    hip.device_status()
    packed = chain._packed(mode, (l1 or (None, None), l2, l3))
    assert list(packed[1:4])[-len(sw):] == sw                # the kernel is handed the distinct exponents
    ref = reference(x, l1, l2, l3, P, relu3)
    err = (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("mode %d c3 %d relu3 %d sw %s: max |out - fp64| / max(1, |ref|) = %.2e" % (mode, c3, relu3, sw, err))
    assert out.shape == (B, c3)
    assert err < CHAIN_TOL


@pytest.mark.parametrize("n_cls", [1, 2])
def test_head_with_distinct_weight_exponents(hip, n_cls):
    from rfdnet_amd import chain
    B, P = 3, 1024
    g = torch.Generator(device="cuda").manual_seed(70 + n_cls)

    def lin(n, k, scale=2.0):
        return ((torch.rand(n, k, device="cuda", generator=g) * 2 - 1) * scale / np.sqrt(k),
                torch.randn(n, device="cuda", generator=g) * 0.3)
    (Wa, _), lb, lc, ld = lin(512, 64), lin(256, 512), lin(128, 256), lin(n_cls, 128)
    gbias = torch.randn(B, 512, device="cuda", generator=g)
    ((Wa, gbias), lb, lc, (Wd, bd)), sw = spread_layers([(Wa, gbias), lb, lc, ld], (5.0, 0.25, 2.0), (0, 1, 2))
    x = torch.randn(B * P, 64, device="cuda", generator=g) * 1.5
    out = chain.head_scores(x, P, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    assert list(chain._head_packed(Wa, lb[0], lc[0])[1:4]) == sw
    h = torch.relu(x.double() @ Wa.double().t() + gbias.double().repeat_interleave(P, 0))
    h = torch.relu(h @ lb[0].double().t() + lb[1].double())
    h = torch.relu(h @ lc[0].double().t() + lc[1].double())
    ref = h @ Wd.double().t() + bd.double()
    err = (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("head n_cls %d sw %s: max |out - fp64| / max(1, |ref|) = %.2e" % (n_cls, sw, err))
    assert out.shape == (B * P, n_cls) and err < CHAIN_TOL


def test_pointseg_rows_path_with_distinct_weight_exponents(hip, monkeypatch):
    """PointSeg.forward_rows after spread_module (every fused launch's folded weights with distinct exponents): the
    fused chains and head against the layer-by-layer path (RFD_NO_CHAIN=1) and against the module before spreading"""
    from rfdnet_amd.iscnet.pointseg import PointSeg
    seg = PointSeg(2, 4)
    synthetic.load_seeded(seg, 7)
    seg = seg.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(3)
    inp = torch.randn(6, 1024, 4, device="cuda", generator=g)
    with torch.no_grad():
        a0, ta0 = seg.forward_rows(inp)
    hip.device_status()
    exps = spread_module(seg, 5)
    with torch.no_grad():
        a, ta = seg.forward_rows(inp)
        hip.device_status()
        monkeypatch.setenv("RFD_NO_CHAIN", "1")
        b, tb = seg.forward_rows(inp)
    hip.device_status()
    d, dt = (a - b).abs().max().item(), (ta - tb).abs().max().item()
    d0, dt0 = (a - a0).abs().max().item(), (ta - ta0).abs().max().item()
    print("spread %s: log-probabilities max |fused - layerwise| = %.2e, |fused - unspread| = %.2e; feature transform "
          "%.2e, %.2e" % (exps, d, d0, dt, dt0))
    assert d < 1e-4 and dt < 1e-4
    assert d0 < 1e-4 and dt0 < 1e-4
