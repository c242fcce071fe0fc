"""GPU (-m gpu): the fused PointNet feature chains (csrc/pointseg_chain.hip) against an fp64 composition of the same
layers -- [d -> 64, ReLU] -> 64 -> 128, ReLU -> 128 -> 1024 [, ReLU] -> max over each proposal's points
(models/iscnet/modules/pointseg.py:7-42, :45-79, :82-129 with the BatchNorms folded).  fp32-class accuracy is the
contract (the layers it replaces ran on the split-precision GEMM / fp32 library GEMMs)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cases  # noqa: E402
import chain_f64  # noqa: E402

pytestmark = pytest.mark.gpu


def reference(x, l1, l2, l3, P, relu3):
    """the float64 restatement (tests/chain_f64.py), as a tensor beside x"""
    return torch.from_numpy(chain_f64.chain_pool(x, l1, l2, l3, P, relu3)).to(x.device)


def layers(g, d, c3=1024):
    def lin(n, k, scale):
        return ((torch.rand(n, k, device="cuda", generator=g) * 2 - 1) * scale / np.sqrt(k),
                torch.randn(n, device="cuda", generator=g) * 0.3)
    return (lin(64, d, 2.0) if d else None), lin(128, 64, 2.0), lin(c3, 128, 2.0)


@pytest.mark.parametrize("mode,d,relu3,B,P", [(1, 4, True, 3, 1024), (1, 3, True, 2, 512), (1, 7, True, 1, 1024),
                                               (2, 64, True, 3, 1024), (0, 0, False, 5, 1024), (0, 0, True, 2, 1536)])
def test_chain_matches_fp64_composition(hip, mode, d, relu3, B, P):
    from rfdnet_amd import chain
    g = torch.Generator(device="cuda").manual_seed(10 * mode + d)
    l1, l2, l3 = layers(g, d)
    if not relu3:
        l3 = (l3[0], l3[1] - 3.0)                       # negative maxima too: the pool keeps the sign
    din = d if mode else 64
    x = torch.randn(B * P, din, device="cuda", generator=g) * 1.5
    if mode == 1:                                        # a strided view like inp.reshape(B * P, D) of a wider buffer
        wide = torch.zeros(B * P, din + 3, device="cuda")
        wide[:, :din] = x
        x = wide[:, :din]
    assert chain.usable(x, P, din)
    out = chain.chain_pool(x, l1, l2, l3, P, relu3)
    hip.device_status()
    ref = reference(x, l1, l2, l3, P, relu3)
    err = (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("mode %d d %d P %d: max |out - fp64| / max(1, |ref|) = %.2e (|ref| up to %.2f, min %.2f)"
          % (mode, din, P, err, ref.abs().max().item(), ref.min().item()))
    assert out.shape == (B, 1024)
    if not relu3:
        assert (ref < 0).any()
    assert err < 2e-5


@pytest.mark.parametrize("c3,mode,d,relu3,B,P", [(256, 1, 3, True, 5, 1024), (64, 1, 3, True, 2, 512),
                                                  (320, 0, 0, False, 3, 1024), (960, 2, 64, True, 2, 1024)])
def test_chain_with_a_narrower_last_layer(hip, c3, mode, d, relu3, B, P):
    """round 6: the last layer's width is a run-time multiple of 64 (256 = STN_Group's STN3d,
    pointnet2_modules.py:420-466); widths whose piece count does not divide the ring's three slots included"""
    from rfdnet_amd import chain
    g = torch.Generator(device="cuda").manual_seed(c3 + d)
    l1, l2, l3 = layers(g, d, c3)
    if not relu3:
        l3 = (l3[0], l3[1] - 3.0)
    din = d if mode else 64
    x = torch.randn(B * P, din, device="cuda", generator=g) * 1.5
    out = chain.chain_pool(x, l1, l2, l3, P, relu3)
    hip.device_status()
    ref = reference(x, l1, l2, l3, P, relu3)
    assert out.shape == (B, c3)
    assert (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item()) < 2e-5
    with pytest.raises(AssertionError):
        chain.chain_pool(x, l1, l2, (l3[0][:c3 - 4], l3[1][:c3 - 4]), P, relu3)  # not a multiple of 64


def test_stn_group_rows_path_matches_the_module(hip):
    """STN_Group.forward_rows (STN3d's conv chain + max as ONE kernel since round 6) against the module's own
    channel-major forward() -- the reference composition (pointnet2_modules.py:468-537)"""
    from rfdnet_amd import synthetic
    from rfdnet_amd.pointnet2_ops.pointnet2_modules import STN_Group
    stn = STN_Group(radius=1., nsample=1024, use_xyz=False, normalize_xyz=True)
    synthetic.load_seeded(stn, 11)
    stn = stn.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(4)
    xyz = (torch.rand(1, 20000, 3, device="cuda", generator=g) - 0.5) * 4
    feats = torch.randn(1, 2, 20000, device="cuda", generator=g)
    centres = xyz[:, :7].contiguous() + 0.05
    heading = torch.rand(1, 7, device="cuda", generator=g) * 6.28
    with torch.no_grad():
        rows, gf = stn.forward_rows(xyz, feats, centres, heading)            # (7, 1024, 3), (1, 2, 7, 1024)
        ref, gf2 = stn(xyz, feats, centres, heading)                          # (1, 3, 7, 1024)
    hip.device_status()
    assert torch.equal(gf, gf2)
    want = ref[0].permute(1, 2, 0)                                            # (7, 1024, 3)
    err = (rows - want).abs().max().item()
    print("STN_Group rows path vs module: max |d| = %.2e (|x| up to %.2f)" % (err, want.abs().max().item()))
    assert err < 1e-4 * max(1.0, want.abs().max().item())


def test_chain_is_what_the_layerwise_path_computes(hip, monkeypatch):
    """PointSeg.forward_rows with the fused chains against the same module with RFD_NO_CHAIN=1 (one GEMM per layer)."""
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.pointseg import PointSeg
    seg = PointSeg(2, 4)
    synthetic.load_seeded(seg, 7)
    seg = seg.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(3)
    inp = torch.randn(6, 1024, 4, device="cuda", generator=g)
    with torch.no_grad():
        a, ta = seg.forward_rows(inp)
        monkeypatch.setenv("RFD_NO_CHAIN", "1")
        b, tb = seg.forward_rows(inp)
    hip.device_status()
    d = (a - b).abs().max().item()
    dt = (ta - tb).abs().max().item()
    print("log-probabilities: max |fused - layerwise| = %.2e; feature transform: %.2e" % (d, dt))
    assert d < 1e-4 and dt < 1e-4


def test_chain_flags_activations_beyond_the_f16_range(hip):
    from rfdnet_amd import chain
    g = torch.Generator(device="cuda").manual_seed(1)
    l1, l2, l3 = layers(g, 4)
    x = torch.randn(1024, 4, device="cuda", generator=g)
    x[5, 0] = 1.0e5                                      # first-layer output ~1e5: * 2^4 leaves the f16 range
    chain.chain_pool(x, l1, l2, l3, 1024, True)
    with pytest.raises(hip.RfdHipError, match="split-precision GEMM"):
        hip.device_status()


def test_chain_pooled_output_is_range_checked_too(hip):
    """The fused chain's POOLED output feeds a split-precision GEMM directly (_TNet.forward_rows: fc1 on the pooled
    feature): like the GEMM's own pool-only path (tests/test_gpu_gemm.py::test_pool_only_launch_is_range_checked_too)
    it must raise status bit 4 when |pooled| * 2^sa leaves the f16 range although every intermediate stayed inside
    (ADVICE round 3)."""
    from rfdnet_amd import chain
    g = torch.Generator(device="cuda").manual_seed(2)
    l1, l2, l3 = layers(g, 4)
    x = torch.randn(1024, 4, device="cuda", generator=g)
    chain.chain_pool(x, l1, l2, l3, 1024, True)
    hip.device_status()                                  # clean
    w3, b3 = l3
    b3 = b3.clone()
    b3[17] = 5000.0                                      # the last layer's bias alone pushes one pooled channel to ~5000
    out = chain.chain_pool(x, l1, l2, (w3, b3), 1024, True)
    assert float(out[0, 17]) > 4095.0                    # * 2^4 > 65504
    with pytest.raises(hip.RfdHipError, match="split-precision GEMM"):
        hip.device_status()


@pytest.mark.parametrize("B,P,n_cls", [(3, 1024, 2), (2, 384, 2), (4, 1024, 1)])
def test_head_matches_fp64_composition(hip, B, P, n_cls):
    """64 -> 512 (+ per-proposal bias, ReLU) -> 256 (ReLU) -> 128 (ReLU) -> n_cls scores (pointseg.py:131-154 folded)."""
    from rfdnet_amd import chain
    g = torch.Generator(device="cuda").manual_seed(40 + P + n_cls)

    def lin(n, k, scale=2.0):
        return ((torch.rand(n, k, device="cuda", generator=g) * 2 - 1) * scale / np.sqrt(k),
                torch.randn(n, device="cuda", generator=g) * 0.3)
    (Wa, _), lb, lc, (Wd, bd) = lin(512, 64), lin(256, 512), lin(128, 256), lin(n_cls, 128)
    gbias = torch.randn(B, 512, device="cuda", generator=g)
    x = torch.randn(B * P, 64, device="cuda", generator=g) * 1.5
    assert chain.head_usable(x, P, n_cls)
    out = chain.head_scores(x, P, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    h = torch.relu(x.double() @ Wa.double().t() + gbias.double().repeat_interleave(P, 0))
    h = torch.relu(h @ lb[0].double().t() + lb[1].double())
    h = torch.relu(h @ lc[0].double().t() + lc[1].double())
    ref = h @ Wd.double().t() + bd.double()
    err = (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("head B %d P %d k %d: max |out - fp64| / max(1, |ref|) = %.2e (|ref| up to %.2f)" % (B, P, n_cls, err, ref.abs().max().item()))
    assert out.shape == (B * P, n_cls) and err < 2e-5


# =====================================================================================================================
# Every row position against float64 (cases: tests/chain_cases.py; their admissibility: tests/test_chain_cases_cpu.py).
# The tolerance is the one above: max |out - ref| < 2e-5 max(1, max |ref|).

def rel_err(out, ref):
    """max |out - ref| / max(1, max |ref|) of a tensor against a numpy float64 reference"""
    return float(np.abs(out.double().cpu().numpy() - ref).max()) / max(1., float(np.abs(ref).max()))


def rows_that_differ(out, first=8):
    """which rows of `out` are not bit-identical to row 0 (for the failure message)"""
    bad = (out.view(torch.int32) != out.view(torch.int32)[:1]).any(1).nonzero().flatten().tolist()
    return "%d rows differ from row 0 in bits: %s%s" % (len(bad), bad[:first], " ..." if len(bad) > first else "")


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("cfg", cases.EXPOSURE, ids=[cases.config_id(c) for c in cases.EXPOSURE])
def test_every_row_position_decides_the_pool_once(hip, cfg, variant):
    """Exposure batch: B = P proposals, proposal b = one background row everywhere but a hot row at row b, so every
    (wave, pass, group, lane group, accumulator register) of the kernel holds the only possible winner once.
    same: one hot row for all -- every output element is the same dot products whichever position holds the point (the
    MFMA's accumulation order does not depend on it) and max is order-free, so all B output rows are bit-identical.
    distinct: each proposal against its own float64 max; a hot row taken from another proposal shows."""
    from rfdnet_amd import chain
    case = cases.exposure(cfg, variant)
    l1, l2, l3 = cases.to_device(case.layers)
    x = cases.exposure_x(case)
    assert chain.usable(x, case.P, case.d)
    out = chain.chain_pool(x, l1, l2, l3, case.P, case.relu3)
    hip.device_status()
    err = rel_err(out, case.ref)
    print("exposure %s %s: max |out - fp64| / max(1, |ref|) = %.2e (|ref| up to %.2f, min %.2f)"
          % (cases.config_id(cfg), variant, err, np.abs(case.ref).max(), case.ref.min()))
    assert out.shape == (case.P, case.c3)
    if variant == "same":
        assert torch.equal(out, out[:1].expand_as(out)), rows_that_differ(out)
    assert err < 2e-5


@pytest.mark.parametrize("relu3", [False, True])
def test_exact_channels(hip, relu3):
    """A zero row of W3 gives b3 itself (relu3 off) or max(b3, 0) (on), bit for bit and +0.0 where it is zero; a channel
    that no row lifts above zero gives +0.0 under the ReLU."""
    from rfdnet_amd import chain
    case = cases.exact(relu3)
    l1, l2, l3 = cases.to_device(case.layers)
    out = chain.chain_pool(cases.exposure_x(case), l1, l2, l3, case.P, relu3)
    hip.device_status()
    bits = out.cpu().numpy().view(np.int32)
    for ch, b in cases.EXACT_ZERO:
        want = np.float32(max(b, 0.) if relu3 else b)
        assert (bits[:, ch] == want.view(np.int32)).all(), (ch, b, out[:4, ch])
    ch = cases.EXACT_NEGATIVE[0]
    if relu3:
        assert (bits[:, ch] == 0).all(), out[:4, ch]                  # +0.0, not -0.0
    else:
        assert (out[:, ch] < 0).all()
    err = rel_err(out, case.ref)
    print("exact channels, relu3 %d: max |out - fp64| / max(1, |ref|) = %.2e" % (relu3, err))
    assert err < 2e-5


def dense_on_device(args, wide=0):
    c = cases.dense(*args)
    x = torch.from_numpy(c.x).cuda()
    if wide:                                             # a strided view like inp.reshape(B * P, D) of a wider buffer
        buf = torch.full((x.shape[0], c.d + wide), 3.25, device="cuda")
        buf[:, :c.d] = x
        x = buf[:, :c.d]
    return c, x, cases.to_device(c.layers)


def test_pool_does_not_depend_on_the_order_of_rows_or_proposals(hip):
    """dense i.i.d. rows, mode 2, three passes: rows permuted within each proposal -> bit-identical; proposals permuted
    -> output rows permuted; each proposal alone (B = 1) -> its row of the batched call"""
    from rfdnet_amd import chain
    c, x, (l1, l2, l3) = dense_on_device(cases.INVARIANCE)
    out = chain.chain_pool(x, l1, l2, l3, c.P, True)
    moved = chain.chain_pool(cases.permute_rows(x, c.P, c.perm), l1, l2, l3, c.P, True)
    order = torch.from_numpy(c.prop_perm).cuda()
    swapped = chain.chain_pool(x.view(c.B, c.P, c.d)[order].reshape(-1, c.d), l1, l2, l3, c.P, True)
    alone = torch.cat([chain.chain_pool(x[b * c.P:(b + 1) * c.P], l1, l2, l3, c.P, True) for b in range(c.B)])
    hip.device_status()
    err = rel_err(out, chain_f64.chain_pool(c.x, *c.layers, c.P, True))
    print("dense mode 2 P %d: max |out - fp64| / max(1, |ref|) = %.2e" % (c.P, err))
    assert err < 2e-5
    assert torch.equal(moved, out)
    assert torch.equal(swapped, out[order])
    assert torch.equal(alone, out)


def test_pool_does_not_depend_on_the_order_of_rows_strided_mode_1(hip):
    from rfdnet_amd import chain
    c, x, (l1, l2, l3) = dense_on_device(cases.INVARIANCE_MODE1, wide=3)
    assert x.stride(0) == c.d + 3 and chain.usable(x, c.P, c.d)
    out = chain.chain_pool(x, l1, l2, l3, c.P, True)
    moved_rows = cases.permute_rows(x, c.P, c.perm)
    wide = torch.full((x.shape[0], c.d + 3), -3.25, device="cuda")
    wide[:, :c.d] = moved_rows
    moved = chain.chain_pool(wide[:, :c.d], l1, l2, l3, c.P, True)
    hip.device_status()
    err = rel_err(out, chain_f64.chain_pool(c.x, *c.layers, c.P, True))
    print("dense mode 1 P %d, strided: max |out - fp64| / max(1, |ref|) = %.2e" % (c.P, err))
    assert err < 2e-5 and torch.equal(moved, out)


@pytest.mark.parametrize("ldx", cases.LDX)
@pytest.mark.parametrize("args", cases.STRIDE, ids=["mode0", "mode2"])
def test_chain_reads_a_column_slice_of_a_wider_buffer(hip, args, ldx):
    """modes 0 and 2 on rows ldx floats apart, the base 16 bytes behind the allocation: bit-identical to the contiguous
    copy; rows that are not 16-byte aligned are not usable"""
    from rfdnet_amd import chain
    c, x, (l1, l2, l3) = dense_on_device(args)
    view = cases.strided(x, ldx)
    assert view.stride(0) == ldx and view.data_ptr() % 16 == 0 and view.storage_offset() == 4
    assert chain.usable(view, c.P, c.d)
    out = chain.chain_pool(x, l1, l2, l3, c.P, True)
    strided = chain.chain_pool(view, l1, l2, l3, c.P, True)
    hip.device_status()
    err = rel_err(out, chain_f64.chain_pool(c.x, *c.layers, c.P, True))
    print("mode %d ldx %d: max |out - fp64| / max(1, |ref|) = %.2e" % (c.mode, ldx, err))
    assert err < 2e-5 and torch.equal(strided, out)
    for bad in (cases.strided(x, 66), cases.strided(x, ldx, shift=1)):
        assert torch.equal(bad, x) and not chain.usable(bad, c.P, c.d)
        with pytest.raises(AssertionError):
            chain.chain_pool(bad, l1, l2, l3, c.P, True)


def head_on_device(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    return t(c.Wa), (t(c.lb[0]), t(c.lb[1])), (t(c.lc[0]), t(c.lc[1])), t(c.Wd), t(c.bd)


@pytest.mark.parametrize("ldx", cases.LDX)
def test_head_reads_a_column_slice_of_a_wider_buffer(hip, ldx):
    from rfdnet_amd import chain
    c = cases.head(128)
    Wa, lb, lc, Wd, bd = head_on_device(c)
    B = 5
    x, gbias = torch.from_numpy(c.x[:B * c.P]).cuda(), torch.from_numpy(c.gbias[:B]).cuda()
    view = cases.strided(x, ldx)
    assert chain.head_usable(view, c.P, 2)
    out = chain.head_scores(x, c.P, Wa, gbias, lb, lc, Wd, bd)
    strided = chain.head_scores(view, c.P, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    err = rel_err(out, chain_f64.head_scores(c.x[:B * c.P], c.P, c.Wa, c.gbias[:B], c.lb, c.lc, c.Wd, c.bd))
    print("head ldx %d: max |out - fp64| / max(1, |ref|) = %.2e" % (ldx, err))
    assert err < 2e-5 and torch.equal(strided, out)
    for bad in (cases.strided(x, 66), cases.strided(x, ldx, shift=1)):
        assert torch.equal(bad, x) and not chain.head_usable(bad, c.P, 2)
        with pytest.raises(AssertionError):
            chain.head_scores(bad, c.P, Wa, gbias, lb, lc, Wd, bd)


@pytest.mark.parametrize("shared_gbias", [True, False], ids=["one-gbias", "gbias-per-proposal"])
@pytest.mark.parametrize("P", cases.HEAD_P)
def test_head_scores_one_row_at_every_position(hip, P, shared_gbias):
    """300 proposals (more than CUs) of one x row at every row position: the scores are bit-constant within a proposal
    -- over all M rows when every proposal has the same gbias -- and each proposal matches its own float64 value
    (consecutive proposals differ decisively: tests/test_chain_cases_cpu.py)"""
    from rfdnet_amd import chain
    c = cases.head(P)
    Wa, lb, lc, Wd, bd = head_on_device(c)
    x = torch.from_numpy(c.row).cuda().expand(c.B * P, 64).contiguous()
    gbias = torch.from_numpy(c.gbias).cuda()
    if shared_gbias:
        gbias = gbias[:1].expand(c.B, 512).contiguous()
    out = chain.head_scores(x, P, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    ref = cases.head_one_row_ref(P, shared_gbias)
    per_proposal = out.view(c.B, P, 2)
    err = rel_err(per_proposal[:, 0], ref)
    print("head, one row everywhere, P %d, %s: max |out - fp64| / max(1, |ref|) = %.2e (|ref| up to %.2f)"
          % (P, "one gbias" if shared_gbias else "gbias per proposal", err, np.abs(ref).max()))
    assert torch.equal(per_proposal, per_proposal[:, :1].expand_as(per_proposal)), \
        rows_that_differ(per_proposal.reshape(c.B, -1).t())
    if shared_gbias:
        assert torch.equal(out, out[:1].expand_as(out)), rows_that_differ(out)
    assert err < 2e-5


@pytest.mark.parametrize("n_cls", [1, 2])
@pytest.mark.parametrize("P", cases.HEAD_P)
def test_head_scores_do_not_depend_on_the_row_position(hip, P, n_cls):
    """300 proposals of distinct rows against float64, and again with the rows of every proposal permuted: a row's
    score is bit-identical wherever in its proposal the row sits"""
    from rfdnet_amd import chain
    c = cases.head(P, n_cls)
    Wa, lb, lc, Wd, bd = head_on_device(c)
    x, gbias = torch.from_numpy(c.x).cuda(), torch.from_numpy(c.gbias).cuda()
    assert chain.head_usable(x, P, n_cls)
    out = chain.head_scores(x, P, Wa, gbias, lb, lc, Wd, bd)
    moved = chain.head_scores(cases.permute_rows(x, P, c.perm), P, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    ref = cases.head_hidden_ref(P) @ chain_f64.f64(c.Wd).T + chain_f64.f64(c.bd)
    err = rel_err(out, ref)
    print("head B %d P %d k %d: max |out - fp64| / max(1, |ref|) = %.2e (|ref| up to %.2f)"
          % (c.B, P, n_cls, err, np.abs(ref).max()))
    assert out.shape == (c.B * P, n_cls) and err < 2e-5
    assert torch.equal(moved, cases.permute_rows(out, P, c.perm))


SENTINEL = -7.0


def test_refusals(hip):
    """What the entries cannot run is refused with hipErrorInvalidValue before anything is launched: the outputs keep
    their sentinel and the status word stays clean.  M = 0 is valid and does nothing; a valid call still works after."""
    from rfdnet_amd import _lib, chain, gemm
    dev = torch.device("cuda")
    c, x, (l1, l2, l3) = dense_on_device(cases.STRIDE[1])                       # mode 2, P = 512, c3 = 256
    M, P, c3 = x.shape[0], c.P, c.c3
    x8 = torch.zeros(M, 8, device=dev)
    w1raw = torch.zeros(64, 8, device=dev)
    packed = torch.full((_lib.lib().rfd_chain_packed_bytes_n(c3),), 0x5a, dtype=torch.uint8, device=dev)
    out = torch.full((M // P, 1024), SENTINEL, device=dev)
    p = lambda t: t.data_ptr()                                                  # noqa: E731
    hip.device_status()

    def pool(mode=0, c3=c3, M=M, P=P, d_in=64, x=p(x), ldx=64, W1raw=None, b1=p(l1[1]), b2=p(l2[1]), b3=p(l3[1]),
             out=p(out)):
        _lib.call("rfd_chain_pool_n", dev, mode, c3, M, P, d_in, x, ldx, p(packed), W1raw, b1, b2, b3, 1, gemm.SA, 0, 0,
                  0, out)
    mode1 = dict(mode=1, x=p(x8), ldx=8, W1raw=p(w1raw))
    for bad in (dict(P=256), dict(P=0), dict(M=3 * P, P=2 * P), dict(mode=3), dict(mode=-1),
                dict(mode1, d_in=0), dict(mode1, d_in=9), dict(mode1, d_in=3, W1raw=None),
                dict(d_in=3), dict(ldx=66), dict(x=p(x) + 4), dict(mode=2, b1=None), dict(b2=None), dict(b3=None),
                dict(out=None), dict(c3=0), dict(c3=96), dict(c3=1088)):
        with pytest.raises(_lib.RfdHipError, match=r"rfd_chain_pool_n failed \(hipError 1\)"):      # hipErrorInvalidValue
            pool(**bad)

    Wa, lb, lc, Wd, bd = head_on_device(cases.head(128))
    gbias = torch.zeros(M // 128, 512, device=dev)
    hpacked = torch.zeros(_lib.lib().rfd_head_packed_bytes(), dtype=torch.uint8, device=dev)
    scores = torch.full((M, 2), SENTINEL, device=dev)

    def head(M=M, P=128, x=p(x), ldx=64, gbias=p(gbias), bb=p(lb[1]), bc=p(lc[1]), Wd=p(Wd), bd=p(bd), n_cls=2,
             out=p(scores)):
        _lib.call("rfd_head_scores", dev, M, P, x, ldx, p(hpacked), gbias, bb, bc, Wd, bd, n_cls, gemm.SA, 0, 0, 0, out)
    for bad in (dict(P=64), dict(M=M - 128, P=256), dict(ldx=66), dict(x=p(x) + 4), dict(n_cls=0), dict(n_cls=3),
                dict(gbias=None), dict(bb=None), dict(bc=None), dict(Wd=None), dict(bd=None), dict(out=None)):
        with pytest.raises(_lib.RfdHipError, match=r"rfd_head_scores failed \(hipError 1\)"):
            head(**bad)

    def pack(mode=2, c3=c3, W1=p(l1[0]), W2=p(l2[0]), W3=p(l3[0])):
        _lib.call("rfd_chain_pack_n", dev, mode, c3, W1, W2, W3, 0, 0, 0, p(packed))
    for bad in (dict(mode=3), dict(W1=None), dict(W2=None), dict(W3=None), dict(c3=96)):
        with pytest.raises(_lib.RfdHipError, match=r"rfd_chain_pack_n failed \(hipError 1\)"):
            pack(**bad)
    assert _lib.lib().rfd_chain_packed_bytes_n(96) == 0 and _lib.lib().rfd_chain_packed_bytes_n(0) == 0
    assert _lib.lib().rfd_chain_packed_bytes_n(1088) == 0 and _lib.lib().rfd_chain_packed_bytes_n(c3) == packed.numel()

    pool(M=0)                                                                    # nothing to do: success, nothing written
    head(M=0)
    hip.device_status()                                                          # synchronises; no flag was raised
    assert (out == SENTINEL).all() and (scores == SENTINEL).all() and (packed == 0x5a).all()
    got = chain.chain_pool(x, l1, l2, l3, P, True)                               # and the entries still work
    got_scores = chain.head_scores(x, 128, Wa, gbias, lb, lc, Wd, bd)
    hip.device_status()
    assert rel_err(got, chain_f64.chain_pool(c.x, *c.layers, P, True)) < 2e-5
    h = cases.head(128)
    assert rel_err(got_scores, chain_f64.head_scores(c.x, 128, h.Wa, gbias, h.lb, h.lc, h.Wd, h.bd)) < 2e-5
