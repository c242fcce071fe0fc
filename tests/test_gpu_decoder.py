"""GPU (-m gpu): fused occupancy decoder vs the oracle / reference fixture.
Tolerance: 1e-4 absolute on logits (BASELINE.json north_star)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from seeded import seeded_decoder

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-4


@pytest.fixture(autouse=True)
def main_kernel_only(request, hip):
    """The kernel-level tests of this module are about occ_decode8_kernel: launches of any size stay on it.  Tests marked
    `tail` choose the launch route themselves; the pipeline tests of the other modules run with the shipped default
    (small launches on csrc/occ_decoder_tail.hip)."""
    if request.node.get_closest_marker("tail"):
        yield
        return
    old = hip.lib().rfd_occ_set_tail_tiles(0)
    try:
        yield
    finally:
        hip.lib().rfd_occ_set_tail_tiles(old)


def test_decoder_matches_reference_fixture(hip, golden_dir):
    """F-DEC: logits of the reference DecoderCBatchNorm (torch CPU fp32)."""
    fx = np.load(os.path.join(golden_dir, "F_DEC.npz"))
    dec = seeded_decoder(int(fx["seed"]))
    with torch.no_grad():
        out = dec(torch.from_numpy(fx["p"]).cuda(), torch.from_numpy(fx["z"]).cuda(),
                  torch.from_numpy(fx["c"]).cuda())
    hip.device_status()
    err = np.abs(out.cpu().numpy() - fx["logits"]).max()
    assert err < LOGIT_TOL, err
    assert err < 2e-5, err            # the parity mode is fp32-class, not just in tolerance


def test_decoder_matches_oracle_ragged(hip, oracle):
    """T not a multiple of the 128-point tile, several proposals, non-zero z"""
    dec = seeded_decoder(99)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in dec.state_dict().items())
    blob = oracle.decoder_param_blob(sd)
    rng = np.random.default_rng(5)
    K, T = 5, 333
    p = ((rng.random((K, T, 3)) - 0.5) * 1.1).astype(np.float32)
    z = rng.normal(0, 1, (K, 32)).astype(np.float32)
    c = rng.normal(0, 1, (K, 512)).astype(np.float32)
    ref = oracle.decoder_cbn(blob, p, z, c)
    with torch.no_grad():
        out = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
    hip.device_status()
    assert np.abs(out.cpu().numpy() - ref).max() < LOGIT_TOL


def test_decoder_throughput_mode_error_is_reported_not_hidden(hip, golden_dir):
    from rfdnet_amd.iscnet import occ_decoder
    fx = np.load(os.path.join(golden_dir, "F_DEC.npz"))
    dec = seeded_decoder(int(fx["seed"]))
    dec.mode = occ_decoder.MODE_F16X1
    with torch.no_grad():
        out = dec(torch.from_numpy(fx["p"]).cuda(), torch.from_numpy(fx["z"]).cuda(),
                  torch.from_numpy(fx["c"]).cuda())
    err = np.abs(out.cpu().numpy() - fx["logits"]).max()
    assert err < 5e-3, err           # f16x1 is NOT the parity mode
    sign = ((out.cpu().numpy() > 0) == (fx["logits"] > 0)).mean()
    assert sign > 0.995


def test_decoder_point_independence(hip):
    """a point's logit must not depend on its tile neighbours / position"""
    dec = seeded_decoder(7)
    rng = np.random.default_rng(1)
    p = ((rng.random((1, 512, 3)) - 0.5)).astype(np.float32)
    z = np.zeros((1, 32), np.float32)
    c = rng.normal(0, 1, (1, 512)).astype(np.float32)
    with torch.no_grad():
        a = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
        perm = rng.permutation(512)
        b = dec(torch.from_numpy(p[:, perm]).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
    np.testing.assert_array_equal(a.cpu().numpy()[0][perm], b.cpu().numpy()[0])


def test_decoder_f16_overflow_falls_back_to_a_smaller_scale(hip, oracle):
    """The reference's fp32 decoder cannot overflow (occ_decoder.py:110-123).  Here activations are scaled by 2^6
    before the f16 split: |a| >= 1023.5 raises status bit 2 -- and the module answers with ONE re-run at scale 2^3
    (|a| < 8190), not with an exception; the logits must still match the oracle.  Only an overflow at the fallback
    scale raises."""
    for kern in ("w8", "w4"):
        dec = seeded_decoder(7)
        dec.kernel = kern
        with torch.no_grad():
            dec.blocks[0].bn_0.conv_beta.bias.fill_(1500.0)      # activations up to ~4800: * 2^6 > f16 max, * 2^3 fits
        rng = np.random.default_rng(2)
        p = ((rng.random((2, 256, 3)) - 0.5) * 1.1).astype(np.float32)
        z = np.zeros((2, 32), np.float32)
        c = rng.normal(0, 1, (2, 512)).astype(np.float32)
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="f16 range"):
            out = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
        assert dec.ka == 3
        hip.device_status()                                       # nothing left flagged
        sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in dec.state_dict().items())
        ref = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
        err = np.abs(out.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
        print("%s: fallback scale 2^3, max |dlogit| / max(1, |logit|) = %.2e (|logit| up to %.3g)" % (kern, err, np.abs(ref).max()))
        assert err < 1e-4
        with torch.no_grad():                                     # the scale stays lowered: no second warning, same result
            again = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
        assert torch.equal(out, again)
        with torch.no_grad():
            dec.blocks[0].bn_0.conv_beta.bias.fill_(5000.0)      # activations up to ~16000 > 8190: beyond the fallback
                                                                  # scale too -- a real error
            with pytest.raises(hip.RfdHipError, match="f16 range"):
                dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
        hip.device_status()


def test_eight_wave_kernel_gives_the_same_logits(hip, golden_dir, oracle):
    """csrc/occ_decoder8.hip (two waves per SIMD, 16x16x32 MFMA): same arithmetic, other
    fragment order -- fixture parity, oracle parity on ragged tiles, and agreement with the
    four-wave kernel to the last few ulps."""
    fx = np.load(os.path.join(golden_dir, "F_DEC.npz"))
    d4 = seeded_decoder(int(fx["seed"]))
    d8 = seeded_decoder(int(fx["seed"]))
    d8.kernel = "w8"
    p, z, c = (torch.from_numpy(fx[k]).cuda() for k in ("p", "z", "c"))
    with torch.no_grad():
        o4, o8 = d4(p, z, c), d8(p, z, c)
    hip.device_status()
    assert np.abs(o8.cpu().numpy() - fx["logits"]).max() < 2e-5
    assert (o8 - o4).abs().max().item() < 2e-6
    rng = np.random.default_rng(8)
    K, T = 3, 517
    pp = ((rng.random((K, T, 3)) - 0.5) * 1.1).astype(np.float32)
    zz = rng.normal(0, 1, (K, 32)).astype(np.float32)
    cc = rng.normal(0, 1, (K, 512)).astype(np.float32)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in d8.state_dict().items())
    ref = oracle.decoder_cbn(oracle.decoder_param_blob(sd), pp, zz, cc)
    with torch.no_grad():
        out = d8(torch.from_numpy(pp).cuda(), torch.from_numpy(zz).cuda(), torch.from_numpy(cc).cuda())
    assert np.abs(out.cpu().numpy() - ref).max() < LOGIT_TOL


def test_decoder_stress_config_full_size(hip, oracle):
    """BASELINE configs[2] at full size: 256 proposals x 262 144 uniform query points (67.1 M), codes ~ N(0,1).
    Size-independent checks: (i) a point's logit does not depend on where it sits -- permuting the
    points of every proposal permutes the logits bit for bit; (ii) 1000 sampled points against the
    CPU oracle decoder (module semantics, occ_decoder.py:110-123) within 1e-4; (iii) no device
    status bit (f16 range) is raised."""
    K, T = 256, 262144
    dec = seeded_decoder(3)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in dec.state_dict().items())
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    p = (torch.rand(K, T, 3, device="cuda", generator=g) - 0.5) * 1.1
    c = torch.randn(K, 512, device="cuda", generator=g)
    z = torch.zeros(K, 32, device="cuda")
    with torch.no_grad():
        out = dec(p, z, c)
        hip.device_status()
        assert out.shape == (K, T) and torch.isfinite(out).all()
        perm = torch.randperm(T, device="cuda", generator=g)
        out_p = dec(p[:, perm].contiguous(), z, c)
        hip.device_status()
    assert torch.equal(out[:, perm], out_p)
    rng = np.random.default_rng(11)
    kk = rng.integers(0, K, 1000)
    tt = rng.integers(0, T, 1000)
    order = np.argsort(kk, kind="stable")
    kk, tt = kk[order], tt[order]
    blob = oracle.decoder_param_blob(sd)
    worst = 0.0
    p_h, c_h, o_h = p[kk, tt].cpu().numpy(), c.cpu().numpy(), out[kk, tt].cpu().numpy()
    for k in np.unique(kk):
        m = kk == k
        ref = oracle.decoder_cbn(blob, p_h[m][None], np.zeros((1, 32), np.float32), c_h[k][None])
        worst = max(worst, float(np.abs(ref[0] - o_h[m]).max()))
    print("stress config: max |dlogit| on the 1000-point oracle sample = %.2e" % worst)
    assert worst < LOGIT_TOL


# ------------------------------------------------------------------ chunk claiming (round 4) ----
def _ragged_launch(dec, K=37, seed=3, skip_every=0):
    """a multi-proposal ragged launch big enough for several chunks per workgroup"""
    rng = np.random.default_rng(seed)
    tiles = rng.integers(1, 90, K)
    tile_prop = np.repeat(np.arange(K, dtype=np.int32), tiles)
    if skip_every:
        tile_prop[::skip_every] = -1                       # tiles the kernel must skip (tile_prop < 0)
    n_tiles = tile_prop.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    pts = ((torch.rand(n_tiles * 128, 3, device="cuda", generator=g) - 0.5) * 1.1).contiguous()
    c = torch.randn(K, 512, device="cuda", generator=g)
    z = torch.zeros(K, 32, device="cuda")
    with torch.no_grad():
        table, fcp = dec.fold(z, c)
    return pts, torch.from_numpy(tile_prop).cuda(), table, fcp


def test_claimed_chunks_and_static_partition_give_identical_logits(hip):
    """The eight-wave kernel hands its tiles out at run time (chunk_range, csrc/occ_decoder8.hip); who computes a tile
    must not matter: bit-identical to rounds 1-3's static partition (rfd_occ_set_launch_shape), run after run, with skipped
    tiles, through the fused MISE scatter, one workgroup per chunk, and on a reduced grid.  The counter pair of a
    launch (its stream's own, or -- on the null stream -- one of the shared pool) is reset by the kernel itself: 1100
    launches in a row, on a stream of its own and on the null stream, then the comparison again."""
    dec = seeded_decoder(11)
    assert dec.kernel == "w8"
    for skip in (0, 7):
        pts, tile_prop, table, fcp = _ragged_launch(dec, skip_every=skip)
        keep = (tile_prop >= 0).repeat_interleave(128)
        with torch.no_grad():
            lib = hip.lib()
            lib.rfd_occ_set_launch_shape(1, -1, -1)
            try:
                ref = dec.decode_tiles(pts, tile_prop, table, fcp)
            finally:
                lib.rfd_occ_set_launch_shape(0, -1, -1)
            runs = [dec.decode_tiles(pts, tile_prop, table, fcp) for _ in range(3)]
            for cap in (0, 1, 5, 16, 255):       # persistent + claiming / one workgroup per chunk of <= cap tiles
                lib.rfd_occ_set_launch_shape(-1, -1, cap)
                try:
                    runs.append(dec.decode_tiles(pts, tile_prop, table, fcp))
                finally:
                    lib.rfd_occ_set_launch_shape(-1, -1, 0)
            for cus in (200, 37):                # a reduced persistent grid
                lib.rfd_occ_set_launch_shape(-1, cus, -1)
                try:
                    runs.append(dec.decode_tiles(pts, tile_prop, table, fcp))
                finally:
                    lib.rfd_occ_set_launch_shape(-1, 0, -1)
        hip.device_status()
        for r in runs:
            assert torch.equal(r[keep], ref[keep])
    # the shared pool of counter pairs (null stream: 960 slots) wraps, a stream's own pair is used 1100 times in a
    # row: every pair must come back zeroed
    small = tile_prop[:3].contiguous()
    with torch.no_grad():
        for _ in range(1100):
            dec.decode_tiles(pts[:3 * 128], small, table, fcp)
        again = dec.decode_tiles(pts, tile_prop, table, fcp)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(1100):
                dec.decode_tiles(pts[:3 * 128], small, table, fcp)
            again2 = dec.decode_tiles(pts, tile_prop, table, fcp)
        side.synchronize()
    hip.device_status()
    assert torch.equal(again[keep], ref[keep])
    assert torch.equal(again2[keep], ref[keep])


def test_claimed_chunks_through_the_fused_scatter(hip):
    dec = seeded_decoder(12)
    pts, tile_prop, table, fcp = _ragged_launch(dec, K=9, seed=5)
    n = pts.shape[0]
    K = int(tile_prop.max().item()) + 1
    # a permutation inside each proposal's own slot range as the lattice index; one padding slot per tile
    lin = torch.arange(n, dtype=torch.int32, device="cuda")
    first = torch.zeros(K, dtype=torch.long, device="cuda")
    tp = tile_prop.long()
    starts = torch.cat([torch.zeros(1, dtype=torch.long, device="cuda"), torch.bincount(tp, minlength=K).cumsum(0)[:-1]]) * 128
    lin = (lin.long() - starts[tp.repeat_interleave(128)]).int()
    lin[::128] = -1
    n_per = int(torch.bincount(tp, minlength=K).max().item()) * 128
    outs = []
    for static in (True, False):
        values = torch.full((K, n_per), float("nan"), device="cuda")
        pstate = torch.ones(K, n_per, dtype=torch.uint8, device="cuda")
        hip.lib().rfd_occ_set_launch_shape(int(static), -1, -1)
        try:
            with torch.no_grad():
                dec.decode_tiles(pts, tile_prop, table, fcp, scatter=(lin, values, pstate))
        finally:
            hip.lib().rfd_occ_set_launch_shape(0, -1, -1)
        hip.device_status()
        outs.append((values, pstate))
    assert torch.equal(outs[0][1], outs[1][1])
    known = outs[0][1] == 2
    assert int(known.sum()) == n - n // 128
    assert torch.equal(outs[0][0][known], outs[1][0][known])
    with torch.no_grad():
        plain = dec.decode_tiles(pts, tile_prop, table, fcp)
    ok = lin >= 0
    got = outs[1][0][tp.repeat_interleave(128)[ok], lin[ok].long()]
    assert torch.equal(got, plain[ok])


# ------------------------------------------------------------------ tail launches (round 6) ----
@pytest.mark.tail
@pytest.mark.parametrize("mode", ["x3", "x1"])
def test_tail_kernel_is_bit_identical_to_the_main_kernel(hip, mode):
    """csrc/occ_decoder_tail.hip (one wave per 16 points, no LDS, weights straight from L2) runs every accumulator through the
    same sequence of matrix instructions as occ_decode8_kernel: identical logits, plain and through the fused MISE scatter,
    with skipped tiles, with 16-slot groups that are all padding (skipped by the tail kernel, computed and dropped by the main
    one), in both arithmetic modes; the f16-range flag is raised by both."""
    from rfdnet_amd.iscnet import occ_decoder
    lib = hip.lib()
    dec = seeded_decoder(21)
    if mode == "x1":
        dec.mode = occ_decoder.MODE_F16X1
    default = lib.rfd_occ_set_tail_tiles(-1)
    assert default == 384
    for K, skip in ((9, 0), (37, 5)):
        pts, tile_prop, table, fcp = _ragged_launch(dec, K=K, seed=7 + K, skip_every=skip)
        n_tiles = tile_prop.shape[0]
        keep = (tile_prop >= 0).repeat_interleave(128)
        try:
            with torch.no_grad():
                lib.rfd_occ_set_tail_tiles(0)
                ref = dec.decode_tiles(pts, tile_prop, table, fcp)
                lib.rfd_occ_set_tail_tiles(n_tiles)
                got = dec.decode_tiles(pts, tile_prop, table, fcp)
                lib.rfd_occ_set_tail_tiles(n_tiles - 1)           # one tile too many for the tail route: main kernel again
                again = dec.decode_tiles(pts, tile_prop, table, fcp)
        finally:
            lib.rfd_occ_set_tail_tiles(default)
        hip.device_status()
        assert torch.equal(got[keep], ref[keep])
        assert torch.equal(again[keep], ref[keep])
        # through the scatter: most slots padding, whole 16-slot groups of padding, a few real points per tile
        n = pts.shape[0]
        tp_h = tile_prop.cpu().numpy()
        rank = np.zeros(n_tiles, dtype=np.int64)                 # a tile's position among its proposal's (unskipped) tiles
        seen = {}
        for t, p_ in enumerate(tp_h):
            if p_ >= 0:
                rank[t] = seen.get(int(p_), 0)
                seen[int(p_)] = rank[t] + 1
        n_per = 128 * max(seen.values())
        tp = tile_prop.long().clamp(min=0)
        g = torch.Generator(device="cuda").manual_seed(3)
        real = torch.rand(n, device="cuda", generator=g) < 0.12
        real &= ((torch.arange(n, device="cuda") // 16) % 3 != 1)          # every third group has no real slot at all
        real &= keep
        lin = (torch.from_numpy(rank).cuda().repeat_interleave(128) * 128 + torch.arange(n, device="cuda") % 128).int()
        lin[~real] = -1
        outs = []
        for tail in (0, n_tiles):
            values = torch.full((K, n_per), float("nan"), device="cuda")
            pstate = torch.ones(K, n_per, dtype=torch.uint8, device="cuda")
            lib.rfd_occ_set_tail_tiles(tail)
            try:
                with torch.no_grad():
                    dec.decode_tiles(pts, tile_prop, table, fcp, scatter=(lin, values, pstate))
            finally:
                lib.rfd_occ_set_tail_tiles(default)
            hip.device_status()
            outs.append((values, pstate))
        assert torch.equal(outs[0][1], outs[1][1])
        known = outs[0][1] == 2
        assert int(known.sum()) == int(real.sum()) > 0
        assert torch.equal(outs[0][0][known], outs[1][0][known])
        assert torch.equal(outs[1][0][tp.repeat_interleave(128)[real], lin[real].long()], ref[real])


@pytest.mark.tail
def test_tail_kernel_against_the_reference_fixture_and_range_flag(hip, golden_dir):
    """F-DEC through the tail route (the fixture's launch is far below the default threshold), and the f16-range flag: the
    tail kernel raises status bit 2 where the main kernel does (a table scaled out of the f16 range)."""
    lib = hip.lib()
    assert lib.rfd_occ_set_tail_tiles(-1) == 384
    fx = np.load(os.path.join(golden_dir, "F_DEC.npz"))
    dec = seeded_decoder(int(fx["seed"]))
    with torch.no_grad():
        out = dec(torch.from_numpy(fx["p"]).cuda(), torch.from_numpy(fx["z"]).cuda(),
                  torch.from_numpy(fx["c"]).cuda())
    hip.device_status()
    assert np.abs(out.cpu().numpy() - fx["logits"]).max() < 2e-5
    pts, tile_prop, table, fcp = _ragged_launch(dec, K=3, seed=2)
    flags = []
    for tail in (0, 384):
        lib.rfd_occ_set_tail_tiles(tail)
        try:
            with torch.no_grad():
                dec.decode_tiles(pts, tile_prop, (table * 4096.0).contiguous(), fcp)
            torch.cuda.synchronize()
            flags.append(hip.stream_status_bits())
        finally:
            lib.rfd_occ_set_tail_tiles(384)
    assert flags[0] == flags[1] and flags[0] & 2, flags


@pytest.mark.tail
def test_tail_kernel_beside_other_matrix_kernels(hip):
    """The tail kernel's waves share SIMDs with whatever else runs (that is its point).  Beside a stream of library GEMMs
    (MFMA kernels of a few workgroups: partner waves on the same SIMDs) and of elementwise passes its logits stay
    bit-identical to the main kernel's, launch after launch -- the situation in which the first build, with hipcc's packed
    fp32 op_sel forms in its prologue, went wrong (profiles/r06_pk_f32_hazard.txt)."""
    lib = hip.lib()
    dec = seeded_decoder(31)
    pts, tile_prop, table, fcp = _ragged_launch(dec, K=9, seed=21)
    n_tiles = tile_prop.shape[0]
    default = lib.rfd_occ_set_tail_tiles(-1)
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(192, 1024, device="cuda", generator=g)
    b = torch.randn(1024, 256, device="cuda", generator=g)
    big = torch.empty(8 << 20, device="cuda")
    side = torch.cuda.Stream()
    try:
        with torch.no_grad():
            lib.rfd_occ_set_tail_tiles(0)
            ref = dec.decode_tiles(pts, tile_prop, table, fcp)
            torch.cuda.synchronize()
            lib.rfd_occ_set_tail_tiles(n_tiles)
            bad = 0
            for it in range(25):
                with torch.cuda.stream(side):
                    for _ in range(40):                      # ~1 ms of small MFMA kernels and HBM passes beside the launch
                        torch.mm(a, b)
                        big.mul_(1.0001)
                got = dec.decode_tiles(pts, tile_prop, table, fcp)
                torch.cuda.synchronize()
                bad += int((got != ref).sum())
    finally:
        lib.rfd_occ_set_tail_tiles(default)
    hip.device_status()
    assert bad == 0, bad


# ------------------------------------------------------------------ logit bands (round 4) ----
BANDS = [  # (name, conditioning scale, fc_out scale, absolute tolerance or None)
    ("+-3 (fc_out x4)", 1.0, 4.0, LOGIT_TOL),
    ("+-3 (codes x3.5)", 3.5, 1.0, LOGIT_TOL),
    ("+-10 (codes x5)", 5.0, 1.0, LOGIT_TOL),
    ("+-30 (codes x5.6)", 5.6, 1.0, LOGIT_TOL),
    ("+-50 (codes x6)", 6.0, 1.0, None),       # beyond the band a checkpoint lives in: relative bound only
]


def _band_case(cs, fs, seed=1234, K=4, T=2048):
    dec = seeded_decoder(seed)
    with torch.no_grad():
        dec.fc_out.weight.mul_(fs)
        dec.fc_out.bias.mul_(fs)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in dec.state_dict().items())
    rng = np.random.default_rng(0)
    p = ((rng.random((K, T, 3)) - 0.5) * 1.1).astype(np.float32)
    z = np.zeros((K, 32), np.float32)
    c = (rng.normal(0, 1, (K, 512)) * cs).astype(np.float32)
    return dec, sd, p, z, c


def test_decoder_logit_bands_where_a_trained_checkpoint_lives(hip, oracle):
    """The reference decoder is fp32 (occ_decoder.py:110-123): its error does not grow with |logit|, the split-f16
    scheme's could.  Bands of |logit| up to 3 / 10 / 30 / 50 are produced by scaling the conditioning codes (larger CBN
    gammas and betas -> larger activations through all five blocks), one by scaling fc_out.  Ground truth = the module
    restated in float64 (tests/dec_f64.py); the fp32 oracle (module semantics, k-ascending sums) is measured against
    it too, because at |logit| ~ 30 one fp32 evaluation of the module is itself 1.4e-4 from the exact value (measured
    in the build container) -- so |HIP - oracle| <= 1e-4 cannot hold there for ANY implementation, the reference on
    another BLAS included.  Asserted per band and kernel:  |HIP - exact| <= 1e-4 up to the +-30 band (measured on MI355X
    at +-50: 1.55e-4 for the kernel, 1.94e-4 for the fp32 oracle -- there only the relative bound 4e-6 of max |logit|
    is asserted);  |HIP - oracle| <= 1e-4 + the oracle's own distance from exact;  HIP at least as close to exact as
    the fp32 evaluation (x1.25 + 2e-6 slack) -- i.e. fp32-class in every band."""
    from dec_f64 import decoder_f64
    lines = ["band                 kernel  |logit|max  act max   |HIP-f64|   |oracle32-f64|  |HIP-oracle32|"]
    failures = []
    for name, cs, fs, tol in BANDS:
        for kern in ("w8", "w4"):
            dec, sd, p, z, c = _band_case(cs, fs)
            dec.kernel = kern
            exact, amax = decoder_f64(sd, p, z, c, return_amax=True)
            ref32 = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
            with torch.no_grad():
                out = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
            hip.device_status()
            assert dec.ka == 6, "band %s tripped the fallback scale" % name
            o = out.cpu().numpy().astype(np.float64)
            e_hip, e_or, e_ho = np.abs(o - exact).max(), np.abs(ref32 - exact).max(), np.abs(o - ref32).max()
            lines.append("%-20s %-6s  %9.2f  %7.1f   %.2e    %.2e        %.2e"
                         % (name, kern, np.abs(exact).max(), amax, e_hip, e_or, e_ho))
            top = np.abs(exact).max()
            if not e_hip <= (tol if tol is not None else 4e-6 * top):
                failures.append(("|HIP - exact|", name, kern, e_hip))
            if not e_ho <= (tol if tol is not None else 4e-6 * top) + e_or:
                failures.append(("|HIP - oracle|", name, kern, e_ho, e_or))
            if not e_hip <= 1.25 * e_or + 2e-6:
                failures.append(("HIP further from exact than the fp32 oracle", name, kern, e_hip, e_or))
    print("\n".join(lines))
    out_dir = os.environ.get("RFD_BANDS_OUT")
    if out_dir:
        with open(out_dir, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    assert not failures, failures


def test_decoder_logit_band_beyond_the_default_scale(hip, oracle):
    """codes x7: activations up to ~1100 (x 2^6 beyond the f16 range) and |logit| up to ~190 -- the launch is answered
    by the fallback scale 2^3 (one re-run, kept), and the logits stay fp32-class: relative to max |logit| the error is
    below the fp32 oracle's own (the absolute 1e-4 has no meaning at |logit| 190: one fp32 ulp there is 1.5e-5)."""
    from dec_f64 import decoder_f64
    for kern in ("w8", "w4"):
        dec, sd, p, z, c = _band_case(7.0, 1.0)
        dec.kernel = kern
        exact, amax = decoder_f64(sd, p, z, c, return_amax=True)
        assert amax * 64 > 65504 > amax * 8
        ref32 = oracle.decoder_cbn(oracle.decoder_param_blob(sd), p, z, c)
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="f16 range"):
            out = dec(torch.from_numpy(p).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda())
        hip.device_status()
        assert dec.ka == 3
        o = out.cpu().numpy().astype(np.float64)
        m = np.abs(exact).max()
        e_hip, e_or = np.abs(o - exact).max(), np.abs(ref32 - exact).max()
        print("codes x7 %s: |logit| max %.1f, act max %.0f, fallback scale: |HIP-f64| %.2e (%.1e relative), "
              "|oracle32-f64| %.2e" % (kern, m, amax, e_hip, e_hip / m, e_or))
        assert e_hip / m < 4e-6
        assert e_hip <= 1.25 * e_or + 2e-6
