"""GPU (-m gpu): the fused set-abstraction layer (csrc/sa_fused.hip) against the op
composition it replaces (ball query -> group_concat -> Conv2d/BN/ReLU x3 -> max)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (npoint, radius, nsample, c_feat, mlp) -- the five parameterisations of the network
# (pointnet2backbone.py:27-61, proposal_module.py:66-73) at reduced point counts
CASES = [
    (512, 0.2, 64, 1, [1, 64, 64, 128]),
    (256, 0.4, 32, 128, [128, 128, 128, 256]),
    (128, 0.8, 16, 256, [256, 128, 128, 256]),
    (64, 1.2, 16, 256, [256, 128, 128, 256]),
    (64, 0.3, 16, 256, [256, 128, 128, 128]),
]


def _module(npoint, radius, nsample, mlp, seed, normalize_xyz=True):
    from rfdnet_amd.pointnet2_ops.pointnet2_modules import PointnetSAModuleVotes
    from rfdnet_amd import synthetic
    mod = PointnetSAModuleVotes(npoint=npoint, radius=radius, nsample=nsample, mlp=list(mlp), use_xyz=True,
                                normalize_xyz=normalize_xyz)
    synthetic.load_seeded(mod, seed)            # non-trivial BN running statistics
    return mod.cuda().eval()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fused_sa_matches_op_composition(hip, case):
    from rfdnet_amd import sa_fused
    npoint, radius, nsample, c_feat, mlp = CASES[case]
    mod = _module(npoint, radius, nsample, mlp, seed=case + 1)
    g = torch.Generator(device="cuda").manual_seed(case)
    B, N = 2, 2048
    xyz = (torch.rand(B, N, 3, device="cuda", generator=g) * 2 - 1).contiguous()
    xyz[:, :8] = 5.0 + torch.arange(8, device="cuda").view(1, 8, 1) * 3.0     # isolated points: sparse / 1-hit balls
    feats = torch.randn(B, c_feat, N, device="cuda", generator=g)
    with torch.no_grad():
        assert sa_fused.usable(mod.mlp_module, feats, nsample, 'max', True)
        new_xyz, fused, inds = mod(xyz, feats)
        # the composition it replaces
        grouped, _ = mod.grouper(xyz, new_xyz, feats)
        ref = mod.mlp_module(grouped).max(dim=3)[0]
    assert fused.shape == ref.shape == (B, mlp[-1], npoint)
    err = (fused - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


def test_fused_sa_with_given_indices_and_empty_balls(hip):
    """Vote aggregation calls the module with `inds`; centres far from every point have no
    neighbour (idx all zero => every row is point 0)."""
    npoint, radius, nsample, c_feat, mlp = CASES[4]
    mod = _module(npoint, radius, nsample, mlp, seed=9)
    g = torch.Generator(device="cuda").manual_seed(3)
    B, N = 1, 1024
    xyz = torch.rand(B, N, 3, device="cuda", generator=g).contiguous()
    xyz[:, 100:110] += 50.0                     # far away: balls around them contain only themselves
    feats = torch.randn(B, c_feat, N, device="cuda", generator=g)
    inds = torch.arange(96, 96 + npoint, device="cuda", dtype=torch.int32).view(1, -1).contiguous()
    with torch.no_grad():
        new_xyz, fused, _ = mod(xyz, feats, inds)
        grouped, _ = mod.grouper(xyz, new_xyz, feats)
        ref = mod.mlp_module(grouped).max(dim=3)[0]
    assert (fused - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


def test_unsupported_widths_fall_back_to_the_composition(hip):
    from rfdnet_amd import sa_fused
    mod = _module(64, 0.5, 16, [8, 32, 32, 64], seed=2)
    feats = torch.randn(1, 8, 512, device="cuda")
    with torch.no_grad():
        assert not sa_fused.usable(mod.mlp_module, feats, 16, 'max', True)
        xyz = torch.rand(1, 512, 3, device="cuda")
        _, out, _ = mod(xyz, feats)
    assert out.shape == (1, 64, 64)


# ---------------------------------------------------------------------------------------------------------------------
# ragged tails against float64 (tests/sa_f64.py): a workgroup owns 128 (centre, neighbour) rows, and every case above
# has npoint * nsample % 128 == 0 -- no dead lane, no dead wave, no half-filled workgroup at 64 neighbours

WIDTHS = [(4, 64, 64, 128), (131, 128, 128, 256), (259, 128, 128, 256), (259, 128, 128, 128)]
# N = 512 points in [-1, 1]^3 are 64 per unit volume: these balls hold about 7, 17 and 34 of them -- partly filled
RADIUS = {16: 0.3, 32: 0.4, 64: 0.5}
B_RAGGED, N_RAGGED = 3, 512


def _ragged_inputs(c_feat, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (B_RAGGED, N_RAGGED, 3)).astype(np.float32)
    # eight isolated points, at the END: furthest-point sampling starts at point 0 (an ordinary point with a partly
    # filled ball) and then takes isolated ones (1-hit balls), so npoint = 1 and 3 see both kinds
    xyz[:, -8:] = 5.0 + np.arange(8, dtype=np.float32).reshape(1, 8, 1) * 3.0
    feats = rng.standard_normal((B_RAGGED, c_feat, N_RAGGED)).astype(np.float32)
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda()


def _check_against_f64(hip, mod, xyz, feats, inds=None):
    """|fused - f64| <= 4 e_ref per element, e_ref = the largest error of the fp32 torch composition against the same
    float64 result: the kernel is exact-fp32 MFMA in another summation order, i.e. the same error class; the factor
    covers the order difference across three layers.  e_ref comes from the reference, never from the kernel."""
    import sa_f64
    from rfdnet_amd import sa_fused
    with torch.no_grad():
        assert sa_fused.usable(mod.mlp_module, feats, mod.nsample, 'max', True)      # no silent fallback
        new_xyz, fused, inds = mod(xyz, feats, inds)
        want, ref32 = sa_f64.sa_layer_f64(mod, xyz, new_xyz, feats)
    hip.device_status()
    e_ref = (ref32.double() - want).abs().max().item()
    err = (fused.double() - want).abs().max().item()
    convs = [m for m in mod.mlp_module if isinstance(m, torch.nn.Conv2d)]
    print("sa_fused %s nsample %d npoint %d vs f64: e_ref (fp32 torch) = %.3e, kernel = %.3e, max|f64| = %.3g" % (
        "x".join(str(n) for n in [convs[0].in_channels] + [cv.out_channels for cv in convs]), mod.nsample, mod.npoint,
        e_ref, err, want.abs().max().item()))
    assert fused.shape == want.shape == (xyz.shape[0], convs[-1].out_channels, mod.npoint)
    assert torch.isfinite(fused).all() and e_ref > 0
    assert err <= 4 * e_ref, (err, e_ref)
    return fused, inds


@pytest.mark.parametrize("npoint", [1, 3, 67])
@pytest.mark.parametrize("nsample", [16, 32, 64])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_fused_sa_ragged_tails_against_float64(hip, widths, nsample, npoint):
    """npoint * nsample % 128 = 16, 48, 32, 96, 64: dead lanes in a wave, dead waves in a workgroup, and at 64
    neighbours an odd centre count (one live centre beside two dead waves in the LDS combine)"""
    from rfdnet_amd import sa_fused
    assert set(WIDTHS) == sa_fused.SHAPES
    assert (npoint * nsample) % 128 != 0
    c_feat = widths[0] - 3
    mod = _module(npoint, RADIUS[nsample], nsample, [c_feat] + list(widths[1:]), seed=WIDTHS.index(widths) + 11)
    xyz, feats = _ragged_inputs(c_feat, seed=1000 * WIDTHS.index(widths) + 10 * nsample + npoint)
    _check_against_f64(hip, mod, xyz, feats)


def test_fused_sa_ragged_with_given_indices_first_last_and_repeated(hip):
    """vote aggregation's widths with `inds` naming point 0, point N - 1 and one centre twice: five centres of 64
    neighbours (the last workgroup holds one centre and two dead waves); a repeated centre gives the same bits"""
    widths, nsample, npoint = WIDTHS[3], 64, 5
    c_feat = widths[0] - 3
    mod = _module(npoint, RADIUS[nsample], nsample, [c_feat] + list(widths[1:]), seed=21)
    xyz, feats = _ragged_inputs(c_feat, seed=77)
    inds = torch.tensor([[0, N_RAGGED - 1, 7, 100, 7]] * B_RAGGED, dtype=torch.int32, device="cuda")
    inds[1] = torch.tensor([200, 0, 33, 200, N_RAGGED - 1], dtype=torch.int32)
    fused, _ = _check_against_f64(hip, mod, xyz, feats, inds.contiguous())
    assert torch.equal(fused[0, :, 2], fused[0, :, 4]) and torch.equal(fused[2, :, 2], fused[2, :, 4])
    assert torch.equal(fused[1, :, 0], fused[1, :, 3])


@pytest.mark.parametrize("widths,nsample,npoint", [(WIDTHS[0], 16, 3), (WIDTHS[1], 64, 3)],
                         ids=["4x64x64x128-16", "131x128x128x256-64"])
def test_fused_sa_ragged_without_xyz_normalisation(hip, widths, nsample, npoint):
    """normalize_xyz=False: inv_r = 1, the relative coordinates enter the first layer unscaled"""
    c_feat = widths[0] - 3
    mod = _module(npoint, RADIUS[nsample], nsample, [c_feat] + list(widths[1:]), seed=31, normalize_xyz=False)
    assert mod.grouper.normalize_xyz is False
    xyz, feats = _ragged_inputs(c_feat, seed=78)
    _check_against_f64(hip, mod, xyz, feats)
