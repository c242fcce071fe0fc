"""Plain-torch restatement of one PointnetSAModuleVotes -> PointnetFPModule chain with a scalar loss, run on the CPU in
float64 and in float32 on given FPS / ball-query / three_nn indices: the yardstick of the module-level gradient test of
tests/test_gpu_ops_grad.py, with the margins that keep the gradient's route (which side of each ReLU, which neighbour of
each max-pool) away from rounding (asserted for the chosen input seed by tests/test_ops_grad_cpu.py); and the small
float64 torch helpers both test files use."""
import numpy as np
import torch

f64 = np.float64


def rel_close(a, b, tol=1e-12):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def t64(a):
    return torch.from_numpy(np.asarray(a, f64))


def tl(a):
    return torch.from_numpy(np.asarray(a, np.int64))


SA_FP = dict(B=2, N=256, npoint=32, nsample=8, radius=0.4, C=4, sa_mlp=[4, 16, 16], fp_mlp=[16 + 4, 16],
             sa_seed=201, fp_seed=202, seed=0)
MARGIN = 64.0


def sa_fp_modules():
    from rfdnet_amd import synthetic
    from rfdnet_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule, PointnetSAModuleVotes
    sa = PointnetSAModuleVotes(mlp=list(SA_FP["sa_mlp"]), npoint=SA_FP["npoint"], radius=SA_FP["radius"],
                               nsample=SA_FP["nsample"], use_xyz=True, normalize_xyz=True)
    fp = PointnetFPModule(mlp=list(SA_FP["fp_mlp"]))
    synthetic.load_seeded(sa, SA_FP["sa_seed"])
    synthetic.load_seeded(fp, SA_FP["fp_seed"])
    return sa.eval(), fp.eval()


def sa_fp_inputs(seed):
    """-> xyz (B,N,3), features (B,C,N), the loss's fixed weighting (B,16,N), all fp32"""
    rng = np.random.default_rng([5, seed])
    B, N, C = SA_FP["B"], SA_FP["N"], SA_FP["C"]
    return (rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), rng.standard_normal((B, C, N)).astype(np.float32),
            rng.standard_normal((B, SA_FP["fp_mlp"][-1], N)).astype(np.float32))


def oracle_indices(oracle, xyz):
    """the non-differentiable indices: FPS, ball query, the three nearest centres"""
    inds = oracle.furthest_point_sampling(xyz, SA_FP["npoint"])
    new_xyz = np.stack([xyz[i][inds[i]] for i in range(xyz.shape[0])])
    idx = oracle.ball_query(new_xyz, xyz, SA_FP["radius"], SA_FP["nsample"])
    _, nn_idx = oracle.three_nn(xyz, new_xyz)
    return inds, idx, nn_idx


def _run_mlp(mlp, h, pre):
    for layer in mlp:
        if isinstance(layer, torch.nn.ReLU):
            pre.append(h)
            h = torch.relu(h)
        else:
            h = layer(h)
    return h


def sa_fp_restatement(dtype, sa, fp, xyz, feats, wl, inds, idx, nn_idx):
    """SA -> FP -> sum(out * wl) in plain torch on the CPU in `dtype`, on the given indices: grouping and interpolation
    are advanced indexing, the shared MLPs deep copies of the modules' (eval-mode BatchNorm).  -> dict: `out`, `d_feats`,
    `d_<parameter>`; `pre` (every ReLU's input) and `pool_in` (the max-pool's input) for the margins."""
    import copy
    mlp_sa = copy.deepcopy(sa.mlp_module).cpu().to(dtype).eval()
    mlp_fp = copy.deepcopy(fp.mlp).cpu().to(dtype).eval()
    x = torch.from_numpy(xyz).to(dtype)
    f = torch.from_numpy(feats).to(dtype).requires_grad_()
    inds, idx, nn_idx = tl(inds), tl(idx), tl(nn_idx)
    B = x.shape[0]
    rows = torch.arange(B)[:, None]
    new_xyz = x[rows, inds]                                                      # (B, npoint, 3)
    g_xyz = (x[rows[:, :, None], idx] - new_xyz[:, :, None]).permute(0, 3, 1, 2) / SA_FP["radius"]
    g_f = torch.stack([f[i][:, idx[i]] for i in range(B)])                       # (B, C, npoint, nsample)
    pre = []
    pool_in = _run_mlp(mlp_sa, torch.cat([g_xyz, g_f], 1), pre)
    pooled = pool_in.max(dim=3)[0]                                               # (B, 16, npoint)
    dist = (x[:, :, None] - new_xyz[rows[:, :, None], nn_idx]).pow(2).sum(-1).sqrt()      # (B, N, 3)
    recip = 1.0 / (dist + 1e-8)
    weight = recip / recip.sum(2, keepdim=True)
    interp = (torch.stack([pooled[i][:, nn_idx[i]] for i in range(B)]) * weight[:, None]).sum(-1)
    out = _run_mlp(mlp_fp, torch.cat([interp, f], 1).unsqueeze(-1), pre).squeeze(-1)
    (out * torch.from_numpy(wl).to(dtype)).sum().backward()
    res = {"out": out.detach(), "d_feats": f.grad}
    for tag, mlp in (("sa.mlp_module.", mlp_sa), ("fp.mlp.", mlp_fp)):
        for k, p in mlp.named_parameters():
            res["d_" + tag + k] = p.grad
    return {k: v.double().numpy() for k, v in res.items()}, [p.detach().double().numpy() for p in pre], \
        pool_in.detach().double().numpy()


def sa_fp_margins(r64, r32, idx):
    """(ReLU margin, max-pool margin): over every ReLU input, the float64 run's smallest |pre-activation| divided by the
    fp32 run's largest deviation on that tensor; over every pool, the float64 lead of the maximum over the runner-up
    divided by the fp32 run's largest deviation on that tensor.  Both must be >= MARGIN.
    The pool's lead is measured on the INPUT of the ReLU in front of it, where max(relu(x)) = relu(max(x)) has no ties
    at the ReLU's zero: with both margins the route of the gradient is fixed for every pool -- if the largest
    pre-activation is positive it is the one maximum after the ReLU too (the runner-up is either a smaller positive
    value, by the lead, or 0, by the ReLU margin), and if it is negative every member is zero behind a closed ReLU and
    no gradient passes whichever the device picks.  The runner-up is the best value of a DIFFERENT neighbour: a ball
    with fewer than nsample points repeats its first hit, and the copies of one point are one value with one source."""
    (_, pre64, _), (_, pre32, _) = r64, r32
    relu = min(np.abs(a).min() / np.abs(b - a).max() for a, b in zip(pre64, pre32))
    at = len(SA_FP["sa_mlp"]) - 2                                                # the ReLU that feeds the pool
    p64, p32 = pre64[at], pre32[at]                                              # (B, C', npoint, nsample)
    top = p64.argmax(3)
    best = np.take_along_axis(p64, top[..., None], 3)
    top_idx = np.take_along_axis(np.broadcast_to(idx[:, None], p64.shape), top[..., None], 3)
    others = np.where(idx[:, None] != top_idx, p64, -np.inf)
    lead = (best[..., 0] - others.max(3)).min()
    return float(relu), float(lead / np.abs(p32 - p64).max())
