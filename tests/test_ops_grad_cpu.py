"""CPU: tests/ops_grad_f64.py, the float64 restatement the backward kernels are held to (tests/test_gpu_ops_grad.py),
checked itself -- against the C oracle at every shape and index pattern of the GPU test, under the same bound (the
oracle adds in one fixed order, one of the admissible ones); against torch's float64 autograd of plain advanced
indexing, which is not a scatter loop, to 1e-12 relative; and the exact-mode generators for the property the exact mode
rests on: every partial sum, in any order, is representable in fp32."""
import numpy as np
import pytest
import torch

import ops_grad_f64 as G
from sa_fp_f64 import (MARGIN, SA_FP, oracle_indices, rel_close, sa_fp_inputs, sa_fp_margins, sa_fp_modules,
                       sa_fp_restatement, t64, tl)

def oracle_chamfer_indices(oracle, x1, x2):
    _, i1, _, i2 = oracle.chamfer_forward(x1, x2)
    return i1, i2


# ---- restatement vs C oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.GROUP_SHAPES)
def test_group_points_grad_f64_vs_oracle(oracle, shape):
    for label, go, idx, n, exact in G.group_cases(shape):
        G.check(oracle.group_points_grad(go, idx, n), G.group_points_grad(go, idx, n), 1, exact, copy_exact=True)


@pytest.mark.parametrize("npoints", [1, 255, 256, 257, 600])
def test_gather_points_grad_f64_vs_oracle(oracle, npoints):
    for shape in (s for s in G.GATHER_SHAPES if s[3] == npoints):
        for label, go, idx, n, exact in G.gather_cases(shape):
            G.check(oracle.gather_points_grad(go, idx, n), G.gather_points_grad(go, idx, n), 1, exact, copy_exact=True)


@pytest.mark.parametrize("shape", G.INTERP_SHAPES)
def test_three_interpolate_grad_f64_vs_oracle(oracle, shape):
    for label, go, idx, w, m, exact in G.interp_cases(shape):
        G.check(oracle.three_interpolate_grad(go, idx, w, m), G.three_interpolate_grad(go, idx, w, m), 1, exact)


@pytest.mark.parametrize("shape", G.CHAMFER_SHAPES)
def test_chamfer_backward_f64_vs_oracle(oracle, shape):
    for label, x1, x2, gd1, gd2, exact in G.chamfer_cases(shape):
        i1, i2 = oracle_chamfer_indices(oracle, x1, x2)
        if label.startswith("clustered"):
            assert i1.max() < 20, label                     # 20 points of xyz2 receive every assignment
        g1, g2 = oracle.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
        r1, r2 = G.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
        G.check(g1, r1, 2, exact)
        G.check(g2, r2, 2, exact)


# ---- restatement vs torch float64 autograd of plain indexing ---------------------------------------------------------
def indexing_grads(kind, go, idx, n, weight=None):
    """d/d features of sum(grad_out * op(features)) with op written as features[b][:, idx[b]] (and, for the
    interpolation, the weighted sum of the three gathered columns), in float64"""
    b, c = go.shape[:2]
    feats = torch.zeros(b, c, n, dtype=torch.float64, requires_grad=True)
    out = torch.stack([feats[i][:, tl(idx[i])] for i in range(b)])          # (b, c) + idx.shape[1:]
    if kind == "interp":
        out = (out * t64(weight)[:, None]).sum(-1)
    (out * t64(go)).sum().backward()
    return feats.grad.numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (3, 9, 300, 51, 5), (1, 17, 5, 3, 86)])
def test_group_points_grad_f64_vs_autograd(shape):
    for label, go, idx, n, exact in G.group_cases(shape):
        rel_close(G.group_points_grad(go, idx, n)[0], indexing_grads("group", go, idx, n))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 3, 300, 257), (1, 9, 300, 600)])
def test_gather_points_grad_f64_vs_autograd(shape):
    for label, go, idx, n, exact in G.gather_cases(shape):
        rel_close(G.gather_points_grad(go, idx, n)[0], indexing_grads("gather", go, idx, n))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 3, 257, 64), (1, 3, 255, 2), (3, 1, 256, 3)])
def test_three_interpolate_grad_f64_vs_autograd(shape):
    for label, go, idx, w, m, exact in G.interp_cases(shape):
        rel_close(G.three_interpolate_grad(go, idx, w, m)[0], indexing_grads("interp", go, idx, m, w))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 257), (1, 257, 1), (3, 255, 256)])
def test_chamfer_backward_f64_vs_autograd(oracle, shape):
    """min over the full distance matrix; torch's min passes the gradient to one index, the same one as the oracle's
    strict '<' wherever the minimum is unique -- asserted, so the lattice cases (ties by construction) use the random
    points only"""
    for label, x1, x2, gd1, gd2, exact in G.chamfer_cases(shape):
        if exact:
            continue
        i1, i2 = oracle_chamfer_indices(oracle, x1, x2)
        a, b = t64(x1).requires_grad_(), t64(x2).requires_grad_()
        D = ((a[:, :, None] - b[:, None]) ** 2).sum(-1)
        d1, j1 = D.min(2)
        d2, j2 = D.min(1)
        assert np.array_equal(j1.numpy(), i1) and np.array_equal(j2.numpy(), i2), label
        ((d1 * t64(gd1)).sum() + (d2 * t64(gd2)).sum()).backward()
        r1, r2 = G.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
        rel_close(r1[0], a.grad.numpy())
        rel_close(r2[0], b.grad.numpy())


# ---- the exact-mode generators ---------------------------------------------------------------------------------------
def test_exact_generators_keep_every_partial_sum_in_fp32(oracle):
    """terms are multiples of q and sum |terms| / q < 2^24 for every element of every exact case: whatever the order,
    each partial sum is an integer multiple of q below 2^24 q, which fp32 holds exactly"""
    worst = {}
    for shape in G.GROUP_SHAPES:
        for label, go, idx, n, exact in G.group_cases(shape):
            if exact:
                worst["group"] = max(worst.get("group", 0), G.partial_sum_headroom(G.group_points_grad(go, idx, n), 1.0))
    for shape in G.GATHER_SHAPES:
        for label, go, idx, n, exact in G.gather_cases(shape):
            if exact:
                worst["gather"] = max(worst.get("gather", 0),
                                      G.partial_sum_headroom(G.gather_points_grad(go, idx, n), 1.0))
    for shape in G.INTERP_SHAPES:
        for label, go, idx, w, m, exact in G.interp_cases(shape):
            if exact:
                worst["interp"] = max(worst.get("interp", 0),
                                      G.partial_sum_headroom(G.three_interpolate_grad(go, idx, w, m), 0.25))
    for shape in G.CHAMFER_SHAPES:
        for label, x1, x2, gd1, gd2, exact in G.chamfer_cases(shape):
            if exact:
                assert np.abs(x1).max() <= 4 and np.abs(x2).max() <= 4
                assert np.array_equal(x1 * 2, np.round(x1 * 2)) and np.array_equal(gd1, np.round(gd1))
                i1, i2 = oracle_chamfer_indices(oracle, x1, x2)
                for ref in G.chamfer_backward(x1, x2, gd1, i1, gd2, i2):
                    worst["chamfer"] = max(worst.get("chamfer", 0), G.partial_sum_headroom(ref, 1.0))
    print("largest sum|terms| / granularity:", worst)
    assert set(worst) == {"group", "gather", "interp", "chamfer"}
    for k, v in worst.items():
        assert 0 < v < 2 ** 24, (k, v)


def test_patterns_are_what_they_say():
    rng = np.random.default_rng(0)
    p = G.make_idx(rng, "permutation", (3, 16, 16), 300)
    assert p is not None and G.make_idx(rng, "permutation", (1, 51, 5), 5) is None
    assert all(len(np.unique(p[i])) == 256 for i in range(3))
    assert (G.make_idx(rng, "all_last", (2, 7), 300) == 299).all() and (G.make_idx(rng, "all_0", (2, 7), 300) == 0).all()
    assert set(np.unique(G.make_idx(rng, "two_valued", (2, 600), 300))) == {0, 299}
    assert G.make_idx(rng, "first_half", (2, 600), 300).max() < 150 and G.make_idx(rng, "first_half", (2, 6), 1) is None
    t = G.make_idx(rng, "iij", (2, 50, 3), 64)
    assert (t[..., 0] == t[..., 1]).all() and (t[..., 1] != t[..., 2]).any()
    t = G.make_idx(rng, "iii", (2, 50, 3), 64)
    assert (t[..., 0] == t[..., 1]).all() and (t[..., 1] == t[..., 2]).all()
    for shapes, axes in ((G.GROUP_SHAPES, ((1, 3), (1, 7, 8, 9, 17), (1, 5, 300))),
                         (G.INTERP_SHAPES, ((1, 3), (1, 3, 256), (1, 255, 256, 257), (1, 2, 3, 64)))):
        for a, values in enumerate(axes):
            assert {s[a] for s in shapes} == set(values)
    assert {s[3:] for s in G.GROUP_SHAPES} == {(1, 1), (51, 5), (16, 16), (257, 1), (3, 86), (64, 64)}


# ---- the input seed of the SA -> FP gradient test (tests/sa_fp_f64.py) -----------------------------------------------
def test_sa_fp_seed_keeps_the_gradient_route_away_from_rounding(oracle):
    """the input seed of the SA -> FP gradient test, chosen here (seeds 0, 2, 3 of 0 .. 3 qualify; 1 has a ReLU margin
    of 56): see sa_fp_margins.  Every ReLU input and every pool counts, nothing is excluded.
    Seed 0: ReLU margin 254.1, max-pool margin 2798.3."""
    sa, fp = sa_fp_modules()
    xyz, feats, wl = sa_fp_inputs(SA_FP["seed"])
    ind = oracle_indices(oracle, xyz)
    r64 = sa_fp_restatement(torch.float64, sa, fp, xyz, feats, wl, *ind)
    r32 = sa_fp_restatement(torch.float32, sa, fp, xyz, feats, wl, *ind)
    relu, pool = sa_fp_margins(r64, r32, ind[1])
    print("seed %d: ReLU margin %.1f, max-pool margin %.1f (x the fp32 run's deviation)" % (SA_FP["seed"], relu, pool))
    assert relu >= MARGIN and pool >= MARGIN
