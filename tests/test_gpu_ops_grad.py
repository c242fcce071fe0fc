"""GPU (-m gpu): the backward half of the point-op drop-in against float64 -- group_points_grad_kernel,
gather_points_grad_kernel, three_interpolate_grad_kernel (through `pointnet2_ops._ext`) and rfd_chamfer_backward
(through `chamfer_distance`), then the autograd Functions, QueryAndGroup's differentiable branch and one
PointnetSAModuleVotes -> PointnetFPModule chain with grad enabled.

The reference, the bound |device - f64| <= gamma(count - 1 + r) * abssum, the exact zeros / exact copies and the exact
mode (inputs for which every order of addition gives the same bits, so the device must EQUAL float64) are those of
tests/ops_grad_f64.py, which tests/test_ops_grad_cpu.py checks against the C oracle and torch's float64 autograd.  Every
test prints the largest observed error divided by its bound."""
import copy

import numpy as np
import pytest
import torch

import ops_grad_f64 as G
from sa_fp_f64 import (MARGIN, SA_FP, oracle_indices, rel_close, sa_fp_inputs, sa_fp_margins, sa_fp_modules,
                       sa_fp_restatement, t64, tl)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
SENTINEL = 12345.0
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ext(hip):
    from rfdnet_amd.pointnet2_ops import _ext
    return _ext


@pytest.fixture(scope="module")
def pu(hip):
    from rfdnet_amd.pointnet2_ops import pointnet2_utils
    return pointnet2_utils


def report(name, shape, ratios):
    print("%s %s: error / bound  %s" % (name, shape, "  ".join("%s %.3f" % kv for kv in ratios)))


# ---- the kernels, every shape x index pattern x {random values, exact mode} ------------------------------------------
@pytest.mark.parametrize("shape", G.GROUP_SHAPES, ids=lambda s: "b%d-c%d-n%d-m%d-ns%d" % s)
def test_group_points_grad_vs_f64(ext, hip, shape):
    """measured on the MI355X: largest error / bound over all shapes and patterns 0.549 (b3-c8-n300-m16-ns16, first
    half); every exact-mode case bit-equal"""
    ratios = []
    for label, go, idx, n, exact in G.group_cases(shape):
        got = host(ext.group_points_grad(dev(go), dev(idx), n))
        ratios.append((label, G.check(got, G.group_points_grad(go, idx, n), 1, exact, copy_exact=True)))
    hip.device_status()
    report("group_points_grad", shape, ratios)


@pytest.mark.parametrize("npoints", [1, 255, 256, 257, 600])
def test_gather_points_grad_vs_f64(ext, hip, npoints):
    """measured on the MI355X: largest error / bound over all shapes and patterns 0.536 (b3-c9-n300, 257 points, first
    half); every exact-mode case bit-equal"""
    for shape in (s for s in G.GATHER_SHAPES if s[3] == npoints):
        ratios = []
        for label, go, idx, n, exact in G.gather_cases(shape):
            got = host(ext.gather_points_grad(dev(go), dev(idx), n))
            ratios.append((label, G.check(got, G.gather_points_grad(go, idx, n), 1, exact, copy_exact=True)))
        report("gather_points_grad", shape, ratios)
    hip.device_status()


@pytest.mark.parametrize("shape", G.INTERP_SHAPES, ids=lambda s: "b%d-c%d-n%d-m%d" % s)
def test_three_interpolate_grad_vs_f64(ext, hip, shape):
    """measured on the MI355X: largest error / bound over all shapes and patterns 0.973 (b1-c256-n1-m64, random: single
    terms, one rounding each); every exact-mode case bit-equal"""
    ratios = []
    for label, go, idx, w, m, exact in G.interp_cases(shape):
        got = host(ext.three_interpolate_grad(dev(go), dev(idx), dev(w), m))
        ratios.append((label, G.check(got, G.three_interpolate_grad(go, idx, w, m), 1, exact)))
    hip.device_status()
    report("three_interpolate_grad", shape, ratios)


def chamfer_grads(cdm, x1, x2, gd1, gd2):
    """forward + backward through ChamferDistanceFunction with the upstream gradients gd1 / gd2 -> numpy
    (dist1, idx1, dist2, idx2 of the device's forward pass, grad_xyz1, grad_xyz2)"""
    a, b = dev(x1).requires_grad_(), dev(x2).requires_grad_()
    d1, i1, d2, i2 = cdm.nearest(a.detach(), b.detach())
    o1, o2 = cdm.ChamferDistanceFunction.apply(a, b)
    assert torch.equal(o1.detach(), d1) and torch.equal(o2.detach(), d2)
    ((o1 * dev(gd1)).sum() + (o2 * dev(gd2)).sum()).backward()
    return tuple(host(t) for t in (d1, i1, d2, i2, a.grad, b.grad))


@pytest.mark.parametrize("shape", G.CHAMFER_SHAPES, ids=lambda s: "b%d-n%d-m%d" % s)
def test_chamfer_backward_vs_f64(oracle, hip, shape):
    """many-to-one (257 -> 1, 1 <- 257, 1030 -> 20 clustered points: both launches add into the same three words),
    coincident points (terms exactly 0), random and lattice points; the indices are the device's own, equal to the
    oracle's.  measured on the MI355X: largest error / bound over all shapes and kinds 0.966 (b3-n1030-m300, random);
    0.928 clustered, 0.913 coincident; every lattice case bit-equal"""
    from rfdnet_amd import chamfer_distance as cdm
    ratios = []
    for label, x1, x2, gd1, gd2, exact in G.chamfer_cases(shape):
        d1, i1, d2, i2, g1, g2 = chamfer_grads(cdm, x1, x2, gd1, gd2)
        hip.device_status()
        for got, want in zip((d1, i1, d2, i2), oracle.chamfer_forward(x1, x2)):
            np.testing.assert_array_equal(got, want)
        if label.startswith("clustered"):
            assert i1.max() < 20
        if label.startswith("coincident"):
            assert (i1[:, 0] == 0).all() and (d1[:, 0] == 0).all() and (d2[:, 0] == 0).all()
        if shape[2] == 1:
            assert (i1 == 0).all()
        if shape[1] == 1:
            assert (i2 == 0).all()
        r1, r2 = G.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
        ratios.append((label, max(G.check(g1, r1, 2, exact), G.check(g2, r2, 2, exact))))
    report("chamfer_backward", shape, ratios)


def test_chamfer_mean_backward_twice(oracle, hip):
    """loss = d1.mean() + d2.mean(): the upstream gradients arrive as stride-0 expansions of one scalar.  Two backward
    passes over one graph: the second result is written into fresh torch.empty_like memory (as a rule the block the
    first result has just left) and must meet the bound on its own, not hold twice the gradient -- the launcher zeroes
    both outputs on every call.  measured on the MI355X: error / bound 0.566 / 0.887 (xyz1 / xyz2) for both passes,
    0.454 / 0.607 under sum()"""
    from rfdnet_amd import chamfer_distance as cdm
    rng = np.random.default_rng(77)
    b, n, m = 3, 257, 600
    x1 = rng.standard_normal((b, n, 3)).astype(f32)
    x2 = rng.standard_normal((b, m, 3)).astype(f32)
    a, c = dev(x1).requires_grad_(), dev(x2).requires_grad_()
    o1, o2 = cdm.ChamferDistanceFunction.apply(a, c)
    loss = o1.mean() + o2.mean()
    loss.backward(retain_graph=True)
    first = host(a.grad), host(c.grad)
    a.grad = c.grad = None                                  # hand the blocks back to the allocator
    loss.backward()
    hip.device_status()
    second = host(a.grad), host(c.grad)
    _, i1, _, i2 = oracle.chamfer_forward(x1, x2)
    _, j1, _, j2 = cdm.nearest(a.detach(), c.detach())
    np.testing.assert_array_equal(host(j1), i1)
    np.testing.assert_array_equal(host(j2), i2)
    gd1 = np.full((b, n), f32(1.0) / f32(b * n), f32)       # mean's backward: 1 / numel, one fp32 division
    gd2 = np.full((b, m), f32(1.0) / f32(b * m), f32)
    refs = G.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
    ratios = []
    for tag, got, ref in (("first/xyz1", first[0], refs[0]), ("first/xyz2", first[1], refs[1]),
                          ("second/xyz1", second[0], refs[0]), ("second/xyz2", second[1], refs[1])):
        ratios.append((tag, G.check(got, ref, 2)))
    for s, f in zip(second, first):
        assert np.abs(f).max() > 0 and np.abs(s - 2 * f).max() > 0.5 * np.abs(f).max()
    # sum(): the upstream gradient is the scalar 1 expanded, stride 0 whatever mean()'s backward materialises
    a, c = dev(x1).requires_grad_(), dev(x2).requires_grad_()
    o1, o2 = cdm.ChamferDistanceFunction.apply(a, c)
    (o1.sum() + o2.sum()).backward()
    hip.device_status()
    refs = G.chamfer_backward(x1, x2, np.ones((b, n), f32), i1, np.ones((b, m), f32), i2)
    ratios += [("sum/xyz1", G.check(host(a.grad), refs[0], 2)), ("sum/xyz2", G.check(host(c.grad), refs[1], 2))]
    report("chamfer mean().backward() x 2", (b, n, m), ratios)


# ---- nothing is written outside (B, C, n): the C ABI on an output slice between sentinels ----------------------------
def guarded(numel, fill):
    big = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    big[GUARD:GUARD + numel] = fill
    return big, big[GUARD:GUARD + numel]


def assert_guards(big):
    h = host(big)
    np.testing.assert_array_equal(h[:GUARD], f32(SENTINEL))
    np.testing.assert_array_equal(h[-GUARD:], f32(SENTINEL))


def test_grad_kernels_write_only_their_output(oracle, hip):
    """one tail shape per kernel, ordinary in-bounds calls: the output is a slice of a larger tensor with 64 sentinel
    floats on either side (zeroed by hand for the three kernels that add into a zero-initialised output, left at NaN
    for rfd_chamfer_backward, which zeroes its own); the sentinels are unchanged and the slice meets the bound"""
    d = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(99)
    b, c, n, m, ns = 3, 9, 5, 3, 86                                          # m * ns = 258, c = 8 + 1
    go, idx = G.make_grad_out(rng, (b, c, m, ns), False), G.make_idx(rng, "two_valued", (b, m, ns), n)
    big, out = guarded(b * c * n, 0.0)
    go_d, idx_d = dev(go), dev(idx)
    hip.call("group_points_grad_kernel_wrapper", d, b, c, n, m, ns, go_d.data_ptr(), idx_d.data_ptr(), out.data_ptr())
    hip.device_status()
    assert_guards(big)
    G.check(host(out).reshape(b, c, n), G.group_points_grad(go, idx, n), 1, copy_exact=True)

    b, c, n, m = 3, 3, 7, 257
    go, idx = G.make_grad_out(rng, (b, c, m), False), G.make_idx(rng, "two_valued", (b, m), n)
    big, out = guarded(b * c * n, 0.0)
    go_d, idx_d = dev(go), dev(idx)
    hip.call("gather_points_grad_kernel_wrapper", d, b, c, n, m, go_d.data_ptr(), idx_d.data_ptr(), out.data_ptr())
    hip.device_status()
    assert_guards(big)
    G.check(host(out).reshape(b, c, n), G.gather_points_grad(go, idx, n), 1, copy_exact=True)

    b, c, n, m = 3, 3, 257, 3
    go, idx, w = (G.make_grad_out(rng, (b, c, n), False), G.make_idx(rng, "two_valued", (b, n, 3), m),
                  G.make_weight(rng, (b, n, 3), False))
    big, out = guarded(b * c * m, 0.0)
    go_d, idx_d, w_d = dev(go), dev(idx), dev(w)
    hip.call("three_interpolate_grad_kernel_wrapper", d, b, c, n, m, go_d.data_ptr(), idx_d.data_ptr(), w_d.data_ptr(),
             out.data_ptr())
    hip.device_status()
    assert_guards(big)
    G.check(host(out).reshape(b, c, m), G.three_interpolate_grad(go, idx, w, m), 1)

    b, n, m = 3, 257, 5
    x1, x2 = rng.standard_normal((b, n, 3)).astype(f32), rng.standard_normal((b, m, 3)).astype(f32)
    gd1, gd2 = rng.standard_normal((b, n)).astype(f32), rng.standard_normal((b, m)).astype(f32)
    _, i1, _, i2 = oracle.chamfer_forward(x1, x2)
    big1, out1 = guarded(b * n * 3, float("nan"))
    big2, out2 = guarded(b * m * 3, float("nan"))
    t = [dev(v) for v in (x1, x2, gd1, i1, gd2, i2)]
    hip.call("rfd_chamfer_backward", d, b, n, t[0].data_ptr(), m, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
             t[4].data_ptr(), t[5].data_ptr(), out1.data_ptr(), out2.data_ptr())
    hip.device_status()
    assert_guards(big1)
    assert_guards(big2)
    r1, r2 = G.chamfer_backward(x1, x2, gd1, i1, gd2, i2)
    G.check(host(out1).reshape(b, n, 3), r1, 2)
    G.check(host(out2).reshape(b, m, 3), r2, 2)


# ---- the autograd Functions ------------------------------------------------------------------------------------------
class Saved(object):
    """stands in for a Function's ctx when backward() is called directly (to see ALL it returns)"""

    def __init__(self, *tensors):
        self.saved_tensors = tensors


def none_or_zeros(t, like):
    return t is None or (t.shape == like.shape and not t.any())


def test_gather_operation_backward(pu, hip):
    """non-contiguous upstream gradient ((out^T * W).sum()), against torch-float64 autograd of features[b][:, idx[b]];
    backward returns (grad, None) as the reference does.  measured on the MI355X: error / bound 0.512"""
    rng = np.random.default_rng(41)
    b, c, n, m = 3, 9, 300, 257
    feats, idx = rng.standard_normal((b, c, n)).astype(f32), rng.integers(0, n, (b, m)).astype(np.int32)
    W = rng.standard_normal((b, m, c)).astype(f32)
    f, idx_d = dev(feats).requires_grad_(), dev(idx)
    out = pu.gather_operation(f, idx_d)
    (out.transpose(1, 2) * dev(W)).sum().backward()
    hip.device_status()
    w64 = t64(feats).requires_grad_()
    o64 = torch.stack([w64[i][:, tl(idx[i])] for i in range(b)])
    np.testing.assert_array_equal(host(out).astype(f64), o64.detach().numpy())
    (o64.transpose(1, 2) * t64(W)).sum().backward()
    ref = G.gather_points_grad(np.ascontiguousarray(W.transpose(0, 2, 1)), idx, n)
    rel_close(ref[0], w64.grad.numpy())
    ratio = G.check(host(f.grad), (w64.grad.numpy(),) + ref[1:], 1, copy_exact=True)
    g = dev(W).transpose(1, 2)
    assert not g.is_contiguous()
    back = pu.GatherOperation.backward(Saved(idx_d, f.detach()), g)
    assert len(back) == 2 and none_or_zeros(back[1], idx_d)
    G.check(host(back[0]), ref, 1, copy_exact=True)
    report("gather_operation", (b, c, n, m), [("transposed", ratio)])


def test_grouping_operation_backward(pu, hip):
    """upstream gradients (out^T * W).sum() (non-contiguous) and out.max(dim=3)[0] weighted by W (zero but for one
    neighbour per group), against torch-float64 autograd of the indexing; the values of a feature row are distinct
    (asserted), so the maximum's source is unique even where a group repeats an index.  backward returns zeros (or None)
    for idx.  measured on the MI355X: error / bound 0.495 (transposed), 0.475 (max)"""
    rng = np.random.default_rng(42)
    b, c, n, m, ns = 3, 9, 300, 51, 5
    feats, idx = rng.standard_normal((b, c, n)).astype(f32), rng.integers(0, n, (b, m, ns)).astype(np.int32)
    idx[:, ::3, 1:] = idx[:, ::3, :1]                       # padded groups, as ball_query writes them
    assert all(len(np.unique(row)) == n for row in feats.reshape(-1, n))
    W = {"transposed": rng.standard_normal((b, m, c, ns)).astype(f32), "max": rng.standard_normal((b, c, m)).astype(f32)}
    idx_d = dev(idx)
    ratios = []
    for kind in ("transposed", "max"):
        f = dev(feats).requires_grad_()
        out = pu.grouping_operation(f, idx_d)
        w64 = t64(feats).requires_grad_()
        o64 = torch.stack([w64[i][:, tl(idx[i])] for i in range(b)])
        o64.retain_grad()
        np.testing.assert_array_equal(host(out).astype(f64), o64.detach().numpy())
        if kind == "transposed":
            (out.transpose(1, 2) * dev(W[kind])).sum().backward()
            (o64.transpose(1, 2) * t64(W[kind])).sum().backward()
        else:
            (out.max(dim=3)[0] * dev(W[kind])).sum().backward()
            (o64.max(dim=3)[0] * t64(W[kind])).sum().backward()
        hip.device_status()
        ref = G.group_points_grad(o64.grad.numpy(), idx, n)
        rel_close(ref[0], w64.grad.numpy())
        ratios.append((kind, G.check(host(f.grad), (w64.grad.numpy(),) + ref[1:], 1, copy_exact=True)))
    g = dev(W["transposed"]).transpose(1, 2)
    assert not g.is_contiguous()
    back = pu.GroupingOperation.backward(Saved(idx_d, dev(feats)), g)
    assert len(back) == 2 and none_or_zeros(back[1], idx_d)
    report("grouping_operation", (b, c, n, m, ns), ratios)


def test_three_interpolate_backward(pu, hip):
    """non-contiguous upstream gradient against torch-float64 autograd of the weighted sum of three gathered columns;
    backward returns zeros for idx and for weight (the reference's convention: no gradient reaches the weights).
    measured on the MI355X: error / bound 0.314"""
    rng = np.random.default_rng(43)
    b, c, n, m = 3, 9, 257, 64
    feats = rng.standard_normal((b, c, m)).astype(f32)
    idx, w = rng.integers(0, m, (b, n, 3)).astype(np.int32), rng.random((b, n, 3)).astype(f32)
    idx[:, ::4, 1] = idx[:, ::4, 0]                         # rows (i, i, j)
    W = rng.standard_normal((b, n, c)).astype(f32)
    f, idx_d, w_d = dev(feats).requires_grad_(), dev(idx), dev(w).requires_grad_()
    out = pu.three_interpolate(f, idx_d, w_d)
    (out.transpose(1, 2) * dev(W)).sum().backward()
    hip.device_status()
    assert w_d.grad is None or not w_d.grad.any()
    w64 = t64(feats).requires_grad_()
    o64 = (torch.stack([w64[i][:, tl(idx[i])] for i in range(b)]) * t64(w)[:, None]).sum(-1)
    (o64.transpose(1, 2) * t64(W)).sum().backward()
    ref = G.three_interpolate_grad(np.ascontiguousarray(W.transpose(0, 2, 1)), idx, w, m)
    rel_close(ref[0], w64.grad.numpy())
    ratio = G.check(host(f.grad), (w64.grad.numpy(),) + ref[1:], 1)
    back = pu.ThreeInterpolate.backward(Saved(idx_d, w_d.detach(), f.detach()), dev(W).transpose(1, 2))
    assert len(back) == 3 and none_or_zeros(back[1], idx_d)
    assert back[2] is not None and back[2].shape == w_d.shape and not back[2].any()
    report("three_interpolate", (b, c, n, m), [("transposed", ratio)])


# ---- QueryAndGroup: the differentiable branch against the fused one, then against float64 ----------------------------
@pytest.mark.parametrize("B,N,M,ns,C", [(2, 512, 32, 8, 5),        # fused branch: features gathered from LDS
                                        (2, 301, 13, 5, 5)])       # N and M * ns no multiples of 4: gathered from L2
def test_query_and_group_branches_and_gradients(pu, oracle, hip, B, N, M, ns, C):
    """both outputs of the needs_grad branch equal the fused group_concat branch bit for bit, for every combination of
    normalize_xyz, use_xyz and features given / None; then d/d features and d/d xyz of a fixed weighting of BOTH
    outputs against torch-float64 autograd of the indexing composition.
    Bound: ops_grad_f64's with r = 1 for the features (copies); for xyz r = 1 without normalize_xyz (the term is the
    sum of the two upstream gradients, fl(W_features + W_grouped)) and r = 4 with it, the term being
    fl(fl(W_features + W_grouped) * fl(1 / fl(radius))): that sum, the radius in fp32, its reciprocal and the product.
    measured on the MI355X: error / bound for xyz at most 0.999 without normalize_xyz (N = 301, use_xyz, features: single
    terms, one rounding each) and 0.492 with it; 0.563 for the features"""
    radius = 0.37
    rng = np.random.default_rng(N)
    xyz = rng.uniform(-1, 1, (B, N, 3)).astype(f32)
    new = xyz[:, :M].copy()
    feats = rng.standard_normal((B, C, N)).astype(f32)
    xyz_d, new_d, feats_d = dev(xyz), dev(new), dev(feats)
    idx = oracle.ball_query(new, xyz, radius, ns)
    np.testing.assert_array_equal(host(pu.ball_query(radius, ns, xyz_d, new_d)), idx)
    assert len({len(np.unique(g)) for g in idx.reshape(-1, ns)}) > 1       # full and padded balls
    ratios = []
    for normalize, use_xyz, with_f in [(nz, ux, wf) for nz in (False, True) for ux in (False, True)
                                       for wf in (False, True) if ux or wf]:
        qg = pu.QueryAndGroup(radius, ns, use_xyz=use_xyz, ret_grouped_xyz=True, normalize_xyz=normalize)
        with torch.no_grad():
            nf0, gx0 = qg(xyz_d, new_d, feats_d if with_f else None)
        x = xyz_d.clone().requires_grad_()
        f = feats_d.clone().requires_grad_() if with_f else None
        nf1, gx1 = qg(x, new_d, f)
        assert nf1.requires_grad and gx1.requires_grad and not nf0.requires_grad
        np.testing.assert_array_equal(host(nf1), host(nf0))
        np.testing.assert_array_equal(host(gx1), host(gx0))
        ctot = (3 if (use_xyz or not with_f) else 0) + (C if with_f else 0)
        assert nf1.shape == (B, ctot, M, ns) and gx1.shape == (B, 3, M, ns)
        W = rng.standard_normal((B, ctot, M, ns)).astype(f32)
        W2 = rng.standard_normal((B, 3, M, ns)).astype(f32)
        ((nf1 * dev(W)).sum() + (gx1 * dev(W2)).sum()).backward()
        hip.device_status()

        x64 = t64(xyz).requires_grad_()
        raw = torch.stack([x64[i].t()[:, tl(idx[i])] for i in range(B)])                 # (B, 3, M, ns)
        raw.retain_grad()
        gx = raw - t64(new).transpose(1, 2).unsqueeze(-1)
        if normalize:
            gx = gx / radius
        if with_f:
            f64_ = t64(feats).requires_grad_()
            gf = torch.stack([f64_[i][:, tl(idx[i])] for i in range(B)])
            gf.retain_grad()
            nf = torch.cat([gx, gf], 1) if use_xyz else gf
        else:
            nf = gx
        ((nf * t64(W)).sum() + (gx * t64(W2)).sum()).backward()
        tag = "%s%s%s" % ("n" if normalize else "-", "x" if use_xyz else "-", "f" if with_f else "-")
        ref = G.group_points_grad(raw.grad.numpy(), idx, N)
        rel_close(ref[0], x64.grad.numpy().transpose(0, 2, 1))
        ratios.append((tag + "/xyz", G.check(np.ascontiguousarray(host(x.grad).transpose(0, 2, 1)), ref,
                                             4 if normalize else 1)))
        if with_f:
            ref = G.group_points_grad(gf.grad.numpy(), idx, N)
            rel_close(ref[0], f64_.grad.numpy())
            ratios.append((tag + "/features", G.check(host(f.grad), ref, 1, copy_exact=True)))
    report("QueryAndGroup", (B, N, M, ns, C), ratios)


# ---- PointnetSAModuleVotes -> PointnetFPModule with grad enabled -----------------------------------------------------
def test_sa_fp_forward_and_gradients_vs_f64(pu, ext, oracle, hip):
    """eval mode, grad enabled (the modules take the op chain: group -> shared MLP -> max, three_nn -> three_interpolate
    -> cat -> shared MLP), seeded weights with non-trivial running statistics; the loss is a fixed random weighting of
    the FP output.  Forward output, d/d input features and the gradient of every parameter against the float64
    restatement of tests/sa_fp_f64.py on the device's own FPS / ball-query / three_nn indices (equal to the
    oracle's).  Per tensor max|device - f64| <= max(8 x max|cpu32 - f64|, 64 * 2^-24 * max|f64|): the fp32 CPU run of the
    same restatement is the yardstick (the convention of tests/test_gpu_loss.py).
    The input seed (SA_FP['seed'] = 0) was chosen on the CPU so that no ReLU and no max-pool can go another way in
    fp32: ReLU margin 254.1, max-pool margin 2798.3 (sa_fp_margins; both must be >= 64, asserted here too, nothing
    excluded).  measured on the MI355X: max|device - f64| (max|cpu32 - f64|) out 1.5e-7 (2.4e-7), d_feats 1.8e-7
    (1.6e-7), parameter gradients 3.7e-7 ... 7.1e-6 (3.9e-7 ... 7.4e-6), the largest ratio device / cpu32 1.43
    (sa.mlp_module.4.weight) against the 8 allowed"""
    sa, fp = sa_fp_modules()
    xyz, feats, wl = sa_fp_inputs(SA_FP["seed"])
    sa_d, fp_d = copy.deepcopy(sa).cuda().eval(), copy.deepcopy(fp).cuda().eval()
    x, f = dev(xyz), dev(feats).requires_grad_()
    assert torch.is_grad_enabled()
    new_xyz, sa_feat, inds = sa_d(x, f)
    out = fp_d(x, new_xyz, f, sa_feat)
    assert sa_feat.grad_fn is not None and out.grad_fn is not None
    idx = pu.ball_query(SA_FP["radius"], SA_FP["nsample"], x, new_xyz)
    _, nn_idx = ext.three_nn(x, new_xyz)
    ind = oracle_indices(oracle, xyz)
    for got, want in zip((inds, idx, nn_idx), ind):
        np.testing.assert_array_equal(host(got), want)
    (out * dev(wl)).sum().backward()
    hip.device_status()

    r64 = sa_fp_restatement(torch.float64, sa, fp, xyz, feats, wl, *ind)
    r32 = sa_fp_restatement(torch.float32, sa, fp, xyz, feats, wl, *ind)
    relu, pool = sa_fp_margins(r64, r32, ind[1])
    print("seed %d: ReLU margin %.1f, max-pool margin %.1f" % (SA_FP["seed"], relu, pool))
    assert relu >= MARGIN and pool >= MARGIN

    got = {"out": out, "d_feats": f.grad}
    for tag, mlp in (("sa.mlp_module.", sa_d.mlp_module), ("fp.mlp.", fp_d.mlp)):
        for k, p in mlp.named_parameters():
            got["d_" + tag + k] = p.grad
    assert set(got) == set(r64[0]) and len(got) == 2 + 3 * 3
    failed = []
    for k in sorted(got):
        want = r64[0][k]
        err = np.abs(host(got[k]).astype(f64) - want).max()
        yard = np.abs(r32[0][k] - want).max()
        lim = max(8 * yard, 64 * G.U * np.abs(want).max())
        print("%-32s max|device - f64| %.3e   max|cpu32 - f64| %.3e   bound %.3e" % (k, err, yard, lim))
        assert np.abs(want).max() > 0
        if not err <= lim:
            failed.append(k)
    assert not failed, failed
