"""float64 numpy restatement of the four scatter-add backward kernels -- group_points_grad (csrc/group_points.hip),
gather_points_grad (csrc/sampling.hip), three_interpolate_grad (csrc/interpolate.hip) and rfd_chamfer_backward
(csrc/chamfer.hip) -- with the shapes, index patterns and input generators that tests/test_ops_grad_cpu.py (against the C
oracle and torch's float64 autograd) and tests/test_gpu_ops_grad.py (against the kernels) share.

Every function scatter-adds with np.add.at the products formed from the fp32 inputs widened to float64, and returns
three arrays of the output's shape: the gradient, `count` (the number of terms added into the element) and `abssum` (the
sum of |term|).

The bound.  A kernel's output element is the fp32 sum, in an order the atomics choose, of its `count` terms; each term is
itself the result of r rounded fp32 operations (r = 1: a plain copy for group / gather, counted as one, and the product
g * w of the interpolation; r = 2: the difference and the product of Chamfer's 2 g (a - b), the factor 2 being exact).
With u = 2^-24 and gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: any
order of count - 1 additions on top of r roundings per term),

    |device - f64| <= gamma(count - 1 + r) * abssum,

an element with count == 0 must be exactly 0.0 and, for group / gather, one with count == 1 must equal its single term
bit for bit.  `bound()` and `check()` state exactly this.

Exact mode.  gamma * abssum cannot tell a reordered sum from a lost, doubled or misplaced atomic once abssum is large.
The `exact=True` generators therefore produce inputs whose every term is a multiple of a granularity q (a power of two)
and whose every partial sum, in ANY order, is below 2^24 q in magnitude (`partial_sum_headroom`), hence representable in
fp32: all orders of addition give the same bits, and the device must equal the float64 result under
assert_array_equal.  grad_out holds integers in [-8, 8], interpolation weights lie in {0.25, 0.5, 1, 2}, Chamfer points on
the lattice of multiples of 0.5 in [-4, 4] with an integer grad_dist."""
import numpy as np

U = 2.0 ** -24
f32, f64 = np.float32, np.float64


def gamma(k):
    k = np.asarray(k, f64)
    return k * U / (1.0 - k * U)


def bound(count, abssum, r):
    """gamma(count - 1 + r) * abssum; 0 where nothing is added"""
    return np.where(count > 0, gamma(np.maximum(count, 1) - 1 + r) * abssum, 0.0)


def _scatter(shape, where, terms):
    out = [np.zeros(shape, f64), np.zeros(shape, np.int64), np.zeros(shape, f64)]
    np.add.at(out[0], where, terms)
    np.add.at(out[1], where, 1)
    np.add.at(out[2], where, np.abs(terms))
    return tuple(out)


def group_points_grad(grad_out, idx, n):
    """grad_out (B,C,M,ns), idx (B,M,ns) -> (grad, count, abssum), each (B,C,n)"""
    b, c, m, ns = grad_out.shape
    bi, ci, ii = np.broadcast_arrays(np.arange(b)[:, None, None, None], np.arange(c)[None, :, None, None],
                                     idx.astype(np.int64)[:, None])
    return _scatter((b, c, n), (bi, ci, ii), grad_out.astype(f64))


def gather_points_grad(grad_out, idx, n):
    """grad_out (B,C,M), idx (B,M) -> (grad, count, abssum), each (B,C,n)"""
    b, c, m = grad_out.shape
    bi, ci, ii = np.broadcast_arrays(np.arange(b)[:, None, None], np.arange(c)[None, :, None],
                                     idx.astype(np.int64)[:, None])
    return _scatter((b, c, n), (bi, ci, ii), grad_out.astype(f64))


def three_interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B,C,n), idx / weight (B,n,3) -> (grad, count, abssum), each (B,C,m)"""
    b, c, n = grad_out.shape
    terms = grad_out.astype(f64)[..., None] * weight.astype(f64)[:, None]               # (B,C,n,3)
    bi, ci, ii = np.broadcast_arrays(np.arange(b)[:, None, None, None], np.arange(c)[None, :, None, None],
                                     idx.astype(np.int64)[:, None])
    return _scatter((b, c, m), (bi, ci, ii), terms)


def chamfer_backward(xyz1, xyz2, gd1, idx1, gd2, idx2):
    """xyz1 (B,n,3), xyz2 (B,m,3), gd1 / idx1 (B,n), gd2 / idx2 (B,m) -> ((grad_xyz1, count, abssum), (grad_xyz2, ..)).
    A term is 2 g (a - b); an element of grad_xyz1 receives its own term of the first launch and minus the term of every
    point of xyz2 that picked it in the second."""
    x1, x2 = xyz1.astype(f64), xyz2.astype(f64)
    b, n, _ = x1.shape
    m = x2.shape[1]
    rows = np.arange(b)[:, None]
    i1, i2 = idx1.astype(np.int64), idx2.astype(np.int64)
    t1 = 2.0 * gd1.astype(f64)[..., None] * (x1 - x2[rows, i1])                         # (B,n,3): launch 1
    t2 = 2.0 * gd2.astype(f64)[..., None] * (x2 - x1[rows, i2])                         # (B,m,3): launch 2
    own1 = (np.broadcast_to(rows, (b, n)), np.broadcast_to(np.arange(n), (b, n)))
    own2 = (np.broadcast_to(rows, (b, m)), np.broadcast_to(np.arange(m), (b, m)))
    out1 = [np.zeros((b, n, 3), f64), np.zeros((b, n, 3), np.int64), np.zeros((b, n, 3), f64)]
    out2 = [np.zeros((b, m, 3), f64), np.zeros((b, m, 3), np.int64), np.zeros((b, m, 3), f64)]
    for out, where, t in ((out1, own1, t1), (out2, (own1[0], i1), -t1), (out2, own2, t2), (out1, (own2[0], i2), -t2)):
        np.add.at(out[0], where, t)
        np.add.at(out[1], where, 1)
        np.add.at(out[2], where, np.abs(t))
    return tuple(out1), tuple(out2)


def check(got, ref, r, exact=False, copy_exact=False):
    """got: the fp32 result under test; ref: (grad, count, abssum).  Asserts the module's bound (see the docstring), the
    exact zeros, with copy_exact the bit-equal single terms, and with exact the whole array; -> the largest observed
    error divided by the bound (over the elements whose bound is not 0)."""
    grad, count, abssum = ref
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == grad.shape, (got.dtype, got.shape, grad.shape)
    np.testing.assert_array_equal(got[count == 0], 0.0)
    if copy_exact:
        one = count == 1
        np.testing.assert_array_equal(got[one], grad[one].astype(f32))
        np.testing.assert_array_equal(got[one].astype(f64), grad[one])
    if exact:
        np.testing.assert_array_equal(got.astype(f64), grad)
    err = np.abs(got.astype(f64) - grad)
    lim = bound(count, abssum, r)
    bad = ~(err <= lim)                                     # a NaN is outside every bound
    assert not bad.any(), "%d elements outside the bound, worst %g x" % (
        bad.sum(), (err[bad] / np.maximum(lim[bad], 1e-300)).max())
    pos = lim > 0
    return float((err[pos] / lim[pos]).max()) if pos.any() else 0.0


def partial_sum_headroom(ref, q):
    """max |partial sum in any order| / q for terms that are multiples of q, bounded by abssum / q; must be < 2^24"""
    grad, count, abssum = ref
    assert np.array_equal(np.round(grad / q), grad / q) and np.array_equal(np.round(abssum / q), abssum / q)
    return float(abssum.max() / q)


# ---- shapes: the smallest at which each loop bound and tail is exercised ---------------------------------------------
# group_points_grad (b, c, n, m, ns): c around the 8-channel chunk, m * ns = 1, 255, 256, 257, 258, 4096; a pruned
# product -- every value of every axis occurs, with both corners
GROUP_SHAPES = [(1, 1, 1, 1, 1), (3, 17, 300, 64, 64), (1, 7, 5, 51, 5), (3, 8, 300, 16, 16), (1, 9, 300, 257, 1),
                (3, 7, 5, 3, 86), (1, 17, 1, 64, 64), (3, 1, 300, 51, 5), (1, 8, 5, 257, 1), (3, 9, 1, 3, 86)]
# gather_points_grad (b, c, n, npoints): the full product
GATHER_SHAPES = [(b, c, n, m) for m in (1, 255, 256, 257, 600) for c in (1, 3, 9) for n in (1, 300) for b in (1, 3)]
# three_interpolate_grad (b, c, n, m): n gradient columns scattered into m known points; a pruned product
INTERP_SHAPES = [(1, 1, 1, 1), (3, 256, 257, 64), (1, 3, 255, 2), (3, 1, 256, 3), (1, 256, 1, 64), (3, 3, 257, 1),
                 (1, 3, 256, 64), (3, 1, 255, 1), (1, 1, 257, 2), (3, 3, 1, 3), (1, 256, 255, 3), (3, 1, 1, 2)]
# chamfer_backward (b, n, m)
CHAMFER_SHAPES = [(b, n, m) for (n, m) in ((1, 1), (1, 257), (255, 256), (257, 1), (1030, 300)) for b in (1, 3)]

PATTERNS = ("random", "permutation", "all_0", "all_last", "two_valued", "first_half")
INTERP_PATTERNS = PATTERNS + ("iii", "iij")


def make_idx(rng, pattern, shape, n):
    """int32 indices of `shape` into n rows, or None where the pattern makes no sense at this shape (a permutation
    needs no more indices per scene than rows; a first half needs two rows)"""
    b, per = shape[0], int(np.prod(shape[1:]))
    if pattern == "random":
        idx = rng.integers(0, n, shape)
    elif pattern == "permutation":                       # nothing collides
        if per > n:
            return None
        idx = np.stack([rng.permutation(n)[:per] for _ in range(b)]).reshape(shape)
    elif pattern == "all_0":                             # every atomic of a channel meets at one address
        idx = np.zeros(shape)
    elif pattern == "all_last":
        idx = np.full(shape, n - 1)
    elif pattern == "two_valued":
        idx = rng.integers(0, 2, shape) * (n - 1)
    elif pattern == "first_half":                        # the second half must stay exact zeros
        if n < 2:
            return None
        idx = rng.integers(0, n // 2, shape)
    elif pattern in ("iii", "iij"):                      # three_nn's rows for one / two known points
        i, j = rng.integers(0, n, shape[:-1]), rng.integers(0, n, shape[:-1])
        idx = np.stack([i, i, i if pattern == "iii" else j], -1)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(idx, dtype=np.int32)


def make_grad_out(rng, shape, exact):
    if exact:
        return rng.integers(-8, 9, shape).astype(f32)
    return rng.standard_normal(shape).astype(f32)


def make_weight(rng, shape, exact):
    if exact:
        return rng.choice(np.array([0.25, 0.5, 1.0, 2.0], f32), shape)
    return rng.random(shape).astype(f32)


def case_rng(*key):
    return np.random.default_rng([int(k) for k in key])


def group_cases(shape):
    """-> [(label, grad_out, idx, n, exact)] for one shape: every pattern that makes sense, plain and exact"""
    b, c, n, m, ns = shape
    out = []
    for p, pattern in enumerate(PATTERNS):
        for exact in (False, True):
            rng = case_rng(1, b, c, n, m, ns, p, exact)
            idx = make_idx(rng, pattern, (b, m, ns), n)
            if idx is not None:
                out.append(("%s%s" % (pattern, "/exact" if exact else ""), make_grad_out(rng, (b, c, m, ns), exact),
                            idx, n, exact))
    return out


def gather_cases(shape):
    b, c, n, m = shape
    out = []
    for p, pattern in enumerate(PATTERNS):
        for exact in (False, True):
            rng = case_rng(2, b, c, n, m, p, exact)
            idx = make_idx(rng, pattern, (b, m), n)
            if idx is not None:
                out.append(("%s%s" % (pattern, "/exact" if exact else ""), make_grad_out(rng, (b, c, m), exact), idx, n,
                            exact))
    return out


def interp_cases(shape):
    """-> [(label, grad_out (b,c,n), idx (b,n,3), weight (b,n,3), m, exact)]"""
    b, c, n, m = shape
    out = []
    for p, pattern in enumerate(INTERP_PATTERNS):
        for exact in (False, True):
            rng = case_rng(3, b, c, n, m, p, exact)
            idx = make_idx(rng, pattern, (b, n, 3), m)
            if idx is not None:
                out.append(("%s%s" % (pattern, "/exact" if exact else ""), make_grad_out(rng, (b, c, n), exact), idx,
                            make_weight(rng, (b, n, 3), exact), m, exact))
    return out


CHAMFER_KINDS = ("random", "coincident", "clustered")


def chamfer_cases(shape):
    """-> [(label, xyz1 (b,n,3), xyz2 (b,m,3), gd1 (b,n), gd2 (b,m), exact)].  `coincident`: the first point of xyz2 is
    the first point of xyz1 (its terms are exactly 0); `clustered` (only where m >= 40): the first 20 points of xyz2 lie
    among xyz1 and the others far away, so those 20 receive every assignment of xyz1.  The nearest-neighbour indices are
    not made here: they come from the forward pass under test."""
    b, n, m = shape
    out = []
    for k, kind in enumerate(CHAMFER_KINDS):
        if kind == "clustered" and m < 40:
            continue
        for exact in (False, True):
            rng = case_rng(4, b, n, m, k, exact)
            if exact:
                lo, hi = (-8, -3) if kind == "clustered" else (-8, 9)          # multiples of 0.5 in [-4, -2] / [-4, 4]
                x1 = rng.integers(lo, hi, (b, n, 3)) * 0.5
                x2 = rng.integers(lo, hi, (b, m, 3)) * 0.5
                if kind == "clustered":
                    x2[:, 20:] = rng.integers(6, 9, (b, m - 20, 3)) * 0.5       # [3, 4]^3: at least 75 away (squared)
                gd1, gd2 = rng.integers(-8, 9, (b, n)), rng.integers(-8, 9, (b, m))
            else:
                x1, x2 = rng.standard_normal((b, n, 3)), rng.standard_normal((b, m, 3))
                if kind == "clustered":
                    x2[:, 20:] += 100.0
                gd1, gd2 = rng.standard_normal((b, n)), rng.standard_normal((b, m))
            if kind == "coincident":
                x2[:, 0] = x1[:, 0]
            out.append(("%s%s" % (kind, "/exact" if exact else ""), x1.astype(f32), x2.astype(f32), gd1.astype(f32),
                        gd2.astype(f32), exact))
    return out
