"""GPU (-m gpu): exact k nearest neighbours on the device (rfdnet_amd/knn.py, csrc/knn.hip) against the float64
restatement of its rules N1 - N7 (tests/knn_f64.py) on the inputs of tests/knn_cases.py.

Equality means BIT equality of d2 and exact equality of idx with the restatement's brute force over all valid points: both
sides perform the same f64 operations in the same order, and the answer is the k least keys (d2, local row), a total
order, so neither the cells, nor the walk, nor the batch, nor the order inside a cell may show.  Every comparison covers
every query and every slot of its case.  The last test prints the file's tally: the number of float64 values compared, how
many were not bit-equal, and the largest difference in units in the last place."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as C  # noqa: E402
import knn_f64 as N  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY = {'values': 0, 'unequal': 0, 'max_ulp': 0}


def ordered(x):
    """float64 -> int64 that ascends with the value (-0 and +0 apart by one)"""
    i = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i - 1, i)


def unequal(name, got, want):
    """counts the float64 values of `got` that are not bit-equal to `want`, for the file's tally -> that number"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, name
    differ = got.view(np.uint64) != want.view(np.uint64)
    TALLY['values'] += got.size
    TALLY['unequal'] += int(differ.sum())
    if differ.any():
        both = differ & np.isfinite(got) & np.isfinite(want)
        ulp = np.abs(ordered(got[both]).astype(object) - ordered(want[both]).astype(object)) if both.any() else []
        worst = max([int(u) for u in ulp], default=0) if both.sum() == differ.sum() else 2 ** 64
        TALLY['max_ulp'] = max(TALLY['max_ulp'], worst)
        print("%s: %d of %d values not bit-equal, worst %s ulp" % (name, differ.sum(), got.size, worst))
    return int(differ.sum())


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def build(points, pend=None, cells=None):
    from rfdnet_amd.knn import PointSets
    return PointSets(cuda(np.asarray(points, np.float64).reshape(-1, 3)), pend, cells=cells)


def ask(sets, queries, obj=None, k=1, mask=None, **kw):
    n = len(queries)
    d2, idx = sets.query(cuda(queries, np.float64), None if obj is None else cuda(obj, np.int32), k=k,
                         mask=None if mask is None else cuda(mask, np.uint8), **kw)
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32
    assert tuple(d2.shape) == tuple(idx.shape) == (n, k)
    return d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def assert_equal(name, got, want):
    assert np.array_equal(got[1], want[1]), name
    assert unequal(name + " d2", got[0], want[0]) == 0


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SMALL_SIZES)
def test_small_sets_every_k_and_query_count(hip, n):
    pts = C.small_set(n)
    sets = build(pts)
    queries = C.small_queries(max(C.SMALL_QUERIES))
    for k in C.SMALL_K:
        want = N.brute_force(queries, pts, k)
        if k > n:
            assert (want[1][:, n:] == -1).all() and np.isinf(want[0][:, n:]).all() and (want[1][:, :n] >= 0).all()
        for count in C.SMALL_QUERIES:                                   # a prefix of the queries has a prefix of the answers
            got = ask(sets, queries[:count], k=k)
            assert_equal("%d points, k %d, %d queries" % (n, k, count), got, (want[0][:count], want[1][:count]))


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.lattice_queries()))
def test_ties_the_lower_row_wins_and_slots_follow_the_key(hip, name):
    pts = C.lattice()
    queries, ways = C.lattice_queries()[name]
    first = 1 if name == 'point' else 0                                 # a lattice point's own row comes before its tie
    for cells in (1, 3, None):
        sets = build(pts, cells=cells)
        for k in (1, 2, 3, 4, 6, 7, 8, 9, 32):
            want = N.brute_force(queries, pts, k)
            got = ask(sets, queries, k=k)
            assert_equal("lattice %s, k %d, cells %s" % (name, k, cells), got, want)
            tied = slice(first, min(first + ways, k))
            if tied.stop - tied.start >= 2:
                assert (got[0][:, tied] == got[0][:, tied.start:tied.start + 1]).all()      # an exact tie
                assert (np.diff(got[1][:, tied], axis=1) > 0).all()                         # the lower row first
            if first + ways > k > first:                                # the tie is cut: the lowest rows of it are kept
                full = N.brute_force(queries, pts, first + ways)[1]
                assert np.array_equal(got[1], full[:, :k])


def test_forty_one_points_at_one_position(hip):
    pts = C.lattice_with_duplicates()
    queries = np.array([C.DUPLICATE_AT, (2.5, 3., 1.), (0., 0., 0.)])
    want = N.brute_force(queries, pts, 32)
    at = int(np.nonzero((C.lattice() == C.DUPLICATE_AT).all(1))[0][0])
    assert want[1][0].tolist() == [at] + list(range(216, 216 + 31)) and (want[0][0] == 0).all()
    for cells in (1, 4, None):
        assert_equal("duplicates, cells %s" % cells, ask(build(pts, cells=cells), queries, k=32), want)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.frame_sets()))
def test_every_cell_count_gives_the_same_bits(hip, name):
    pts = C.frame_sets()[name]
    queries = C.frame_queries(pts)
    for k in (1, 5):
        want = N.brute_force(queries, pts, k)
        if name == 'empty':
            assert (want[1] == -1).all() and np.isinf(want[0]).all()
        assert np.isinf(want[0][-4:]).all() and (want[1][-4:] == -1).all()      # at 1e300 every d2 overflows: no candidate
        for cells in C.CELLS + (None,):
            sets = build(pts, cells=cells)
            assert sets.res.tolist() == [N.frame_of(pts, cells).R]
            assert_equal("%s, k %d, cells %s" % (name, k, cells), ask(sets, queries, k=k), want)
    hip.device_status()


# 4 -------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_per_set_calls_any_set_order_and_unsorted(hip):
    case = C.ragged_case()
    k = 8
    want = N.Batch(case['points'], case['pend']).query(case['queries'], case['obj'], k)
    sets = build(case['points'], case['pend'])
    assert sets.n_valid.tolist() == list(C.RAGGED_SIZES)
    got = ask(sets, case['queries'], case['obj'], k=k)
    assert_equal("ragged batch", got, want)
    empty = case['obj'] == 0
    assert empty.sum() > 10 and (got[1][empty] == -1).all() and np.isinf(got[0][empty]).all()
    assert (got[1][case['obj'] == 1] == [0] + [-1] * (k - 1)).all()
    for s, pts in enumerate(case['sets']):
        mine = case['obj'] == s
        assert_equal("set %d alone" % s, ask(build(pts), case['queries'][mine], k=k), (got[0][mine], got[1][mine]))
    assert_equal("unsorted launch", ask(sets, case['queries'], case['obj'], k=k, sort_points=False), got)
    other = C.ragged_case(order=[4, 2, 0, 3, 1])
    assert np.array_equal(other['canonical_obj'], case['obj']) and not np.array_equal(other['pend'], case['pend'])
    assert_equal("another set order", ask(build(other['points'], other['pend']), other['queries'], other['obj'], k=k), got)
    d2, idx = sets._query(cuda(case['queries']), cuda(case['obj'], np.int32), k, sorted_copy=False)
    assert_equal("without the cell-ordered copy", (d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)), got)
    offsets_on_device = build(case['points'], cuda(case['pend'], np.int64))
    assert_equal("offsets from the device", ask(offsets_on_device, case['queries'], case['obj'], k=k), got)


# 5 -------------------------------------------------------------------------------------------------------------------
def test_bounds_masks_and_rows_that_are_not_finite(hip):
    pts = C.axis_points()
    origin = np.zeros((1, 3))
    sets = build(pts)
    got = ask(sets, origin, k=4, distance_upper_bound=0.5)               # 0.5 * 0.5 is d2 of rows 2 and 3 exactly: strict
    assert got[1].tolist() == [[0, 1, -1, -1]] and got[0].tolist() == [[0.015625, 0.0625, np.inf, np.inf]]
    assert_equal("bound at a neighbour", got, N.brute_force(origin, pts, 4, limit2=0.25))
    got = ask(sets, origin, k=4, distance_upper_bound=np.nextafter(0.5, 1.))
    assert got[1].tolist() == [[0, 1, 2, 3]]
    got = ask(sets, origin, k=2, distance_upper_bound=0.)
    assert got[1].tolist() == [[-1, -1]] and np.isinf(got[0]).all()
    mask = np.array([1, 0, 1, 0, 0, 0, 0], np.uint8)
    got = ask(sets, origin, k=3, mask=mask)
    assert got[1].tolist() == [[1, 3, 4]]                                 # the neighbours behind a masked row move up
    assert_equal("mask", got, N.brute_force(origin, pts, 3, mask=mask))
    got = ask(sets, origin, k=3, mask=np.ones(7, np.uint8))
    assert got[1].tolist() == [[-1, -1, -1]] and np.isinf(got[0]).all()
    d2, idx = sets.query(cuda(origin), k=3, mask=cuda(mask.astype(bool)))
    assert idx.tolist() == [[1, 3, 4]]
    # data rows that are not finite take no part; queries that are not finite give (NaN, -1); all with a bound and a mask
    bad = C.small_set(33).copy()
    bad[3, 1], bad[20, 0], bad[21] = np.nan, np.inf, -np.inf
    queries = C.small_queries(130).copy()
    queries[4, 2], queries[77, 0], queries[129] = np.nan, np.inf, np.nan
    mask = np.zeros(33, np.uint8)
    mask[[0, 5, 6, 30]] = 1
    for cells in (1, 2, None):
        sets = build(bad, cells=cells)
        assert sets.n_valid.tolist() == [30]
        for k, bound in ((6, None), (6, 0.9), (32, 1.5)):
            want = N.brute_force(queries, bad, k, np.inf if bound is None else bound * bound, mask)
            got = ask(sets, queries, k=k, distance_upper_bound=bound, mask=mask)
            assert_equal("bad rows, k %d, bound %s, cells %s" % (k, bound, cells), got, want)
            assert np.isnan(got[0][[4, 77, 129]]).all() and (got[1][[4, 77, 129]] == -1).all()
            assert not np.isin(got[1], [3, 20, 21, 0, 5, 6, 30]).any()
    with pytest.raises(ValueError):
        sets.query(cuda(queries), distance_upper_bound=-1.)
    with pytest.raises(ValueError):
        sets.query(cuda(queries), k=33)
    with pytest.raises(ValueError):
        sets.query(cuda(queries), k=0)
    with pytest.raises(ValueError):
        sets.query(cuda(queries), mask=cuda(np.zeros(32, np.uint8)))
    with pytest.raises(ValueError):
        sets.query(cuda(queries), cuda(np.ones(len(queries)), np.int32))          # an object outside the batch
    # the kernel's own answer to an object outside the batch (query() refuses it before): (NaN, -1)
    d2, idx = sets._query(cuda(queries[:3]), cuda(np.array([0, 1, -1]), np.int32), 2)
    assert torch.isnan(d2[1:]).all() and (idx[1:] == -1).all() and (idx[0] >= 0).all()


# 6 -------------------------------------------------------------------------------------------------------------------
def test_kdtree_returns_what_pykdtree_returns(hip):
    from rfdnet_amd.knn import KDTree
    data, queries = C.small_set(33), C.small_queries(65)
    tree = KDTree(data)
    assert (tree.n, tree.ndim, tree.leafsize) == (33, 3, 16) and tree.data is tree.data_pts
    want = N.brute_force(queries, data, 5)
    dist, idx = tree.query(queries)
    assert dist.shape == idx.shape == (65,) and dist.dtype == np.float64 and idx.dtype == np.uint32
    assert np.array_equal(idx, want[1][:, 0]) and unequal("KDTree k 1", dist, np.sqrt(want[0][:, 0])) == 0
    dist, idx = tree.query(queries, k=5, sqr_dists=True, eps=0.1)
    assert dist.shape == idx.shape == (65, 5) and np.array_equal(idx, want[1]) and unequal("KDTree k 5", dist, want[0]) == 0
    dist, idx = KDTree(data[:3]).query(queries, k=5)
    assert (idx[:, 3:] == 3).all() and np.isinf(dist[:, 3:]).all() and (idx[:, :3] < 3).all()
    dist, idx = KDTree(C.axis_points()).query(np.zeros((1, 3)), k=4, distance_upper_bound=0.5)
    assert idx.tolist() == [[0, 1, 7, 7]] and dist.tolist() == [[0.125, 0.25, np.inf, np.inf]]
    mask = np.zeros(33, bool)
    mask[want[1][:, 0]] = True
    assert np.array_equal(tree.query(queries, mask=mask)[1], N.brute_force(queries, data, 1, mask=mask)[1][:, 0])
    # the float32 rule: compared in float64, float32(sqrt_f64(d2)) or float32(d2)
    d32, q32 = data.astype(np.float32), queries.astype(np.float32)
    w2, wi = N.brute_force(q32.astype(np.float64), d32.astype(np.float64), 3)
    dist, idx = KDTree(d32).query(q32, k=3)
    assert dist.dtype == np.float32 and np.array_equal(idx, wi) and np.array_equal(dist, np.sqrt(w2).astype(np.float32))
    dist, _ = KDTree(d32).query(q32, k=3, sqr_dists=True)
    assert dist.dtype == np.float32 and np.array_equal(dist, w2.astype(np.float32))
    assert KDTree(data).query(q32)[0].dtype == np.float64
    with pytest.raises(TypeError):
        KDTree(d32).query(queries)
    # one and two dimensions: the missing columns are zeros
    x = np.array([0., 1., 2.5, 4., 10.])
    dist, idx = KDTree(x).query(np.array([2.4, 9.]), k=2)
    assert idx.tolist() == [[2, 1], [4, 3]] and dist.tolist() == [[2.5 - 2.4, 2.4 - 1.], [1., 5.]]
    dist, idx = KDTree(np.array([[0., 0.], [3., 4.], [6., 8.]])).query(np.zeros((1, 2)), k=3)
    assert idx.tolist() == [[0, 1, 2]] and dist.tolist() == [[0., 5., 10.]]


# 7 -------------------------------------------------------------------------------------------------------------------
def test_the_two_helpers_of_the_reference(hip):
    from rfdnet_amd.knn import chamfer_distance_kdtree, get_nearest_neighbors_indices_batch
    B, T = 3, 257
    rng = np.random.default_rng(31)
    p1, p2 = rng.uniform(-1., 1., (B, T, 3)), rng.uniform(-1., 1., (B, T, 3)) + [0.1, 0., 0.]
    want12 = [N.brute_force(p1[b], p2[b], 3) for b in range(B)]
    want21 = [N.brute_force(p2[b], p1[b], 1) for b in range(B)]
    indices, distances = get_nearest_neighbors_indices_batch(p1, p2)
    assert len(indices) == len(distances) == B
    for b in range(B):
        assert indices[b].shape == distances[b].shape == (T,) and indices[b].dtype == np.uint32
        assert np.array_equal(indices[b], want12[b][1][:, 0])
        assert unequal("nearest of pair %d" % b, distances[b], np.sqrt(want12[b][0][:, 0])) == 0
    indices, distances = get_nearest_neighbors_indices_batch(p1, p2, k=3)
    for b in range(B):
        assert indices[b].shape == (T, 3) and np.array_equal(indices[b], want12[b][1])
        assert unequal("3 nearest of pair %d" % b, distances[b], np.sqrt(want12[b][0])) == 0
    t1, t2 = torch.from_numpy(p1), torch.from_numpy(p2)
    i12 = torch.from_numpy(np.stack([w[1][:, 0] for w in want12]))
    i21 = torch.from_numpy(np.stack([w[1][:, 0] for w in want21]))
    c1 = (t1 - torch.gather(t2, 1, i12.view(B, -1, 1).expand_as(t1))).pow(2).sum(2).mean(1)      # the same expression in
    c2 = (t2 - torch.gather(t1, 1, i21.view(B, -1, 1).expand_as(t2))).pow(2).sum(2).mean(1)      # torch on the CPU
    # all terms are non-negative, so any summation order is within (T - 1) u of the exact sum: twice that between two
    tol = 2 * (T - 1) * 2. ** -53
    chamfer = chamfer_distance_kdtree(t1.cuda(), t2.cuda())
    assert chamfer.is_cuda and chamfer.dtype == torch.float64 and tuple(chamfer.shape) == (B,)
    print("chamfer: device", chamfer.tolist(), "cpu", (c1 + c2).tolist())
    assert (torch.abs(chamfer.cpu() - (c1 + c2)) <= tol * (c1 + c2)).all()
    g1, g2, g12, g21 = chamfer_distance_kdtree(t1.cuda(), t2.cuda(), give_id=True)
    assert tuple(g1.shape) == tuple(g2.shape) == (B,) and tuple(g12.shape) == tuple(g21.shape) == (B, T)
    assert g12.dtype == torch.int64 and g21.dtype == torch.int64
    assert torch.equal(g12.cpu(), i12) and torch.equal(g21.cpu(), i21)
    assert (torch.abs(g1.cpu() - c1) <= tol * c1).all() and (torch.abs(g2.cpu() - c2) <= tol * c2).all()


# 8 -------------------------------------------------------------------------------------------------------------------
def metric_sets():
    """A: two predictions (a shifted cube of 257 samples, a sphere of 1 000); B: their ground truth and an empty set"""
    a0, na0 = C.cube_samples(257, 41, shift=0.03)
    a1, na1 = C.sphere_samples(1000, 42, radius=0.52)
    b0, nb0 = C.cube_samples(1000, 43)
    b1, nb1 = C.sphere_samples(257, 44)
    A = (np.concatenate([a0, a1]), np.concatenate([na0, na1]), np.array([0, 257, 1257]))
    B = (np.concatenate([b0, b1]), np.concatenate([nb0, nb1]), np.array([0, 1000, 1257, 1257]))
    return A, B


def one_way_f64(src, src_set, tgt, tgt_set, tau):
    """the N7 restatement of one direction of one pair -> sums (3), counts (1 + T), the number of source points"""
    (ps, ns, es), (pt, nt, et) = src, tgt
    rows = slice(es[src_set], es[src_set + 1])
    q = ps[rows]
    d2, idx = N.Batch(pt, et).query(q, np.full(len(q), tgt_set), 1)
    sums, counts = N.sums([0, len(q)], d2[:, 0], idx[:, 0], np.full(len(q), tgt_set), et, ns[rows], nt, tau)
    return sums[0], counts[0], len(q)


def test_pointcloud_metrics_equal_the_restated_sums(hip):
    from rfdnet_amd.knn import PointSets, pointcloud_metrics, segment_sums
    A, B = metric_sets()
    tau = (0.05, 0.10)
    pairs = [[0, 0], [1, 1], [0, 2]]
    SA, SB = build(A[0], A[2]), build(B[0], B[2])
    m = pointcloud_metrics(SA, SB, pairs, cuda(A[1]), cuda(B[1]), tau)
    from rfdnet_amd.iscnet import mesh_eval
    assert set(m) == set(mesh_eval.METRIC_KEYS)
    assert all(v.dtype == torch.float64 and v.is_cuda and v.shape[0] == 3 for v in m.values())
    # the device's sums and counts themselves, bit for bit
    for p, (a, b) in enumerate(pairs[:2]):
        for src, s_set, tgt, t_set, s_dev, t_dev, ns_dev, nt_dev in ((A, a, B, b, SA, SB, A[1], B[1]),
                                                                     (B, b, A, a, SB, SA, B[1], A[1])):
            want_sums, want_counts, n = one_way_f64(src, s_set, tgt, t_set, tau)
            rows = slice(src[2][s_set], src[2][s_set + 1])
            obj = torch.full((n,), t_set, dtype=torch.int32, device="cuda")
            d2, idx = t_dev.query(s_dev.points[rows], obj, k=2)                          # slot 0 of a (n,2) result
            sums, counts = segment_sums(t_dev, cuda(np.array([0, n]), np.int32), d2, idx, obj, cuda(ns_dev[rows]),
                                        cuda(nt_dev), tau)
            assert np.array_equal(counts.cpu().numpy()[0], want_counts) and want_counts[0] == 0
            assert unequal("sums of pair %d" % p, sums.cpu().numpy()[0], want_sums) == 0
    # the dictionary from the restated sums, in the same float64 arithmetic
    for p, (a, b) in enumerate(pairs[:2]):
        s_ab, c_ab, n_a = one_way_f64(A, a, B, b, tau)
        s_ba, c_ba, n_b = one_way_f64(B, b, A, a, tau)
        want = {'accuracy': s_ab[0] / n_a, 'completeness': s_ba[0] / n_b,
                'chamfer_l1': (s_ab[0] / n_a + s_ba[0] / n_b) / 2, 'chamfer_sq': (s_ab[1] / n_a + s_ba[1] / n_b) / 2,
                'normal_consistency': (s_ab[2] / n_a + s_ba[2] / n_b) / 2,
                'rms': np.sqrt((s_ab[1] + s_ba[1]) / (n_a + n_b))}
        for key, value in want.items():
            assert unequal("%s of pair %d" % (key, p), m[key][p:p + 1].cpu().numpy(), np.array([value])) == 0
        assert m['precision'][p].tolist() == (c_ab[1:] / n_a).tolist() and m['recall'][p].tolist() == (c_ba[1:] / n_b).tolist()
    assert 0 < float(m['accuracy'][0]) < 0.1 and 0.0199 < float(m['accuracy'][1]) < 0.1        # radii 0.52 and 0.5
    assert float(m['normal_consistency'][1]) > 0.9
    for key, value in m.items():                                        # an empty target: NaN means
        assert torch.isnan(value[2]).all(), key
    plain = pointcloud_metrics(SA, SB, pairs[:2], thresholds=tau)
    assert (plain['normal_consistency'] == 0).all() and torch.equal(plain['chamfer_l1'], m['chamfer_l1'][:2])
    with pytest.raises(ValueError):
        pointcloud_metrics(SA, SB, [[0, 3]])
    with pytest.raises(ValueError):
        pointcloud_metrics(SA, SB, pairs, thresholds=range(9))
    assert isinstance(SA, PointSets) and hip.stream_status_bits() == 0


def test_pointcloud_distance_tool_end_to_end(hip, tmp_path):
    from rfdnet_amd import io
    v = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                  [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    mesh, cloud = str(tmp_path / "cube.off"), str(tmp_path / "pointcloud.npz")
    io.write_off(mesh, v, f)
    points, normals = C.cube_samples(3000, 51)
    io.write_pointcloud_npz(cloud, points, normals, np.zeros(3), 1.)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pointcloud_distance.py"), mesh, cloud, "--samples",
                          "2000", "--thresholds", "0.05", "0.1", "--seed", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["tool"] == "pointcloud_distance" and r["samples"] == 2000 and r["points"] == 3000
    assert 0 < r["chamfer_l1"] < 0.05 and r["fscore"]["0.1"] > 0.99 and r["normal_consistency"] > 0.9
    assert set(r["precision"]) == {"0.05", "0.1"}


# 9 -------------------------------------------------------------------------------------------------------------------
def test_twenty_thousand_points_against_the_brute_force(hip):
    data, queries = C.large_case()
    want = N.brute_force(queries, data, 8)
    sets = build(data)
    assert sets.res.tolist() == [14]
    assert_equal("20 000 points, k 8", ask(sets, queries, k=8), want)
    hip.device_status()


# 10 ------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from rfdnet_amd.knn import PointSets
    lib = hip.lib()
    inf = float("inf")
    assert lib.rfd_knn_points(-1, 1, *[None] * 9, None) != 0
    assert lib.rfd_knn_points(1, 0, *[None] * 9, None) != 0
    assert lib.rfd_knn_points(1, 1, *[None] * 9, None) != 0                                   # null pointers
    assert lib.rfd_knn_cells(-1, None, 1, None, None, 0, None, None, None) != 0
    assert lib.rfd_knn_cells(1, None, 1, None, None, 0, None, None, None) != 0
    assert lib.rfd_knn_query(-1, None, None, 1, inf, None, 1, 1, *[None] * 11, 1, None, None, None, None) != 0
    assert lib.rfd_knn_query(1, None, None, 0, inf, None, 1, 1, *[None] * 11, 1, None, None, None, None) != 0
    assert lib.rfd_knn_query(1, None, None, 33, inf, None, 1, 1, *[None] * 11, 1, None, None, None, None) != 0
    assert lib.rfd_knn_query(1, None, None, 1, float("nan"), None, 1, 1, *[None] * 11, 1, None, None, None, None) != 0
    assert lib.rfd_knn_query(1, None, None, 1, inf, None, 1, 1, *[None] * 11, 1, None, None, None, None) != 0
    assert lib.rfd_knn_sums(-1, 0, 1, *[None] * 4, 0, 0, *[None] * 3, 0, *[None] * 3, None) != 0
    assert lib.rfd_knn_sums(1, 0, 0, *[None] * 4, 0, 0, *[None] * 3, 0, *[None] * 3, None) != 0          # stride 0
    assert lib.rfd_knn_sums(1, 0, 1, *[None] * 4, 0, 0, *[None] * 3, 9, *[None] * 3, None) != 0          # 9 thresholds
    assert b"rfd_knn_sums" in lib.rfd_last_error_string()
    pts = cuda(C.small_set(7))
    for cells in (0, 65):
        with pytest.raises(ValueError, match="cells"):
            PointSets(pts, cells=cells)
    for bad in ([0, 8], [0, 5, 3, 7], [1, 7], [0, 3]):
        with pytest.raises(ValueError):
            PointSets(pts, bad)
    with pytest.raises(TypeError):
        PointSets(pts.half())
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PointSets(pts.cpu())
    with pytest.raises(ValueError):
        PointSets(pts, [0, 3, 7]).query(pts)                                                 # two sets need `obj`
    assert hip.stream_status_bits() == 0


# the tally -----------------------------------------------------------------------------------------------------------
def test_report_the_tally_of_the_file(hip):
    print("knn: %d float64 values compared with the restatement, %d not bit-equal, largest difference %d ulp"
          % (TALLY['values'], TALLY['unequal'], TALLY['max_ulp']))
    assert TALLY['values'] > 0 and TALLY['unequal'] == 0 and TALLY['max_ulp'] == 0
