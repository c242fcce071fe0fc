"""CPU: the float64 restatement of the k-nearest-neighbour rules (tests/knn_f64.py) against itself (the shell walk equals
the brute force at every cell count) and against scipy's cKDTree; the argument checks and return shapes of
rfdnet_amd.knn.KDTree with the device call stubbed; read_pointcloud_npz against write_pointcloud_npz."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as C  # noqa: E402
import knn_f64 as N  # noqa: E402


def same(a, b):
    """bit equality of two float64 arrays (NaN equals NaN, -0 differs from +0)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def walk_cases():
    """-> [(name, points, pend, queries, obj, k, limit2, mask)]: every input of tests/knn_cases.py, thinned where the
    per-query walk in Python would take long"""
    out = []
    for n in C.SMALL_SIZES:
        for k in (1, 4, 9, 32):
            out.append(("small %d k %d" % (n, k), C.small_set(n), None, C.small_queries(40), None, k, np.inf, None))
    for name, (q, _) in C.lattice_queries().items():
        out.append(("lattice " + name, C.lattice(), None, q, None, 9, np.inf, None))
    out.append(("duplicates", C.lattice_with_duplicates(), None, np.array([C.DUPLICATE_AT, (2.5, 3., 1.)]), None, 32,
                np.inf, None))
    for name, pts in C.frame_sets().items():
        out.append(("frame " + name, pts, None, C.frame_queries(pts), None, 5, np.inf, None))
    rc = C.ragged_case()
    out.append(("ragged", rc['points'], rc['pend'], rc['queries'][:120], rc['obj'][:120], 8, np.inf, None))
    bad = C.small_set(33).copy()
    bad[3, 1], bad[20, 0] = np.nan, np.inf
    mask = np.zeros(33, np.uint8)
    mask[[0, 5, 6, 30]] = 1
    q = C.small_queries(30).copy()
    q[4, 2] = np.nan
    out.append(("bound, mask, NaN rows", bad, None, q, None, 6, 0.9 ** 2, mask))
    out.append(("axis, strict bound", C.axis_points(), None, np.zeros((1, 3)), None, 4, 0.25, None))
    return out


@pytest.mark.parametrize("cells", C.CELLS)
def test_the_walk_equals_the_brute_force_at_every_cell_count(cells):
    for name, pts, pend, q, obj, k, limit2, mask in walk_cases():
        b = N.Batch(pts, pend, cells=cells)
        want = b.query(q, obj, k, limit2, mask, brute=True)
        got = b.query(q, obj, k, limit2, mask, brute=False)
        assert np.array_equal(got[1], want[1]), name
        assert same(got[0], want[0]), name


def test_the_brute_force_on_cases_written_down_by_hand():
    d2, idx = N.brute_force(np.zeros((1, 3)), C.axis_points(), 8)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, 5, 6, -1]                              # the tie at 0.5: the lower row first
    assert d2[0].tolist() == [0.015625, 0.0625, 0.25, 0.25, 1., 4., 16., np.inf]
    d2, idx = N.brute_force(np.zeros((1, 3)), C.axis_points(), 4, limit2=0.25)       # strict: neither 0.5 is within 0.5
    assert idx[0].tolist() == [0, 1, -1, -1] and d2[0].tolist() == [0.015625, 0.0625, np.inf, np.inf]
    d2, idx = N.brute_force(np.zeros((1, 3)), C.axis_points(), 2, limit2=0.)
    assert idx[0].tolist() == [-1, -1]
    mask = np.array([1, 0, 1, 0, 0, 0, 0])
    assert N.brute_force(np.zeros((1, 3)), C.axis_points(), 3, mask=mask)[1][0].tolist() == [1, 3, 4]
    assert N.brute_force(np.zeros((1, 3)), C.axis_points(), 3, mask=np.ones(7))[1][0].tolist() == [-1, -1, -1]
    d2, idx = N.brute_force(np.array([[np.nan, 0., 0.]]), C.axis_points(), 2)
    assert np.isnan(d2).all() and idx[0].tolist() == [-1, -1]
    for name, (q, ways) in C.lattice_queries().items():
        k = ways + 1 if name == 'point' else ways
        d2, idx = N.brute_force(q, C.lattice(), k + 1)
        tied = d2[:, k - ways:k]
        assert (tied == tied[:, :1]).all() and (d2[:, k] > d2[:, k - 1]).all(), name
        assert (np.diff(idx[:, k - ways:k], axis=1) > 0).all(), name                 # among equals the rows ascend


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_the_restatement_agrees_with_ckdtree(dtype):
    from scipy.spatial import cKDTree
    data, queries = C.large_case(dtype)
    data, queries = data.astype(np.float64), queries.astype(np.float64)             # float32 inputs upcast, which is exact
    k = 32
    d2, idx = N.brute_force(queries, data, k + 1)
    ties = (np.diff(d2, axis=1) == 0).any(1)
    assert ties.sum() == 0                                                           # no query is left out below
    dist, index = cKDTree(data).query(queries, k=k)
    assert np.array_equal(idx[:, :k], index)
    assert same(np.sqrt(d2[:, :k]), dist)


def test_the_sums_on_a_case_written_down_by_hand():
    pend = [0, 2, 5]
    seg = [0, 3, 3, 7]
    d2 = np.array([0.25, 1., np.inf, 4., np.nan, 0.0625, 9.])
    row = np.array([0, 1, -1, 2, 0, 3, 1])
    qobj = np.array([0, 0, 0, 1, 1, 1, 1])
    n_s = np.tile([0., 0., 1.], (7, 1))
    n_t = np.array([[0., 0., 1.], [0., 0., -0.5], [1., 0., 0.], [0., 0., 1.], [0., 0., 0.25]])
    sums, counts = N.sums(seg, d2, row, qobj, pend, n_s, n_t, [1., 2.])
    assert sums[0].tolist() == [1.5, 1.25, 1.5] and counts[0].tolist() == [1, 2, 2]
    assert sums[1].tolist() == [0., 0., 0.] and counts[1].tolist() == [0, 0, 0]
    # object 1 owns three rows: local row 3 is outside it and left out with the NaN
    assert sums[2].tolist() == [5., 13., 1.25] and counts[2].tolist() == [2, 0, 1]
    plain, _ = N.sums(seg, d2, row, qobj, pend, None, n_t, [])
    assert plain[:, 2].tolist() == [0., 0., 0.] and plain[:, :2].tolist() == sums[:, :2].tolist()


# the KDTree wrapper, the device call stubbed ---------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    from rfdnet_amd import knn

    def search(data, queries, k, bound, mask):
        assert data.dtype == np.float64 and queries.dtype == np.float64 and data.shape[1] == 3 and queries.shape[1] == 3
        assert mask is None or (mask.dtype == np.uint8 and mask.shape == (len(data),))
        return N.brute_force(queries, data, k, np.inf if bound is None else float(bound) * float(bound), mask)
    monkeypatch.setattr(knn, "_device_search", search)
    return knn


def test_kdtree_refuses_what_pykdtree_refuses(stubbed):
    KDTree = stubbed.KDTree
    data = C.small_set(33)
    tree = KDTree(data)
    q = C.small_queries(5)
    with pytest.raises(ValueError, match="leafsize"):
        KDTree(data, leafsize=0)
    with pytest.raises(ValueError, match="1 to 3 dimensions"):
        KDTree(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="neighbours"):
        tree.query(q, k=0)
    with pytest.raises(ValueError, match="eps"):
        tree.query(q, eps=-1)
    with pytest.raises(ValueError, match="distance_upper_bound"):
        tree.query(q, distance_upper_bound=-0.5)
    with pytest.raises(ValueError, match="Mask"):
        tree.query(q, mask=np.zeros(32, bool))
    with pytest.raises(ValueError, match="same dimensions"):
        tree.query(q[:, :2])
    with pytest.raises(ValueError, match="same dimensions"):
        tree.query(q[:, 0])
    with pytest.raises(TypeError, match="float32"):
        KDTree(data.astype(np.float32)).query(q)
    with pytest.raises(ValueError, match="neighbours"):
        tree.query(q, k=33)


def test_kdtree_has_pykdtrees_attributes_shapes_and_types(stubbed):
    KDTree = stubbed.KDTree
    data = C.small_set(7)
    tree = KDTree(data, leafsize=4)
    assert (tree.n, tree.ndim, tree.leafsize) == (7, 3, 4)
    assert tree.data_pts.shape == (21,) and tree.data_pts.dtype == np.float64 and tree.data is tree.data_pts
    q = C.small_queries(11)
    want_d2, want_i = N.brute_force(q, data, 9)
    dist, idx = tree.query(q)
    assert dist.shape == idx.shape == (11,) and dist.dtype == np.float64 and idx.dtype == np.uint32
    assert np.array_equal(idx, want_i[:, 0]) and same(dist, np.sqrt(want_d2[:, 0]))
    dist, idx = tree.query(q, k=9, eps=0.5, sqr_dists=True)
    assert dist.shape == idx.shape == (11, 9) and idx.dtype == np.uint32
    assert (idx[:, 7:] == 7).all() and np.isinf(dist[:, 7:]).all()                   # k > n: n and inf for missing
    assert np.array_equal(idx[:, :7], want_i[:, :7]) and same(dist, want_d2)
    dist, idx = KDTree(C.axis_points()).query(np.zeros((1, 3)), k=4, distance_upper_bound=0.5)
    assert idx.tolist() == [[0, 1, 7, 7]] and dist.tolist() == [[0.125, 0.25, np.inf, np.inf]]      # strict at 0.5
    mask = np.zeros(7, bool)
    mask[want_i[:, 0]] = True
    assert not np.isin(tree.query(q, mask=mask)[1], want_i[:, 0]).any()
    # float32 data and queries: float32 distances, rounded from the float64 ones; float64 queries of a float64 tree only
    d32, q32 = data.astype(np.float32), q.astype(np.float32)
    w2, wi = N.brute_force(q32.astype(np.float64), d32.astype(np.float64), 2)
    dist, idx = KDTree(d32).query(q32, k=2)
    assert dist.dtype == np.float32 and np.array_equal(idx, wi)
    assert np.array_equal(dist, np.sqrt(w2).astype(np.float32))
    dist, _ = KDTree(d32).query(q32, k=2, sqr_dists=True)
    assert dist.dtype == np.float32 and np.array_equal(dist, w2.astype(np.float32))
    assert KDTree(data).query(q32)[0].dtype == np.float64
    assert KDTree(d32).data_pts.dtype == np.float32
    assert KDTree(np.arange(5)).data_pts.dtype == np.float64                         # integers become float64


def test_kdtree_serves_one_and_two_dimensions(stubbed):
    KDTree = stubbed.KDTree
    x = np.array([0., 1., 2.5, 4., 10.])
    tree = KDTree(x)
    assert (tree.n, tree.ndim) == (5, 1)
    dist, idx = tree.query(np.array([2.4, 9.]), k=2)
    assert idx.tolist() == [[2, 1], [4, 3]] and same(dist, np.array([[2.5 - 2.4, 2.4 - 1.], [1., 5.]]))
    xy = np.array([[0., 0.], [3., 4.], [6., 8.]])
    tree = KDTree(xy)
    assert (tree.n, tree.ndim) == (3, 2) and tree.data_pts.shape == (6,)
    dist, idx = tree.query(np.zeros((1, 2)), k=3)
    assert idx.tolist() == [[0, 1, 2]] and dist.tolist() == [[0., 5., 10.]]


def test_read_pointcloud_npz_round_trips(tmp_path):
    from rfdnet_amd import io
    points, normals = C.sphere_samples(50, 3)
    loc, scale = np.array([0.5, -1.25, 3.]), 2.5
    for float16 in (False, True):
        path = str(tmp_path / ("pc_%d.npz" % float16))
        io.write_pointcloud_npz(path, points, normals, loc, scale, float16=float16)
        stored = np.float16 if float16 else np.float32
        p, n, l, s = io.read_pointcloud_npz(path)
        assert p.dtype == n.dtype == np.float32 and l.dtype == np.float64 and isinstance(s, float)
        assert np.array_equal(p, points.astype(stored).astype(np.float32))
        assert np.array_equal(n, normals.astype(stored).astype(np.float32))
        assert np.array_equal(l, loc) and s == scale
        world = io.read_pointcloud_npz(path, original_frame=True)[0]
        assert world.dtype == np.float64 and np.array_equal(world, p.astype(np.float64) * scale + loc)
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, points=points)
    with pytest.raises(ValueError, match="normals"):
        io.read_pointcloud_npz(bad)
