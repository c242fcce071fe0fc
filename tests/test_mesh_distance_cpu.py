"""CPU: the float64 restatement of the mesh-distance rules (tests/mesh_dist_f64.py, include/rfd_mesh_dist.h) against
closest points written down by hand, its shell walk against its own brute force bit for bit, its region walk against the
per-point numpy loop of tests/simplify_cases.py, and the host module's refusal of CPU tensors.  The kernels are compared
with the same restatement in tests/test_gpu_mesh_distance.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_dist_cases as M  # noqa: E402
import mesh_dist_f64 as D  # noqa: E402
import simplify_cases as C  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same(a, b):
    """bit equality of two float64 arrays (a NaN equals a NaN of the same bits)"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_the_seven_regions_of_one_triangle_and_their_boundaries():
    v, f = M.TRIANGLE
    tri = v[f]
    for p, want, region in M.REGIONS:
        p, want = np.array(p), np.array(want)
        q, d2 = D.closest_points(p, tri)
        assert np.array_equal(q[0], want), region
        assert d2[0] == ((p - want) ** 2).sum(), region
        best = D.brute_force(p, tri, np.array([True]))
        assert best[0] == d2[0] and best[1] == 0 and np.array_equal(best[2], want), region


def test_a_face_without_area_takes_no_part_where_the_region_walk_alone_divides_zero_by_zero():
    tri = np.array([[[0., 0., 0.], [0., 0., 0.], [1., 0., 0.]]])
    p = np.array([0.5, 1., 0.])
    with np.errstate(all='ignore'):
        assert np.isnan(C.point_triangle_distance(p[None], tri)[0])              # what rule D1 is for
    v, f = M.ZERO_AREA
    _, valid, _ = D.triangles(v, f, [0, len(v)], [0, len(f)])
    assert not valid.any()
    b = D.Batch(v, f, [0, len(v)], [0, len(f)])
    d2, face, q = b.query(p[None], [0])
    assert d2[0] == np.inf and face[0] == -1 and np.isnan(q).all()
    v, f = M.OBJECTS['bad_mesh']
    _, valid, _ = D.triangles(v, f, [0, len(v)], [0, len(f)])
    assert valid.tolist() == [True, False, True, False, False, True, False, False, True]


@pytest.mark.parametrize("cells", M.WALK_CELLS)
def test_the_walk_equals_the_brute_force_bit_for_bit(cells):
    case = M.ragged_case()
    want = case['brute']
    got = M.restated_batch(cells).query(case['points'], case['obj'])
    assert np.array_equal(got[1], want[1])
    assert same(got[0], want[0]) and same(got[2], want[2])
    # rule D5 for the object without faces and for the query with a NaN
    empty = case['obj'] == M.NAMES.index('empty')
    nan = ~np.isfinite(case['points']).all(1)
    assert nan.sum() == len(M.NAMES)
    assert (got[1][empty | nan] == -1).all() and np.isnan(got[0][nan]).all() and (got[0][empty & ~nan] == np.inf).all()
    assert (got[1][~(empty | nan)] >= 0).all()


@pytest.mark.parametrize("name", list(M.TIES))
@pytest.mark.parametrize("cells", (1, 2, 5))
def test_the_lowest_face_row_wins_a_tie(name, cells):
    (v, f), points, rows = M.TIES[name]
    b = D.Batch(v, f, [0, len(v)], [0, len(f)], cells=cells)
    obj = np.zeros(len(points), np.int64)
    d2, face, q = b.query(points, obj)
    bd2, bface, bq = b.query(points, obj, brute=True)
    assert np.array_equal(face, bface) and same(d2, bd2) and same(q, bq)
    for i, p in enumerate(points):
        _, every = D.closest_points(p, b.tri)
        tied = np.nonzero(every == every.min())[0]
        assert len(tied) >= 2 and face[i] == tied.min(), (name, i)
    if rows is not None:
        assert face.tolist() == rows


def test_the_far_queries_are_pruned_and_the_walk_never_passes_the_frame():
    case = M.ragged_case()
    b = M.restated_batch(7)
    k = M.NAMES.index('icosphere1280')
    inside = np.nonzero(case['obj'] == k)[0][:12]
    shells = [D.walk(case['points'][i], b.tri[b.tend[k]:b.tend[k + 1]], b.frames[k], b.lists[k])[1] for i in inside]
    assert max(shells) <= 7 and min(shells) < 7                                   # bounded, and the bound does stop walks


@pytest.mark.parametrize("name", ('icosphere320', 'icosphere1280'))
def test_the_region_walk_agrees_with_the_per_point_loop_on_the_noisy_icospheres(name):
    v, f = M.OBJECTS[name]
    points = M.object_queries(name, 3)
    points = points[np.isfinite(points).all(1)]
    b = D.Batch(v, f, [0, len(v)], [0, len(f)])
    d2 = b.query(points, np.zeros(len(points), np.int64), brute=True)[0]
    want = C.point_triangle_distance(points, np.asarray(v)[np.asarray(f)])
    assert np.array_equal(np.sqrt(d2), want)            # the same operations in the same order: equal, not merely close


def test_the_sum_tree_has_the_fixed_shape():
    x = np.random.default_rng(0).uniform(0, 1, 200)
    keep = np.ones(200, bool)
    keep[[3, 64, 199]] = False
    part = [sum(x[e] for e in range(j, 200, 64) if keep[e]) for j in range(64)]
    for w in (32, 16, 8, 4, 2, 1):
        part = [part[j] + part[j + w] for j in range(w)]
    assert D.tree_sum(x, keep) == part[0]
    assert D.tree_sum(x[:0], keep[:0]) == 0.


def test_two_parallel_squares_are_a_quarter_apart_everywhere():
    (va, fa), (vb, fb) = M.squares()
    v, f, vend, tend = C.batch([(va, fa), (vb, fb)])
    b = D.Batch(v, f, vend, tend)
    u = np.random.default_rng(5).uniform(0, 1, (2, 1000, 3))
    points, face, normals = D.sample(b.tri, b.tend, D.area_prefix(b.tri, b.valid, b.tend), u)
    d2 = b.query(points.reshape(-1, 3), np.repeat([1, 0], 1000), brute=True)[0]
    assert (np.sqrt(d2) == 0.25).all()
    assert (np.abs(normals[..., 2]) == 1).all()


def test_point_mesh_distance_refuses_cpu_tensors():
    from rfdnet_amd.mesh_distance import MeshDistance, point_mesh_distance
    v, f = M.TRIANGLE
    with pytest.raises(RuntimeError, match="CPU not supported"):
        point_mesh_distance(torch.from_numpy(v), torch.from_numpy(f), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        MeshDistance(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError, match="cells"):
        MeshDistance(torch.from_numpy(v), torch.from_numpy(f), cells=65)
