"""CPU: the numpy float64 restatement of the mesh decimation (tests/decimate_f64.py) against hand-computed cases and the
invariants of the five rules (include/rfd_decimate.h), and the guards of rfdnet_amd.iscnet.decimate that need no GPU.
The kernels are compared with the same restatement in tests/test_gpu_decimate.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases as cases  # noqa: E402
import decimate_f64 as D  # noqa: E402

F32_EPS = 2.0 ** -23


# ------------------------------------------------------------------------------------------------- hand-computed ----
def test_a_cube_in_one_cell_collapses_to_nothing():
    v, f = cases.unit_cube()
    out = D.decimate(v, f, [0, 8], [0, 12], 1, lo=np.zeros((1, 3)), h=np.ones(1))
    assert out['v'].shape == (0, 3) and out['f'].shape == (0, 3)
    assert out['vend'] == [0, 0] and out['tend'] == [0, 0]


def test_a_cube_with_one_vertex_per_cell_comes_back_as_itself():
    v, f = cases.unit_cube()
    out = D.decimate(v, f, [0, 8], [0, 12], 2, lo=np.zeros((1, 3)), h=np.full(1, 0.5))
    # vertex i sits in cell (i & 1, (i >> 1) & 1, i >> 2), whose key is i: the candidates are the vertices in their order
    assert out['vend'] == [0, 8] and out['tend'] == [0, 12]
    assert out['key'].tolist() == list(range(8))
    assert np.array_equal(out['f'], f)
    assert out['corners'].tolist() == [np.count_nonzero(f == i) for i in range(8)]
    # three orthogonal planes meet in a corner: the quadric's minimum is the corner itself, which is also the weighted
    # mean of the cell's one vertex, so the regularisation does not move it
    assert np.abs(out['v'].astype(np.float64) - v).max() <= 4 * F32_EPS
    assert (np.abs(out['v'] - out['centre']) <= 0.25 * (1 + 4 * F32_EPS)).all()


def test_cell_index_on_a_boundary_outside_the_cube_and_not_finite():
    x = np.array([[0.5, 1.0, 1.5], [-3.0, 0.0, 7.0], [2.0, 1e300, -1e300], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1]])
    ijk, has = D.vertex_cells(x, np.zeros(3), 0.5, 4)
    assert ijk[:3].tolist() == [[1, 2, 3], [0, 0, 3], [3, 3, 0]]       # a boundary belongs to the upper cell; edge cells
    assert has.tolist() == [True, True, True, False, False]


def test_tree_sum_has_the_written_shape():
    rng = np.random.default_rng(0)
    for n in (0, 1, 15, 16, 17, 33):
        t = rng.normal(0, 1, (n, 13)) * 10.0 ** rng.integers(-8, 8, (n, 1))
        part = [np.zeros(13) for _ in range(16)]
        for i in range(n):
            part[i % 16] = part[i % 16] + t[i]
        want = (((part[0] + part[8]) + (part[4] + part[12])) + ((part[2] + part[10]) + (part[6] + part[14]))) + \
               (((part[1] + part[9]) + (part[5] + part[13])) + ((part[3] + part[11]) + (part[7] + part[15])))
        assert np.array_equal(D.tree_sum(list(t)), want), n


def test_a_large_regularisation_gives_the_weighted_mean():
    v, f = cases.fan(7)
    big = D.decimate(v, f, [0, len(v)], [0, len(f)], 2, lo=np.full((1, 3), -2.0), h=np.full(1, 2.0), regularise=1e9)
    out = D.decimate(v, f, [0, len(v)], [0, len(f)], 2, lo=np.full((1, 3), -2.0), h=np.full(1, 2.0))
    assert big['tend'] == out['tend'] and np.array_equal(big['f'], out['f'])
    x = v.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]]), axis=1)
    ijk, _ = D.vertex_cells(x, np.full(3, -2.0), 2.0, 2)
    key = (ijk[:, 2] * 2 + ijk[:, 1]) * 2 + ijk[:, 0]
    for row, k in enumerate(big['key']):
        num, den = np.zeros(3), 0.0
        for j in range(len(f)):
            for c in range(3):
                if key[f[j, c]] == k:
                    num, den = num + area[j] * x[f[j, c]], den + area[j]
        assert np.abs(big['v'][row] - num / den).max() <= 1e-6


# ----------------------------------------------------------------------------------------------------- invariants ----
@pytest.mark.parametrize("cells", [4, 7])
def test_a_closed_sphere_keeps_even_edge_counts_and_every_vertex_stays_in_its_cell(cells):
    v, f = cases.sphere()
    assert D.all_edges_even(f) and len(f) > 500
    h = cases.CUBE_SIDE / cells
    out = D.decimate(v, f, [0, len(v)], [0, len(f)], cells, lo=np.zeros((1, 3)), h=np.full(1, h))
    assert 0 < out['tend'][1] < len(f) and 0 < out['vend'][1] < len(v)
    assert D.all_edges_even(out['f'])
    assert out['f'].min() == 0 and out['f'].max() == out['vend'][1] - 1
    assert sorted(set(out['f'].reshape(-1).tolist())) == list(range(out['vend'][1]))      # compacted: every vertex is named
    assert (np.diff(out['key']) > 0).all()                                                 # ascending key order
    slack = 2 * F32_EPS * cases.CUBE_SIDE                                                  # the one f32 rounding
    assert (np.abs(out['v'] - out['centre']) <= h / 2 + slack).all()
    ijk, has = D.vertex_cells(v, np.zeros(3), h, cells)
    key = (ijk[:, 2] * cells + ijk[:, 1]) * cells + ijk[:, 0]
    rep = {int(k): out['v'][i].astype(np.float64) for i, k in enumerate(out['key'])}
    far = [np.linalg.norm(v[i] - rep[int(key[i])]) for i in range(len(v)) if int(key[i]) in rep]
    assert len(far) > len(v) // 2 and max(far) <= h * np.sqrt(3) + slack


def test_two_meshes_do_not_see_each_other():
    s, e = cases.sphere(), cases.ellipsoid()
    v, f, vend, tend = cases.batch([s, e])
    both = D.decimate(v, f, vend, tend, 5, lo=np.zeros((2, 3)), h=np.full(2, cases.CUBE_SIDE / 5))
    alone = D.decimate(e[0], e[1], [0, len(e[0])], [0, len(e[1])], 5, lo=np.zeros((1, 3)), h=np.full(1, cases.CUBE_SIDE / 5))
    assert np.array_equal(both['v'][both['vend'][1]:], alone['v'])
    assert np.array_equal(both['f'][both['tend'][1]:], alone['f'])
    assert np.array_equal(both['key'][both['vend'][1]:] - 125, alone['key'])


# ------------------------------------------------------------------------------------------------ mod 2 and guards ----
TRIANGLE = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.25, 0.75, 0.25]])


def test_two_coincident_opposite_faces_vanish():
    out = D.decimate(TRIANGLE, [[0, 1, 2], [0, 2, 1]], [0, 3], [0, 2], 2, lo=np.zeros((1, 3)), h=np.full(1, 0.5))
    assert out['vend'] == [0, 0] and out['tend'] == [0, 0] and out['v'].shape == (0, 3)


def test_three_coincident_faces_leave_the_first():
    out = D.decimate(TRIANGLE, [[1, 2, 0], [0, 2, 1], [0, 1, 2]], [0, 3], [0, 3], 2, lo=np.zeros((1, 3)), h=np.full(1, 0.5))
    assert out['vend'] == [0, 3] and out['tend'] == [0, 1]
    assert out['f'].tolist() == [[1, 2, 0]]


def test_a_bad_index_or_a_vertex_without_a_cell_removes_its_faces_only():
    v = np.concatenate([TRIANGLE, [[0.75, 0.75, 0.25], [np.nan, 0.25, 0.75]]])
    out = D.decimate(v, [[0, 1, 2], [1, 3, 2], [0, 1, 4], [0, 1, 5], [0, -1, 2]], [0, 5], [0, 5], 2,
                     lo=np.zeros((1, 3)), h=np.full(1, 0.5))
    assert out['f'].tolist() == [[0, 1, 2], [1, 3, 2]] and out['vend'] == [0, 4]


def test_the_guards_of_the_device_entry_need_no_gpu():
    from rfdnet_amd.iscnet.decimate import decimate_meshes
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="cells"):
        decimate_meshes(v, f, [0, 3], [0, 1], 0)
    with pytest.raises(ValueError, match="2\\^31"):
        decimate_meshes(v, f, [0, 3], [0, 1], 1291)                     # 1291^3 >= 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        decimate_meshes(v, f, [0, 1, 2, 3, 3], [0, 1, 1, 1, 1], 813)    # 4 x 813^3 >= 2^31 > 4 x 812^3
    with pytest.raises(RuntimeError, match="CPU not supported"):
        decimate_meshes(v, f, [0, 3], [0, 1], 4)
    with pytest.raises(ValueError):
        D.decimate(v.numpy(), f.numpy(), [0, 3], [0, 1], 0)
    with pytest.raises(ValueError):
        D.decimate(v.numpy(), f.numpy(), [0, 3], [0, 1], 1291)


# ------------------------------------------------------------------------------------------------------ the layers ----
def test_the_generator_switch_and_the_config_key():
    from rfdnet_amd.iscnet.config import DEFAULT_CONFIG, Config
    from rfdnet_amd.iscnet.generator import Generator3D
    from rfdnet_amd.iscnet.occupancy_net import ONet
    assert 'decimate_cells' not in DEFAULT_CONFIG['generation']         # every default is a key of the reference's file
    assert ONet(Config({})).generator.decimate_cells == 0
    g = ONet(Config({'generation': {'decimate_cells': 16}})).generator
    assert g.decimate_cells == 16
    assert g.set_decimation(None) is g and g.decimate_cells == 0
    assert g.set_decimation(8).decimate_cells == 8 and g.set_decimation(0).decimate_cells == 0
    with pytest.raises(ValueError):
        g.set_decimation(-1)
    with pytest.raises(NotImplementedError):                             # the reference's edge collapse stays out
        Generator3D(None, simplify_nfaces=1000)


def test_the_demo_has_the_flag():
    import demo
    assert demo.build_parser().parse_args(["--decimate_cells", "16"]).decimate_cells == 16
    assert demo.build_parser().parse_args([]).decimate_cells is None
