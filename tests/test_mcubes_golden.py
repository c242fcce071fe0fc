"""CPU: marching cubes pinned by the meshes the reference itself holds
(demo/outputs/scene0549_00/proposal_*_mesh.ply -> tests/golden/F_MC.npz, data only).

What they pin: the `-1.5` vertex transform of generator.py:163-168 (PyMCubes returns plain
padded-grid index coordinates), the orientation, one shared vertex per crossed edge, the
rows of the library's case table that occur (189 of 256), and its vertex / triangle order.
The oracle (oracle_marching_cubes + oracle.extract_mesh) reproduces every demo mesh from a
value grid rebuilt from it: identical face arrays, vertices to float32-PLY precision.
Not observable there: a grid value exactly on the iso level; the last bit of the double
interpolation; 67 table rows that do not occur (validated structurally instead,
tools/gen_mc_tables.py)."""
import collections

import numpy as np
import pytest

import mc_golden as MG
import mc_ref
from oracle import oracle


@pytest.fixture(scope="module")
def meshes():
    z, names = MG.load()
    out = []
    for n in names:
        v, f = z[n + "_v"], z[n + "_f"]
        out.append((n, v, f) + MG.analyse(v, f))
    return out


def test_vertices_sit_on_padded_lattice_edges_under_the_reference_transform(meshes):
    """generator.py:163-168 subtracts 0.5 + 1 from the library's output: undoing exactly that
    (+1.5) leaves two integer coordinates per vertex; undoing only the padding (+1.0) none."""
    for n, v, f, u, *_ in meshes:
        r = np.abs(u - np.round(u)) < MG.TOL
        assert (r.sum(1) >= 2).all(), n
        u1 = MG.to_lattice(v, 1.0)
        r1 = np.abs(u1 - np.round(u1)) < MG.TOL
        assert r1.sum(1).mean() < 0.02, n
        assert u.min() >= 1 - MG.TOL and u.max() <= MG.D - 2 + MG.TOL, n


def test_orientation_sharing_closedness(meshes):
    for n, v, f, u, base, axis, t, inside in meshes:
        p = v.astype(np.float64)
        vol = np.einsum('ij,ij->i', p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6
        assert vol > 0, n                                   # normals towards lower values
        keys = set(zip(base[:, 0], base[:, 1], base[:, 2], axis))
        assert len(keys) == len(v), n                       # one vertex per crossed edge
        mc_ref.assert_closed_oriented_manifold(f)
        assert f.min() == 0 and f.max() == len(v) - 1


def test_vertex_order_is_high_end_point_x_major_then_axis(meshes):
    for n, v, f, u, base, axis, t, inside in meshes:
        hi = base.copy()
        hi[np.arange(len(v)), axis] += 1
        key = ((hi[:, 0] * MG.D + hi[:, 1]) * MG.D + hi[:, 2]) * 3 + axis
        assert (np.diff(key) > 0).all(), n


def test_triangle_order_is_cell_x_major(meshes):
    for n, v, f, u, base, axis, t, inside in meshes:
        cells = [c for c, _ in MG.faces_by_cell(base, axis, f)]
        lin = [(c[0] * MG.D + c[1]) * MG.D + c[2] for c in cells]
        assert (np.diff(lin) > 0).all(), n                  # each cell once, ascending


def test_case_table_rows_read_back_from_the_demo_meshes(meshes):
    tb = mc_ref.table()
    seen = collections.defaultdict(set)
    for n, v, f, u, base, axis, t, inside in meshes:
        ci = MG.cube_indices(inside)
        by_cell = MG.faces_by_cell(base, axis, f)
        assert len(by_cell) == int(((ci != 0) & (ci != 255)).sum()), n
        for cell, tris in by_cell:
            seen[int(ci[cell])].add(tuple(tris))
    assert len(seen) >= 189
    for case, variants in seen.items():
        assert len(variants) == 1, case                     # the library is table driven
        assert list(next(iter(variants))) == [tuple(t) for t in tb[case]], case


def test_oracle_reproduces_every_demo_mesh(meshes):
    worst = 0.0
    for n, v, f, u, base, axis, t, inside in meshes:
        g = MG.rebuild_grid(base, axis, t, inside)
        ov, of = oracle.extract_mesh(g, 0.0)
        assert of.shape == f.shape and np.array_equal(of, f), n      # identical face array
        assert ov.shape == v.shape, n
        err = np.abs(ov - v.astype(np.float64)).max() * (MG.N - 1) / MG.BOX     # in cells
        worst = max(worst, err)
        assert err < 2e-3, (n, err)
    print("max vertex deviation from the demo meshes: %.2e cells" % worst)


def test_oracle_iso_level_convention_and_midpoint():
    g = np.full((3, 3, 3), -1.0)
    g[1, 1, 1] = 0.0                    # exactly on the level: counts as below -> empty mesh
    v, t = oracle.marching_cubes(g, 0.0)
    assert len(v) == 0 and len(t) == 0
    g[1, 1, 1] = 1.0
    v, t = oracle.marching_cubes(g, 0.0)
    assert len(v) == 6 and len(t) == 8
    assert np.allclose(np.sort(np.abs(v - 1).sum(1)), 0.5)


@pytest.mark.parametrize("iso", [np.log(0.3 / 0.7), 0.1])
def test_oracle_at_non_zero_iso_levels_matches_the_numpy_restatement(iso):
    """everything above pins the oracle at iso 0 only; tests/test_gpu_mcubes.py leans on it at other levels.  On a
    random grid without on-level values it must give the triangle soup of the independent restatement (mc_ref)."""
    rng = np.random.default_rng(5)
    g = iso + rng.standard_normal((6, 6, 6))
    assert (g != iso).all()
    v, t = oracle.marching_cubes(np.pad(g, 1, constant_values=-1e6), iso)
    ref = mc_ref.marching_cubes_soup(g, iso)
    assert len(t) == len(ref) > 100
    assert mc_ref.canon(v[t]) == mc_ref.canon(ref)
    mc_ref.assert_closed_oriented_manifold(t)
    # and the level matters: the mesh at iso is not the mesh at 0
    v0, t0 = oracle.marching_cubes(np.pad(g, 1, constant_values=-1e6), 0.0)
    assert len(t0) != len(t) or not np.array_equal(t0, t)
