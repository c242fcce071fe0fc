"""GPU (-m gpu): mesh decimation on the device (rfdnet_amd/iscnet/decimate.py, csrc/mesh_decimate.hip) against the numpy
float64 restatement of its five rules (tests/decimate_f64.py).

Offsets and faces must be EQUAL.  A vertex coordinate may differ by one f32 unit in the last place of
max(|coordinate|, h): both sides perform the same f64 operations in the same order, only the f64 divisions and square
roots may differ, in their last place, and the single rounding to f32 can then fall the other way at a rounding boundary
only.  Every comparison prints the largest difference in such units and the number of unequal coordinates.

Measured on MI355X: every comparison of this file came out with 0 unequal coordinates (largest difference 0 units)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases as cases  # noqa: E402
import decimate_f64 as D  # noqa: E402
from seeded import seeded_onet  # noqa: E402

pytestmark = pytest.mark.gpu


def on_device(v, f, vend, tend, cells, lo=None, h=None, dtype=np.float64, **kw):
    """decimate_meshes on numpy inputs -> (v2 f32, f2 int64, vend2, tend2) as numpy / lists"""
    from rfdnet_amd.iscnet.decimate import decimate_meshes
    vt = torch.from_numpy(np.array(v, dtype=dtype).reshape(-1, 3)).cuda()            # a copy: the cases stay unchanged
    ft = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).cuda()
    v2, f2, vend2, tend2 = decimate_meshes(vt, ft, vend, tend, cells, lo=lo, h=h, **kw)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and v2.is_cuda and f2.is_cuda
    assert tuple(v2.shape) == (vend2[-1], 3) and tuple(f2.shape) == (tend2[-1], 3)
    return v2.cpu().numpy(), f2.cpu().numpy().astype(np.int64), vend2, tend2


def assert_same(name, got, want):
    """the comparison of the module docstring; -> (largest difference in units, unequal coordinates)"""
    v2, f2, vend2, tend2 = got
    assert vend2 == want['vend'] and tend2 == want['tend'], (name, vend2, want['vend'], tend2, want['tend'])
    assert np.array_equal(f2, want['f']), name
    if v2.size == 0:
        print("%s: empty" % name)
        return 0.0, 0
    unit = np.spacing(np.maximum(np.abs(want['v']), want['h'][:, None].astype(np.float32)))
    d = np.abs(v2.astype(np.float64) - want['v'].astype(np.float64)) / unit
    unequal = int((v2 != want['v']).sum())
    print("%s: %d vertices, %d faces, largest difference %.3g units, %d of %d coordinates unequal"
          % (name, v2.shape[0], f2.shape[0], d.max(), unequal, v2.size))
    assert d.max() <= 1.0, name
    return float(d.max()), unequal


def both(name, v, f, vend, tend, cells, lo, h, dtype=np.float64, **kw):
    want = D.decimate(np.asarray(v, dtype), f, vend, tend, cells, lo=lo, h=h, **kw)
    got = on_device(v, f, vend, tend, cells, lo=lo, h=h, dtype=dtype, **kw)
    assert_same(name, got, want)
    return got, want


ONE_FACE = (np.array([[1., 1., 1.], [10., 1., 1.], [1., 10., 1.]]), np.array([[0, 1, 2]]))
EMPTY = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))


@pytest.fixture(scope="module")
def ragged_batch():
    return cases.batch([cases.sphere(), cases.ellipsoid(), EMPTY, ONE_FACE])


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [4, 7])
def test_a_ragged_batch_equals_the_restatement(hip, ragged_batch, cells):
    v, f, vend, tend = ragged_batch
    lo, h = np.zeros((4, 3)), np.full(4, cases.CUBE_SIDE / cells)
    got, want = both("ragged batch, cells %d" % cells, v, f, vend, tend, cells, lo, h)
    hip.device_status()
    assert got[2][2] == got[2][3] and got[3][2] == got[3][3]                 # the empty mesh stays empty
    assert got[3][4] - got[3][3] == 1 and got[2][4] - got[2][3] == 3           # the one face survives
    assert 0 < got[3][1] < tend[1]
    for k in range(2):                                                        # closed in, even edge counts out
        assert D.all_edges_even(got[1][got[3][k]:got[3][k + 1]])


def test_f32_vertices_and_the_default_cube(hip):
    """f32 input is widened, not converted beforehand; lo / h default to the generator's cube [-0.55, 0.55]^3"""
    v, f = cases.sphere()
    v = ((v / cases.CUBE_SIDE - 0.5) * 1.1).astype(np.float32)
    vend, tend = [0, len(v)], [0, len(f)]
    want = D.decimate(v, f, vend, tend, 6)
    assert_same("f32 vertices, default cube", on_device(v, f, vend, tend, 6, dtype=np.float32), want)
    assert want['tend'][1] > 0 and np.allclose(want['h'], 1.1 / 6)


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [2, 4, 8, 16])
def test_lattice_aligned_vertices_get_numpy_s_cells(hip, cells):
    """the 17^3 points of the 16^3 lattice over the generator's cube, computed as lo + i * step and once more through
    the a * x + c form of the marching-cubes kernel (the same points up to a rounding): every one lies on, or a rounding
    away from, a cell boundary of a grid that divides 16"""
    box, n = 1.1, 17
    i = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1).reshape(-1, 3)
    a = box / (n - 1)
    forms = np.concatenate([-box / 2 + i * a, a * (i + 1.5) + (-1.5 * a - 0.5 * box)])
    lo, h = np.full((1, 3), -box / 2), np.full(1, box / cells)
    vt = torch.from_numpy(forms).cuda()
    par = torch.from_numpy(np.concatenate([lo.reshape(-1), 1.0 / h])).cuda()
    vend = torch.tensor([0, len(forms)], dtype=torch.int32, device="cuda")
    key = torch.empty(len(forms), dtype=torch.int32, device="cuda")
    hip.call("rfd_decimate_vertex_keys", vt.device, len(forms), 1, cells, 0, vt.data_ptr(), vend.data_ptr(),
             par[:3].data_ptr(), par[3:].data_ptr(), key.data_ptr())
    ijk, has = D.vertex_cells(forms, lo[0], h[0], cells)
    assert has.all()
    assert np.array_equal(key.cpu().numpy(), (ijk[:, 2] * cells + ijk[:, 1]) * cells + ijk[:, 0])
    t = (forms - lo[0]) * (1.0 / h[0])
    assert (t == np.floor(t)).any(1).sum() > 4000                # exactly on a boundary in f64; the rest a rounding away


@pytest.mark.parametrize("cells", [6, 9])
def test_a_sphere_with_vertices_on_cell_boundaries(hip, cells):
    """marching-cubes vertices have two integer coordinates; h = 3 and h = 2 put many of them on a boundary"""
    v, f = cases.sphere()
    h = cases.CUBE_SIDE / cells
    assert h == int(h) and (np.mod(v, h) == 0).any(1).sum() > 100
    both("boundary sphere, cells %d" % cells, v, f, [0, len(v)], [0, len(f)], cells, np.zeros((1, 3)), np.full(1, h))


# 3 -------------------------------------------------------------------------------------------------------------------
def test_vertices_outside_the_cube_bad_indices_and_a_nan(hip):
    v, f = (a.copy() for a in cases.sphere())
    v = (v - 9.0) * 2.5 + 9.0                                   # the sphere now leaves [0, 18]^3 on every side
    assert (v < 0).any() and (v > cases.CUBE_SIDE).any()
    v[10, 1], v[200, 0], v[333, 2] = np.nan, np.inf, -np.inf
    f[5, 2], f[77, 0], f[500, 1] = len(v), -1, 2 ** 31 - 1
    vend, tend = [0, len(v)], [0, len(f)]
    lo, h = np.zeros((1, 3)), np.full(1, cases.CUBE_SIDE / 6)
    got, want = both("outside / non-finite / bad index", v, f, vend, tend, 6, lo, h)
    hip.device_status()
    assert np.isfinite(got[0]).all() and 0 < got[3][1]
    assert (got[0] >= -1e-6).all() and (got[0] <= cases.CUBE_SIDE + 1e-5).all()        # clamped into edge cells
    # the hand-made case: of five faces the NaN vertex's, the index past the end and the negative index go, nothing else
    tri = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [0.75, 0.75, 0.25], [np.nan, 0.25, 0.75]])
    small = on_device(tri, [[0, 1, 2], [1, 3, 2], [0, 1, 4], [0, 1, 5], [0, -1, 2]], [0, 5], [0, 5], 2,
                      lo=np.zeros((1, 3)), h=np.full(1, 0.5))
    assert small[1].tolist() == [[0, 1, 2], [1, 3, 2]] and small[2] == [0, 4] and small[3] == [0, 2]


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_corners", [1, 15, 16, 17, 33])
def test_cells_with_a_given_number_of_corners(hip, n_corners):
    """the hub cell visits exactly n_corners corners: every length of the lanes' loops around the sixteen partial sums"""
    v, f = cases.two_hubs(n_corners)
    lo, h = np.full((1, 3), -1.25), np.full(1, 0.5)
    got, want = both("%d corners" % n_corners, v, f, [0, len(v)], [0, len(f)], 5, lo, h)
    hub = np.nonzero(want['key'] == (2 * 5 + 2) * 5 + 2)[0]
    assert len(hub) == 1 and want['corners'][hub[0]] == n_corners
    assert (np.abs(want['v'][hub[0]] - want['centre'][hub[0]]) < 0.24).all()              # not clamped: the sums show
    if n_corners > 1:
        # ... and they matter: without the last corner the hub would sit elsewhere
        less = D.decimate(v, f[:-1], [0, len(v)], [0, len(f) - 1], 5, lo=lo, h=h)
        other = less['v'][np.nonzero(less['key'] == 62)[0][0]]
        assert np.abs(other - want['v'][hub[0]]).max() > 1e-4


# 5 -------------------------------------------------------------------------------------------------------------------
def test_a_cell_of_zero_area_faces_sits_at_its_centre(hip):
    v = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [1.1, 0.1, 0.1]])               # collinear, three cells
    got, want = both("zero weight", v, [[0, 1, 2]], [0, 3], [0, 1], 4, np.zeros((1, 3)), np.full(1, 0.5))
    assert (want['W'] == 0).all()
    assert np.array_equal(got[0], np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.25, 0.25, 0.25]], np.float32))
    assert got[1].tolist() == [[0, 1, 2]]


# 6, 7 ----------------------------------------------------------------------------------------------------------------
def test_a_mesh_alone_equals_itself_in_a_batch_and_two_calls_are_equal(hip):
    e, s = cases.ellipsoid(), cases.sphere()
    cells = 7
    h = cases.CUBE_SIDE / cells
    alone = on_device(e[0], e[1], [0, len(e[0])], [0, len(e[1])], cells, lo=np.zeros((1, 3)), h=np.full(1, h))
    v, f, vend, tend = cases.batch([s, ONE_FACE, EMPTY, e, s])
    one = on_device(v, f, vend, tend, cells, lo=np.zeros((5, 3)), h=np.full(5, h))
    two = on_device(v, f, vend, tend, cells, lo=np.zeros((5, 3)), h=np.full(5, h))
    hip.device_status()
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(one[1], two[1])
    assert one[2:] == two[2:]
    vs, fs = slice(one[2][3], one[2][4]), slice(one[3][3], one[3][4])
    assert np.array_equal(one[0][vs].view(np.uint32), alone[0].view(np.uint32)) and alone[0].shape[0] > 20
    assert np.array_equal(one[1][fs], alone[1])
    first, last = slice(one[2][0], one[2][1]), slice(one[2][4], one[2][5])
    assert np.array_equal(one[0][first].view(np.uint32), one[0][last].view(np.uint32))


def test_empty_meshes_at_the_head_and_twice_in_a_row(hip):
    """[empty, tetrahedron, empty, empty, octahedron]: offsets that begin with a repeat and repeat twice in the middle, the
    inputs of the search for the mesh of a vertex or face.  Two cells a side; every vertex of both meshes has a cell of
    its own, so every face stays.  (An octahedron with its vertices ON the axes cannot do that in any 2^3 grid -- one vertex
    of every axis shares the cell of the origin -- so this one has them pushed into six octants.)"""
    tet = (np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]),
           np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))
    octa = (np.array([[1., .2, .2], [-1., -.2, -.2], [-.2, 1.25, .2], [.2, -1., -.2], [.2, -.2, 1.5], [-.2, .2, -.75]]),
            np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))
    meshes = [EMPTY, tet, EMPTY, EMPTY, octa]
    v, f, vend, tend = cases.batch(meshes)
    lo = np.array([[0.] * 3, [-.5] * 3, [0.] * 3, [0.] * 3, [-2.] * 3])
    h = np.array([1., 1., 1., 1., 2.])
    for k in (1, 4):
        ijk, has = D.vertex_cells(meshes[k][0], lo[k], h[k], 2)
        assert has.all() and len(set(map(tuple, ijk.tolist()))) == len(meshes[k][0])
    got, want = both("empties around a tetrahedron and an octahedron", v, f, vend, tend, 2, lo, h)
    hip.device_status()
    assert got[2] == [0, 0, 4, 4, 4, 10] and got[3] == [0, 0, 4, 4, 4, 12]
    for k in (1, 4):
        mv, mf = meshes[k]
        alone = on_device(mv, mf, [0, len(mv)], [0, len(mf)], 2, lo=lo[k:k + 1], h=h[k:k + 1])
        vs, fs = slice(got[2][k], got[2][k + 1]), slice(got[3][k], got[3][k + 1])
        assert np.array_equal(got[0][vs].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(got[1][fs], alone[1])


# 8 -------------------------------------------------------------------------------------------------------------------
def test_a_thin_sheet_loses_its_duplicates_mod_2(hip):
    v, f = cases.slab()
    assert D.all_edges_even(f)
    lo, h = np.full((1, 3), -0.5), np.ones(1)
    got, want = both("thin sheet", v, f, [0, len(v)], [0, len(f)], 8, lo, h)
    ijk, _ = D.vertex_cells(v, lo[0], 1.0, 8)
    candidates = len(np.unique((ijk[:, 2] * 8 + ijk[:, 1]) * 8 + ijk[:, 0]))
    assert 0 < got[2][1] < candidates                    # the thin part's cells are candidates nobody names any more
    assert 0 < got[3][1] < len(f)
    assert sorted(set(got[1].reshape(-1).tolist())) == list(range(got[2][1]))
    assert D.all_edges_even(got[1])
    sets = [tuple(sorted(t)) for t in got[1].tolist()]
    assert len(set(sets)) == len(sets)                   # no vertex set twice


def test_the_c_entries_refuse_what_they_cannot_index(hip):
    """the launchers' own argument checks (nothing is launched): the key range, a null pointer, 3 F past int32"""
    dev = torch.device("cuda", 0)
    t = torch.zeros(16, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    for cells, K in ((0, 1), (1291, 1), (1290, 2)):
        with pytest.raises(hip.RfdHipError, match="cells"):
            hip.call("rfd_decimate_vertex_keys", dev, 1, K, cells, 0, p, p, p, p, p)
    with pytest.raises(hip.RfdHipError, match="null"):
        hip.call("rfd_decimate_vertex_keys", dev, 1, 1, 4, 0, p, p, None, p, p)
    with pytest.raises(hip.RfdHipError, match="3 F"):
        hip.call("rfd_decimate_cell_solve", dev, 1, 1, 2 ** 30, 4, 0, p, p, p, p, p, p, p, p, p, 1e-3, p)
    with pytest.raises(hip.RfdHipError, match="regularise"):
        hip.call("rfd_decimate_cell_solve", dev, 1, 1, 1, 4, 0, p, p, p, p, p, p, p, p, p, -1.0, p)
    hip.device_status()


# 9 -------------------------------------------------------------------------------------------------------------------
def test_the_generator_decimates_before_normals_and_refinement(hip, golden_dir):
    fx = np.load(os.path.join(golden_dir, "F_GEN.npz"))
    codes = torch.from_numpy(fx["codes"]).cuda()

    def generate(configure):
        onet = seeded_onet(fx, generation={'resolution_0': 8, 'upsampling_steps': 1})
        g = configure(onet.generator)
        with torch.no_grad():
            np.random.seed(4)
            meshes = g.generate_mesh(codes, None)
        hip.device_status()
        return g, meshes

    def full(g):
        g.with_normals = True
        return g.set_refinement(2)
    g0, plain = generate(full)
    g1, thin = generate(lambda g: full(g).set_decimation(4))
    v0, f0, vend0, tend0 = g0.last_buffers
    v1, f1, vend1, tend1 = g1.last_buffers
    K = codes.shape[0]
    assert len(plain) == len(thin) == K and tend0[-1] > 0
    assert 0 < tend1[-1] < tend0[-1] and 0 < vend1[-1] < vend0[-1]
    assert len(vend1) == len(tend1) == K + 1 and vend1[0] == tend1[0] == 0
    assert tuple(v1.shape) == (vend1[-1], 3) and tuple(f1.shape) == (tend1[-1], 3)
    assert v1.dtype == torch.float32 and torch.isfinite(v1).all()
    assert tuple(g1.last_normals.shape) == (vend1[-1], 3)
    for k, m in enumerate(thin):
        nv, nf = vend1[k + 1] - vend1[k], tend1[k + 1] - tend1[k]
        assert nv <= vend0[k + 1] - vend0[k] and nf <= tend0[k + 1] - tend0[k]
        assert tuple(m.vertices.shape) == (nv, 3) and tuple(m.faces.shape) == (nf, 3)
        if nv:
            assert tuple(m.vertex_normals.shape) == (nv, 3)
            assert int(m.faces.min()) == 0 and int(m.faces.max()) == nv - 1
            assert float(m.vertices.abs().max()) <= 0.55 + 3e-3           # in the cube, moved by two RMSprop steps at most
    # switched off again, the generator makes the calls it always made
    g2, again = generate(lambda g: full(g).set_decimation(4).set_decimation(0))
    for a, b in zip(g0.last_buffers[:2], g2.last_buffers[:2]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert list(g0.last_buffers[2]) == list(g2.last_buffers[2]) and list(g0.last_buffers[3]) == list(g2.last_buffers[3])
    assert torch.equal(g0.last_normals, g2.last_normals)
