"""GPU (-m gpu): exact point-to-mesh distance on the device (rfdnet_amd/mesh_distance.py, csrc/mesh_dist.hip) against the
float64 restatement of its rules D1 - D8 (tests/mesh_dist_f64.py) on the shapes of tests/mesh_dist_cases.py.

Equality means BIT equality of d2, face and closest point with the restatement's brute force over all valid faces: both
sides perform the same f64 operations in the same order (divisions and square roots are correctly rounded on both), and
the answer is the least key (d2, face row), a total order, so neither the cells, nor the walk, nor the batch may show.
Every comparison covers every query of its case.  The last test prints the file's tally: the number of float64 values
compared, how many were not bit-equal, and the largest difference in units in the last place."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_dist_cases as M  # noqa: E402
import mesh_dist_f64 as D  # noqa: E402
import simplify_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

TALLY = {'values': 0, 'unequal': 0, 'max_ulp': 0}

# test 7: the largest relative gap, measured on the CPU, between the two-sided RMS of tests/mesh_dist_f64.py (brute
# force, tree sums) and simplify_cases.two_sided_rms (numpy's mean) on the six pairs of tests/golden/F_SIMPLIFY.npz, both
# float64 and neither the code under test: 2.2144e-16 (blobby_sphere / ref; 1.2347e-16 torus / clu; 0 on the other four)
RMS_GAP = 2.2144e-16


def ordered(x):
    """float64 -> int64 that ascends with the value (-0 and +0 apart by one)"""
    i = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i - 1, i)        # negative floats: reversed below the positive ones


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


def build(v, f, vend=None, tend=None, cells=None):
    from rfdnet_amd.mesh_distance import MeshDistance
    return MeshDistance(cuda(np.asarray(v, np.float64).reshape(-1, 3)), cuda(np.asarray(f).reshape(-1, 3), np.int32),
                        vend, tend, cells=cells)


def ask(md, points, obj=None, **kw):
    d2, face, closest = md.query(cuda(points, np.float64), None if obj is None else cuda(obj, np.int32),
                                 return_closest=True, **kw)
    assert d2.dtype == torch.float64 and face.dtype == torch.int32 and closest.dtype == torch.float64
    assert tuple(d2.shape) == tuple(face.shape) == (len(points),) and tuple(closest.shape) == (len(points), 3)
    return d2.cpu().numpy(), face.cpu().numpy().astype(np.int64), closest.cpu().numpy()


def assert_equal(name, got, want):
    assert np.array_equal(got[1], want[1]), name
    assert unequal(name + " d2", got[0], want[0]) == 0
    assert unequal(name + " closest", got[2], want[2]) == 0


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_one_triangle_every_region_and_boundary(hip, n):
    v, f = M.TRIANGLE
    points = M.triangle_queries(n)
    got = ask(build(v, f), points)
    want = D.Batch(v, f, [0, 3], [0, 1]).query(points, np.zeros(n, np.int64), brute=True)
    assert_equal("one triangle, %d queries" % n, got, want)
    assert (got[1] == 0).all()
    for i, (_, q, region) in enumerate(M.REGIONS[:n]):
        assert np.array_equal(got[2][i], np.array(q)), region               # the closest points written down by hand


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.TIES))
def test_the_lowest_face_row_wins_a_tie(hip, name):
    (v, f), points, rows = M.TIES[name]
    b = D.Batch(v, f, [0, len(v)], [0, len(f)], cells=1)
    want = b.query(points, np.zeros(len(points), np.int64), brute=True)
    for i, p in enumerate(points):
        every = D.closest_points(p, b.tri)[1]
        tied = np.nonzero(every == every.min())[0]
        assert len(tied) >= 2 and want[1][i] == tied.min()
    if rows is not None:
        assert want[1].tolist() == rows
    for cells in (1, 2, 5):
        assert_equal("%s, %d cells" % (name, cells), ask(build(v, f, cells=cells), points), want)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(hip):
    """the ragged batch on the device at every cell count -> {cells: (d2, face, closest)}, computed once"""
    case = M.ragged_case()
    out = {}
    for cells in M.DEVICE_CELLS:
        md = build(case['v'], case['f'], case['vend'], case['tend'], cells=cells)
        out[cells] = (md, ask(md, case['points'], case['obj']))
    return out


@pytest.mark.parametrize("cells", M.DEVICE_CELLS)
def test_the_ragged_batch_equals_the_brute_force_at_every_cell_count(hip, ragged, cells):
    case = M.ragged_case()
    md, got = ragged[cells]
    hip.device_status()
    assert np.array_equal(md.valid.cpu().numpy().astype(bool), case['valid'])
    assert md.res.tolist() == [f.R for f in M.restated_batch(cells).frames]
    assert_equal("ragged batch, cells %s" % cells, got, case['brute'])
    empty = case['obj'] == M.NAMES.index('empty')
    nan = ~np.isfinite(case['points']).all(1)
    assert nan.sum() == len(M.NAMES) and empty.sum() > 10
    assert (got[1][empty | nan] == -1).all() and np.isnan(got[0][nan]).all() and (got[0][empty & ~nan] == np.inf).all()
    assert np.isnan(got[2][empty | nan]).all() and (got[1][~(empty | nan)] >= 0).all()


# 4 -------------------------------------------------------------------------------------------------------------------
def test_an_object_alone_equals_itself_in_the_batch_and_calls_and_orders_agree(hip, ragged):
    case = M.ragged_case()
    md, got = ragged[None]
    for name in ('icosphere320', 'bad_mesh', 'square'):
        k = M.NAMES.index(name)
        mine = case['obj'] == k
        v, f = M.OBJECTS[name]
        alone = ask(build(v, f), case['points'][mine])
        in_batch = (got[0][mine], np.where(got[1][mine] >= 0, got[1][mine] - case['tend'][k], -1), got[2][mine])
        assert_equal(name + " alone", alone, in_batch)
    assert_equal("second call", ask(md, case['points'], case['obj']), got)
    assert_equal("unsorted launch", ask(md, case['points'], case['obj'], sort_points=False), got)
    perm = np.random.default_rng(0).permutation(len(case['points']))
    shuffled = ask(md, case['points'][perm], case['obj'][perm])
    assert_equal("shuffled queries", shuffled, tuple(x[perm] for x in got))


# 5 -------------------------------------------------------------------------------------------------------------------
def test_the_sums_of_every_segment_equal_the_restatement(hip):
    from rfdnet_amd.mesh_distance import segment_sums
    v, f = M.OBJECTS['octahedron']
    md = build(v, f)
    tri = md.tri.cpu().numpy()
    rng = np.random.default_rng(1)
    lengths = [0, 1, 63, 64, 65, 4097, 10, 6]
    seg = np.concatenate([[0], np.cumsum(lengths)])
    n = int(seg[-1])
    d2 = rng.uniform(0, 0.3, n) ** 2
    face = rng.integers(0, len(f), n)
    normals = rng.normal(size=(n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    tau = [0.25, 0.1, 0.3]
    a = int(seg[6])                                                        # a segment holding non-finite distances
    d2[a + 2], d2[a + 5], d2[a + 7] = np.inf, np.nan, -1.
    face[a + 2], face[a + 5] = -1, -1
    b = int(seg[7])                                                        # d == tau exactly, and one place either side
    d2[b:b + 6] = [0.0625, np.nextafter(0.25, 1) ** 2, np.nextafter(0.0625, 0), 0.01, 0.09, 0.09]
    assert np.sqrt(d2[b]) == 0.25 and np.sqrt(d2[b + 1]) > 0.25 and np.sqrt(d2[b + 2]) < 0.25 and np.sqrt(0.01) == 0.1
    want_sums, want_counts = D.sums(seg, d2, face, normals, tri, tau)
    assert want_counts[6, 0] == 3 and want_counts[0].tolist() == [0, 0, 0, 0]
    assert want_counts[7].tolist() == [0, 3, 1, 6]
    sums, counts = segment_sums(md, cuda(seg, np.int32), cuda(d2), cuda(face, np.int32), cuda(normals), tau)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert unequal("segment sums", sums.cpu().numpy(), want_sums) == 0
    plain, _ = segment_sums(md, cuda(seg, np.int32), cuda(d2), cuda(face, np.int32), None, ())
    assert unequal("sums without normals", plain.cpu().numpy()[:, :2], want_sums[:, :2]) == 0
    assert (plain.cpu().numpy()[:, 2] == 0).all()


# 6 -------------------------------------------------------------------------------------------------------------------
def test_two_parallel_squares_read_a_quarter(hip):
    from rfdnet_amd.mesh_distance import mesh_metrics, sample_surface_ragged
    (va, fa), (vb, fb) = M.squares()
    A, B = build(va, fa), build(vb, fb)
    gen = torch.Generator(device="cuda").manual_seed(3)
    points, face, normals = sample_surface_ragged(A, 1000, generator=gen)
    d2, _ = B.query(points[0])
    assert (torch.sqrt(d2) == 0.25).all() and (d2 == 0.0625).all()
    m = mesh_metrics(A, B, [[0, 0]], count=1000, thresholds=(0.25, 0.2), generator=gen)
    assert all(v.dtype == torch.float64 and v.is_cuda and v.shape[0] == 1 for v in m.values())
    assert float(m['accuracy']) == 0.25 and float(m['completeness']) == 0.25 and float(m['chamfer_l1']) == 0.25
    assert float(m['chamfer_sq']) == 0.0625 and float(m['rms']) == 0.25
    assert m['precision'].tolist() == [[1., 0.]] and m['recall'].tolist() == [[1., 0.]]
    assert m['fscore'].tolist() == [[1., 0.]]
    assert float(m['normal_consistency']) == 1.


def test_a_mesh_against_itself(hip):
    from rfdnet_amd.mesh_distance import mesh_metrics, sample_surface_ragged
    v, f = M.OBJECTS['icosphere320']
    md = build(v, f)
    extent = float((v.max(0) - v.min(0)).max())
    gen = torch.Generator(device="cuda").manual_seed(4)
    points, face, _ = sample_surface_ragged(md, 2000, generator=gen)
    d2, _ = md.query(points[0])
    assert float(torch.sqrt(d2).max()) <= 1e-15 * extent
    m = mesh_metrics(md, md, [[0, 0]], count=2000, generator=gen)
    assert (m['fscore'] == 1).all() and tuple(m['fscore'].shape) == (1, 2)
    assert abs(float(m['normal_consistency']) - 1) <= 1e-12
    assert float(m['chamfer_l1']) <= 1e-15 * extent


# 7 -------------------------------------------------------------------------------------------------------------------
def test_the_two_sided_rms_of_the_simplification_fixture(hip, golden_dir):
    """The device's two-sided RMS of input against `ref` and against `clu`, with the fixture's own samples as queries,
    against E_r and E_c of tests/golden/F_SIMPLIFY.npz.  Those come from a differently ordered float64 evaluation
    (numpy's mean instead of the tree), so this is not bit equality: the relative gap between the two float64
    evaluations, measured on the CPU, is at most RMS_GAP = 2.2144e-16, and 100 x that is asserted."""
    from rfdnet_amd.mesh_distance import segment_sums
    fx = np.load(os.path.join(golden_dir, "F_SIMPLIFY.npz"))

    def one_way(md, samples):
        d2, face = md.query(cuda(samples))
        seg = cuda(np.array([0, len(samples)]), np.int32)
        sums, counts = segment_sums(md, seg, d2, face)
        assert int(counts[0, 0]) == 0
        return float(sums[0, 1]), len(samples)
    for name in [str(n) for n in fx["names"]]:
        m_in = build(fx[name + "_v"], fx[name + "_f"])
        for tag, key in (("ref", "E_r"), ("clu", "E_c")):
            m_out = build(fx[name + "_%s_v" % tag], fx[name + "_%s_f" % tag])
            s12, n12 = one_way(m_out, fx[name + "_s_in"])
            s21, n21 = one_way(m_in, fx[name + "_s_" + tag])
            rms = float(np.sqrt((s12 + s21) / (n12 + n21)))
            want = float(fx[name + "_" + key])
            print("%s %s: device %.17g  fixture %.17g  relative gap %.3g" % (name, key, rms, want, abs(rms - want) / want))
            assert abs(rms - want) <= 100 * RMS_GAP * want


# 8 -------------------------------------------------------------------------------------------------------------------
def test_ragged_samples_equal_sample_surface_per_object(hip):
    from rfdnet_amd import mesh_sample
    from rfdnet_amd.mesh_distance import sample_surface_ragged
    names = ['icosphere320', 'zero_area', 'empty', 'tetrahedron', 'bad_mesh']
    meshes = [M.ZERO_AREA if n == 'zero_area' else M.OBJECTS[n] for n in names]
    v, f, vend, tend = C.batch(meshes)
    md = build(v, f, vend, tend)
    count = 257
    u = torch.rand(len(names), count, 3, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    points, face, normals = sample_surface_ragged(md, count, u=u)
    cum = md.area_prefix()
    want = D.sample(md.tri.cpu().numpy(), np.asarray(tend), cum.cpu().numpy(), u.cpu().numpy())
    assert np.array_equal(face.cpu().numpy(), want[1])
    assert unequal("ragged samples", points.cpu().numpy(), want[0]) == 0
    assert unequal("ragged normals", normals.cpu().numpy(), want[2]) == 0
    for k, name in enumerate(names):
        rows = slice(tend[k], tend[k + 1])
        if name == 'empty':
            assert torch.isnan(points[k]).all() and (face[k] == -1).all() and (normals[k] == 0).all()
            continue
        if name in ('zero_area', 'bad_mesh'):
            # sample_surface refuses a mesh of no area and one with a NaN vertex: its kernel on this object's triangles
            tri = md.tri[rows].contiguous()
            p1 = torch.empty(count, 3, dtype=torch.float64, device="cuda")
            f1 = torch.empty(count, dtype=torch.int32, device="cuda")
            n1 = torch.empty_like(p1)
            hip.call("rfd_sample_surface", p1.device, count, int(tri.shape[0]), tri.data_ptr(), cum[rows].contiguous().data_ptr(),
                     u[k].contiguous().data_ptr(), p1.data_ptr(), f1.data_ptr(), n1.data_ptr())
        else:
            mv, mf = meshes[k]
            p1, f1, n1 = mesh_sample.sample_surface(cuda(mv), cuda(mf, np.int32), count, u=u[k], return_normals=True,
                                                    dtype=torch.float64, cum=cum[rows])
        assert np.array_equal(face[k].cpu().numpy() - tend[k], f1.cpu().numpy()), name
        assert unequal(name + " samples", points[k].cpu().numpy(), p1.cpu().numpy()) == 0
        assert unequal(name + " normals", normals[k].cpu().numpy(), n1.cpu().numpy()) == 0
        if name == 'zero_area':
            assert (normals[k] == 0).all() and (face[k] == tend[k]).all()
        if name == 'bad_mesh':
            assert md.valid[rows][face[k].long() - tend[k]].all()           # only valid faces are drawn


# 9 -------------------------------------------------------------------------------------------------------------------
def slab():
    """The squares of test 6 made placeable: the placement divides by the mesh's extent on every axis, so a flat mesh
    comes out NaN; two unit squares at z = 0 and z = 1 have an extent, and every point of one such pair is exactly 0.25
    from the same pair shifted by 0.25 along z."""
    (va, fa), _ = M.squares()
    return np.concatenate([va, va + [0., 0., 1.]]), np.concatenate([fa, fa + 4])


def test_scene_mesh_distance_on_placed_objects(hip):
    from rfdnet_amd.iscnet import mesh_eval, scene
    from rfdnet_amd.iscnet.box_util import box_corners_upright_camera
    meshes = [C.tetrahedron(), C.icosphere(2, seed=1), C.torus(), slab(), C.EMPTY]
    ids = np.array([0, 2, 3, 4, 5])
    centre = torch.tensor([[0., 0., 0.], [9., 9., 9.], [1.5, -1., 0.5], [-2., 0.5, 1.], [0.5, 3., 0.25], [4., 4., 1.]],
                          dtype=torch.float64, device="cuda")
    size = torch.tensor([[1., 0.75, 0.5], [1., 1., 1.], [0.5, 0.5, 0.5], [1.25, 1., 0.375], [1., 2., 1.5], [1., 1., 1.]],
                        dtype=torch.float64, device="cuda")
    angle = torch.tensor([0.3, 0., -1.1, 2.0, 0., 0.], dtype=torch.float64, device="cuda")
    corners = box_corners_upright_camera(centre, size, angle)
    box_size = float(size.max())
    # the axis of the scan that is the placed squares' normal, found on the placed mesh itself (its box is not rotated)
    as_mesh = lambda m: mesh_eval.Mesh(cuda(m[0]), cuda(m[1]))
    placed = scene.place_in_corners([as_mesh(slab())], corners[4:5], [0])
    first = placed.vertices[placed.faces[0].long()]
    flat = [a for a in range(3) if len(torch.unique(first[:, a])) == 1]
    assert len(flat) == 1
    shifted = centre[ids].clone()
    shifted[3, flat[0]] += 0.25
    gt_corners = torch.zeros(1, 6, 8, 3, dtype=torch.float64, device="cuda")
    gt_corners[0, :5] = box_corners_upright_camera(shifted, size[ids], angle[ids])
    parsed = {'pred_corners_3d_upright_camera': corners[None]}
    gts = {'gt_corners_3d_upright_camera': gt_corners, 'sem_cls_label': torch.zeros(1, 6, dtype=torch.int64, device="cuda"),
           'box_label_mask': torch.tensor([[1., 1., 1., 1., 1., 0.]], device="cuda")}
    gt_meshes = meshes[:4] + [None]
    pairs = np.array([[0, 0], [2, 1], [3, 2], [4, 3], [5, 4], [0, 4], [5, 0], [1, 0], [0, 5]])
    m = mesh_eval.scene_mesh_distance(meshes, ids, parsed, gts, gt_meshes, pairs, count=2000)
    assert set(m) == set(mesh_eval.METRIC_KEYS)
    assert all(v.dtype == torch.float64 and v.is_cuda and v.shape[0] == len(pairs) for v in m.values())
    l1 = m['chamfer_l1'].cpu().numpy()
    print("chamfer_l1 per pair:", l1)
    assert (l1[:3] <= 1e-6 * box_size).all()
    assert abs(l1[3] - 0.25) <= 1e-6 * box_size
    assert abs(float(m['accuracy'][3]) - 0.25) <= 1e-6 * box_size and abs(float(m['rms'][3]) - 0.25) <= 1e-6 * box_size
    assert (m['fscore'][:3] == 1).all() and (m['fscore'][3] == 0).all()
    for key, value in m.items():
        assert torch.isnan(value[4:]).all(), key                             # no mesh on one side: NaN rows
        assert torch.isfinite(value[:4]).all(), key
    with pytest.raises(ValueError):
        mesh_eval.scene_mesh_distance(meshes, ids, parsed, gts, gt_meshes[:-1], pairs)
    means = mesh_eval.class_means(m, np.zeros(len(pairs), np.int64))
    assert abs(means[0] - l1[:4].mean()) <= 1e-15


def test_evaluate_keeps_its_end_points_without_the_flag(hip, golden_dir):
    """ISCNet.evaluate on the scene of tests/test_gpu_mesh_eval.py: without mesh_distance the end points are what they
    were; with it, 'mesh_distance' is the one key more"""
    from test_gpu_evaluation import labels_from_proposals
    from test_gpu_mesh_eval import CUBE_F, CUBE_V
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet import mesh_eval
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    fn = np.load(os.path.join(golden_dir, "F_NET.npz"))
    fnms = np.load(os.path.join(golden_dir, "F_NMS.npz"))
    seed, n_raw, n_pts = (int(v) for v in fn["pc_seed"])
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=seed, n_raw=n_raw, n_points=n_pts)[None]).cuda()
    cfg = Config({'generation': {'resolution_0': 8, 'upsampling_steps': 1}}, mean_size_arr=fnms['mean_size_arr'])
    net = ISCNet(cfg)
    for name, s in (('backbone', 101), ('voting', 102), ('detection', 103), ('skip_propagation', 104),
                    ('completion', 105)):
        synthetic.load_seeded(getattr(net, name), s)
    net = net.cuda().eval()
    detect = net.detect

    def detect_like_the_fixture(point_clouds):
        ep, pf = detect(point_clouds)
        ep['objectness_scores'] = torch.from_numpy(fnms['objectness_scores']).cuda()
        ep['size_residuals_normalized'] = ep['size_residuals_normalized'] * 0.2
        return ep, pf
    net.detect = detect_like_the_fixture
    end_points, ids, meshes = net.generate({'point_clouds': pc}, selection='nms')
    before = set(end_points)
    labels, n_gt = labels_from_proposals(end_points['parsed_predictions'], end_points['pred_mask'], fnms['mean_size_arr'])
    data = dict(labels, point_clouds=pc, gt_meshes=[(CUBE_V, CUBE_F)] * n_gt)
    off, _, _, _ = net.evaluate(data, fit=False, mesh_distance=False)
    assert set(off) == before and 'mesh_distance' not in off
    on, ids2, meshes2, _ = net.evaluate(data, fit=False, mesh_distance=True, distance_samples=500)
    assert set(on) == before | {'mesh_distance'}
    md = on['mesh_distance']
    P = ids2.shape[1]
    assert set(md) == set(mesh_eval.METRIC_KEYS) | {'pairs'} and tuple(md['pairs'].shape) == (P, 3)
    assert tuple(md['chamfer_l1'].shape) == (P,) and tuple(md['fscore'].shape) == (P, 2)
    has_faces = torch.tensor([int(m.faces.shape[0]) > 0 for m in meshes2], device="cuda")
    assert has_faces.any() and torch.isfinite(md['chamfer_l1'][has_faces]).all() and (md['chamfer_l1'][has_faces] > 0).all()
    assert torch.isnan(md['chamfer_l1'][~has_faces]).all()
    assert hip.stream_status_bits() == 0


# 10 ------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from rfdnet_amd.mesh_distance import MeshDistance, mesh_metrics, segment_sums
    lib = hip.lib()
    assert lib.rfd_mdist_faces(-1, 1, 3, *[None] * 12, None) != 0
    assert lib.rfd_mdist_faces(1, 0, 3, *[None] * 12, None) != 0
    assert lib.rfd_mdist_cells(-1, None, 1, None, None, None) != 0
    assert lib.rfd_mdist_query(-1, None, None, 1, 1, *[None] * 13, None) != 0
    assert lib.rfd_mdist_query(1, None, None, 1, 1, *[None] * 13, None) != 0                    # null pointers
    assert lib.rfd_mdist_sample(-1, 1, 1, *[None] * 7, None) != 0
    assert lib.rfd_mdist_sample(1, -1, 1, *[None] * 7, None) != 0
    assert lib.rfd_mdist_sums(-1, 0, 0, *[None] * 5, 0, *[None] * 3, None) != 0
    assert lib.rfd_mdist_sums(1, 0, 0, *[None] * 5, 9, *[None] * 3, None) != 0                 # more than 8 thresholds
    assert b"rfd_mdist_sums" in lib.rfd_last_error_string()
    v, f = M.TRIANGLE
    vt, ft = cuda(v), cuda(f, np.int32)
    for cells in (0, 65):
        with pytest.raises(ValueError, match="cells"):
            MeshDistance(vt, ft, cells=cells)
    md = MeshDistance(vt, ft)
    with pytest.raises(ValueError, match="thresholds"):
        mesh_metrics(md, md, [[0, 0]], count=10, thresholds=tuple(0.01 * i for i in range(9)))
    seg = cuda(np.array([0, 0]), np.int32)
    with pytest.raises(ValueError, match="thresholds"):
        segment_sums(md, seg, torch.zeros(0, dtype=torch.float64, device="cuda"),
                     torch.zeros(0, dtype=torch.int32, device="cuda"), None, range(9))
    v2, f2, vend, tend = C.batch([M.TRIANGLE, M.TRIANGLE])
    for bad_v, bad_t in (([0, 4, 3], tend), (vend, [0, 2, 1]), ([1, 3, 6], tend), (vend, tend[:2]), (vend, [0, 1, 3])):
        with pytest.raises(ValueError):
            MeshDistance(cuda(v2), cuda(f2, np.int32), bad_v, bad_t)
    with pytest.raises(ValueError):
        md.query(cuda(np.zeros((2, 3))), cuda(np.array([0, 1]), np.int32))                       # an object outside the batch
    with pytest.raises(ValueError):
        mesh_metrics(md, md, [[0, 1]], count=10)
    assert hip.stream_status_bits() == 0


# the tally -----------------------------------------------------------------------------------------------------------
def test_report_the_tally_of_the_file(hip):
    print("mesh distance: %d float64 values compared with the restatement, %d not bit-equal, largest difference %d ulp"
          % (TALLY['values'], TALLY['unequal'], TALLY['max_ulp']))
    assert TALLY['values'] > 0 and TALLY['unequal'] == 0 and TALLY['max_ulp'] == 0
