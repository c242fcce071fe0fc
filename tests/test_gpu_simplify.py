"""GPU (-m gpu): mesh simplification on the device (rfdnet_amd/iscnet/simplify.py, csrc/mesh_simplify.hip) against the
restatement of its rules S0-S7 (tests/simplify_f64.py) on the shapes of tests/simplify_cases.py.

Offsets and faces must be EQUAL and every vertex coordinate BIT-EQUAL: both sides perform the same f64 operations in the
same order (divisions and square roots are correctly rounded on both), and a cost that differed in its last place could
change the order of the collapses, so nothing less would hold either."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_cases as C  # noqa: E402
import simplify_f64 as S  # noqa: E402
from seeded import seeded_onet  # noqa: E402

pytestmark = pytest.mark.gpu


def on_device(v, f, vend, tend, n_faces, dtype=np.float64, **kw):
    """simplify_meshes on numpy inputs -> (v2 f64, f2 int64, vend2, tend2, reached) as numpy / lists"""
    from rfdnet_amd.iscnet.simplify import simplify_meshes
    vt = torch.from_numpy(np.array(v, dtype=dtype).reshape(-1, 3)).cuda()            # a copy: the cases stay unchanged
    ft = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).cuda()
    v2, f2, vend2, tend2, reached = simplify_meshes(vt, ft, vend, tend, n_faces, **kw)
    assert v2.dtype == torch.float64 and f2.dtype == torch.int32 and v2.is_cuda and f2.is_cuda
    assert tuple(v2.shape) == (vend2[-1], 3) and tuple(f2.shape) == (tend2[-1], 3)
    assert reached.dtype == torch.bool and tuple(reached.shape) == (len(vend) - 1,)
    return v2.cpu().numpy(), f2.cpu().numpy().astype(np.int64), vend2, tend2, reached.numpy()


def one(v, f, n_faces, **kw):
    return on_device(v, f, [0, len(v)], [0, len(f)], n_faces, **kw)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_mesh(name, got, k, want):
    """mesh k of a device result equals a restatement's dict"""
    v2, f2, vend2, tend2, reached = got
    vs, fs = slice(vend2[k], vend2[k + 1]), slice(tend2[k], tend2[k + 1])
    assert f2[fs].shape == want['f'].shape and np.array_equal(f2[fs], want['f']), name
    assert v2[vs].shape == want['v'].shape, name
    unequal = int((bits(v2[vs]) != bits(want['v'])).sum())
    print("%s: %d vertices, %d faces, %d of %d coordinates not bit-equal" % (name, len(want['v']), len(want['f']), unequal,
                                                                             want['v'].size))
    assert unequal == 0, name
    assert bool(reached[k]) == want['reached'], name


@pytest.fixture(scope="module")
def whole_batch():
    names = list(C.CASES)
    v, f, vend, tend = C.batch([C.CASES[n][0] for n in names])
    return names, on_device(v, f, vend, tend, [C.CASES[n][1] for n in names])


# 1 -------------------------------------------------------------------------------------------------------------------
def test_the_ragged_batch_of_all_cases_equals_the_restatement(hip, whole_batch):
    names, got = whole_batch
    hip.device_status()
    for k, name in enumerate(names):
        assert_mesh(name, got, k, C.restated(name)[0])


def test_f32_vertices_are_widened(hip):
    (v, f), target = C.CASES['icosphere320']
    v32 = v.astype(np.float32)
    a, b = one(v32, f, target, dtype=np.float32), one(v32.astype(np.float64), f, target)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[3] == b[3] == [0, target]
    assert_mesh("f32 icosphere", a, 0, S.simplify(v32, f, target))


def test_a_mesh_alone_equals_itself_in_the_batch_and_two_calls_are_equal(hip, whole_batch):
    names, got = whole_batch
    for name in ('torus', 'icosphere1280'):
        k = names.index(name)
        (v, f), target = C.CASES[name]
        alone = one(v, f, target)
        assert np.array_equal(bits(alone[0]), bits(got[0][got[2][k]:got[2][k + 1]]))
        assert np.array_equal(alone[1], got[1][got[3][k]:got[3][k + 1]]) and alone[4][0] == got[4][k]
    v, f, vend, tend = C.batch([C.CASES[n][0] for n in names])
    again = on_device(v, f, vend, tend, [C.CASES[n][1] for n in names])
    assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(again[1], got[1])
    assert again[2:4] == got[2:4] and np.array_equal(again[4], got[4])


def test_empty_meshes_at_the_head_and_twice_in_a_row(hip):
    """[empty, tetrahedron, empty, empty, octahedron] to six faces: offsets that begin with a repeat and repeat twice in the
    middle, the inputs of the search for the mesh of a vertex or face.  Only the octahedron takes part."""
    meshes = [C.EMPTY, C.tetrahedron(), C.EMPTY, C.EMPTY, C.octahedron()]
    v, f, vend, tend = C.batch(meshes)
    got = on_device(v, f, vend, tend, 6)
    hip.device_status()
    assert_mesh("octahedron behind empties", got, 4, C.restated('octahedron')[0])
    assert got[3][5] - got[3][4] == 6
    for k in range(4):                                                  # as they went in
        mv, mf = meshes[k]
        assert_mesh("mesh %d" % k, got, k, S.simplify(mv, mf, 6))
        vs, fs = slice(got[2][k], got[2][k + 1]), slice(got[3][k], got[3][k + 1])
        assert np.array_equal(bits(got[0][vs]), bits(mv)) and np.array_equal(got[1][fs], mf) and got[4][k]


# 5 -------------------------------------------------------------------------------------------------------------------
def test_targets_from_one_collapse_to_none(hip):
    (v, f), _ = C.CASES['icosphere320']
    F = len(f)
    targets = [F - 2, F - 3, 250, 161, 40, F, F + 7]
    vb, fb, vend, tend = C.batch([(v, f)] * len(targets))
    got = on_device(vb, fb, vend, tend, targets)
    hip.device_status()
    for k, t in enumerate(targets):
        faces = got[3][k + 1] - got[3][k]
        if t >= F:                                                      # returned bitwise
            assert faces == F and np.array_equal(got[1][got[3][k]:got[3][k + 1]], f)
            assert np.array_equal(bits(got[0][got[2][k]:got[2][k + 1]]), bits(v)) and got[4][k]
        else:
            assert_mesh("target %d" % t, got, k, S.simplify(v, f, t))
            assert got[4][k] and faces in (t - 1, t) and faces % 2 == 0     # a closed mesh loses two faces per collapse
    assert got[3][1] - got[3][0] == F - 2 and got[2][1] - got[2][0] == len(v) - 1


# 6 -------------------------------------------------------------------------------------------------------------------
def test_borders_frozen_parts_and_bad_input_obey_s0(hip, whole_batch):
    names, got = whole_batch
    hip.device_status()

    def result(name):
        k = names.index(name)
        return got[0][got[2][k]:got[2][k + 1]], got[1][got[3][k]:got[3][k + 1]], bool(got[4][k])
    for name in ('patch', 'folded_strip'):                              # every border vertex is still where it was
        (v, f), target = C.CASES[name]
        v2, f2, _ = result(name)
        border = C.border_vertices(f)
        assert len(border) > 20 and len(f2) < len(f)
        kept = set(map(bytes, bits(v2)))
        assert all(bytes(bits(v[i])) in kept for i in border)
        assert len(C.border_vertices(f2)) == len(border)
    (v, f), _ = C.CASES['two_tetrahedra']                               # every vertex lies on, or next to, the bad edge
    v2, f2, reached = result('two_tetrahedra')
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and not reached
    (v, f), _ = C.CASES['tetrahedron']
    v2, f2, reached = result('tetrahedron')
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and not reached
    (v, f), target = C.CASES['bad_input']
    v2, f2, reached = result('bad_input')
    assert reached and len(f2) <= target and f2.min() == 0 and f2.max() == len(v2) - 1
    assert np.isnan(v2).sum() == 1 and C.no_degenerate_or_duplicate_face(f2)      # the NaN vertex is frozen, and still named
    v2, f2, reached = result('empty')
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and reached


# 7 -------------------------------------------------------------------------------------------------------------------
def test_the_c_entries_refuse_what_they_cannot_index(hip):
    """the launchers' own argument checks (nothing is launched): counts, 3 F past int32, a null pointer"""
    dev = torch.device("cuda", 0)
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    calls = {
        "rfd_simplify_init": lambda V, F, K, q: (V, F, K, 0, p, p, p, p, p, p, p, q),
        "rfd_simplify_quadrics": lambda V, F, K, q: (V, F, p, p, p, p, q),
        "rfd_simplify_edges": lambda V, F, K, q: (V, F, p, p, p, p, p, p, p, p, q),
        "rfd_simplify_edge_costs": lambda V, F, K, q: (V, F, K, p, p, p, p, p, p, p, p, p, p, p, p, p, p, q),
        "rfd_simplify_vertex_min": lambda V, F, K, q: (V, F, 0, p, p, p, p, p, q),
        "rfd_simplify_select": lambda V, F, K, q: (V, F, p, p, p, p, p, q),
        "rfd_simplify_apply": lambda V, F, K, q: (V, F, p, p, p, p, p, p, p, p, p, q),
        "rfd_simplify_compact_faces": lambda V, F, K, q: (V, F, K, p, p, p, p, p, p, p, p, p, q),
    }
    for name, args in calls.items():
        for V, F in ((0, 1), (-1, 1), (1, 0), (1, -5), (1, 2 ** 30)):
            with pytest.raises(hip.RfdHipError, match="3 F"):
                hip.call(name, dev, *args(V, F, 1, p))
        with pytest.raises(hip.RfdHipError, match="null"):
            hip.call(name, dev, *args(1, 1, 1, None))
    for name in ("rfd_simplify_init", "rfd_simplify_edge_costs", "rfd_simplify_compact_faces"):
        with pytest.raises(hip.RfdHipError, match="K must be positive"):
            hip.call(name, dev, *calls[name](1, 1, 0, p))
    with pytest.raises(hip.RfdHipError, match="pass"):
        hip.call("rfd_simplify_vertex_min", dev, 1, 1, 2, p, p, p, p, p, p)
    hip.device_status()


# 8 -------------------------------------------------------------------------------------------------------------------
def test_the_generator_simplifies_before_normals_and_refinement(hip, golden_dir):
    """the fixture's three meshes (3 464, 2 524, 3 464 faces) are boxes of a seeded network whose marching cubes leaves more
    than a tenth of the faces with no area; under the reference's flip guard nothing takes them below 782 / 204 / 786 faces
    (the reference's own mesh_simplify stops at 778 / 258 / 778), so the budget here is 1 000"""
    from rfdnet_amd.mesh_sample import is_watertight
    fx = np.load(os.path.join(golden_dir, "F_GEN.npz"))
    codes = torch.from_numpy(fx["codes"]).cuda()
    budget = 1000

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
    g1, thin = generate(lambda g: full(g).set_simplification(budget))
    v0, f0, vend0, tend0 = g0.last_buffers
    v1, f1, vend1, tend1 = g1.last_buffers
    K = codes.shape[0]
    assert len(plain) == len(thin) == K and max(np.diff(tend0)) > budget
    assert len(vend1) == len(tend1) == K + 1 and vend1[0] == tend1[0] == 0
    assert tuple(v1.shape) == (vend1[-1], 3) and tuple(f1.shape) == (tend1[-1], 3)
    assert v1.dtype == torch.float32 and torch.isfinite(v1).all()             # refined: refine_meshes returns f32
    assert tuple(g1.last_normals.shape) == (vend1[-1], 3)                     # the normals of the simplified vertices
    for k, m in enumerate(thin):
        before, after = tend0[k + 1] - tend0[k], tend1[k + 1] - tend1[k]
        nv = vend1[k + 1] - vend1[k]
        tight0 = is_watertight(f0[tend0[k]:tend0[k + 1]])
        print("mesh %d: %d -> %d faces, watertight %s" % (k, before, after, tight0))
        if before <= budget:
            assert after == before and nv == vend0[k + 1] - vend0[k]
        else:
            assert after in (budget - 1, budget), (k, before, after)          # at its budget
        assert is_watertight(f1[tend1[k]:tend1[k + 1]]) == tight0
        assert tuple(m.vertices.shape) == (nv, 3) and tuple(m.faces.shape) == (after, 3)
        if nv:
            assert tuple(m.vertex_normals.shape) == (nv, 3)
            assert int(m.faces.min()) == 0 and int(m.faces.max()) == nv - 1
    # with both set the clustering runs first and the collapse takes its result to the budget, or leaves it where it is
    g3, _ = generate(lambda g: full(g).set_decimation(12))
    g4, _ = generate(lambda g: full(g).set_decimation(12).set_simplification(400))
    for k in range(K):
        clustered, both = g3.last_buffers[3][k + 1] - g3.last_buffers[3][k], g4.last_buffers[3][k + 1] - g4.last_buffers[3][k]
        print("mesh %d: clustering %d faces, then collapse %d" % (k, clustered, both))
        assert both <= clustered                                            # (a clustered mesh may hold frozen parts)
    assert tuple(g4.last_buffers[1].shape) == (g4.last_buffers[3][-1], 3) and g4.last_buffers[0].dtype == torch.float32
    # switched off again, the generator makes the calls it always made
    g2, again = generate(lambda g: full(g).set_simplification(budget).set_simplification(0))
    for a, b in zip(g0.last_buffers[:2], g2.last_buffers[:2]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert list(g0.last_buffers[2]) == list(g2.last_buffers[2]) and list(g0.last_buffers[3]) == list(g2.last_buffers[3])
    assert torch.equal(g0.last_normals, g2.last_normals)


# 9 -------------------------------------------------------------------------------------------------------------------
def test_quality_against_the_reference_and_the_clustering(hip, golden_dir):
    """E_o <= E_c and E_o <= (E_r + E_c) / 2 (tests/test_simplify_cpu.py says what they are), E_o of the device's result"""
    import test_simplify_cpu as T
    fx = np.load(os.path.join(golden_dir, "F_SIMPLIFY.npz"))
    names = [str(n) for n in fx["names"]]
    v, f, vend, tend = C.batch([(fx[n + "_v"], fx[n + "_f"]) for n in names])
    got = on_device(v, f, vend, tend, [int(fx[n + "_target"]) for n in names])
    for k, n in enumerate(names):
        v2, f2 = got[0][got[2][k]:got[2][k + 1]], got[1][got[3][k]:got[3][k + 1]]
        assert got[4][k] and C.is_closed_oriented_manifold(f2)
        T.assert_quality(fx, n, v2, f2)
