"""CPU: the restatement of the mesh simplification (tests/simplify_f64.py) against the invariants of rules S0-S7
(include/rfd_simplify.h) on every shape of tests/simplify_cases.py, the guards of rfdnet_amd.iscnet.simplify and of the
layers above it that need no GPU, and the quality of the result against the reference's simplifier and the project's
clustering decimation (tests/golden/F_SIMPLIFY.npz, written by tests/golden/make_simplify_fixtures.py).  The kernels are
compared with the same restatement in tests/test_gpu_simplify.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_cases as C  # noqa: E402
import simplify_f64 as S  # noqa: E402

QUALITY_SAMPLES = 1000          # points drawn on a result (seed 7), as many as the fixture holds per surface


# ----------------------------------------------------------------------------------------------------- invariants ----
@pytest.mark.parametrize("name", list(C.CASES))
def test_the_selected_edges_of_every_round_have_disjoint_stars(name):
    out, trace = C.restated(name)
    assert len(trace) == out['rounds'] or (len(trace) == out['rounds'] - 1 and not out['reached'])
    for kept in trace:
        seen = set()
        for a, b, star in kept:
            assert a < b and not (star & seen), (name, a, b)
            seen |= star


@pytest.mark.parametrize("name", C.CLOSED)
def test_a_closed_manifold_stays_one(name):
    (v, f), target = C.CASES[name]
    out, _ = C.restated(name)
    assert C.is_closed_oriented_manifold(f) and C.is_closed_oriented_manifold(out['f'])
    assert C.euler(out['f']) == C.euler(f) == (0 if name == 'torus' else 2)
    assert np.isfinite(out['v']).all()


@pytest.mark.parametrize("name", list(C.CASES))
def test_faces_targets_and_compaction(name):
    (v, f), target = C.CASES[name]
    out, _ = C.restated(name)
    assert C.no_degenerate_or_duplicate_face(out['f'])
    if len(out['f']):
        assert sorted(set(out['f'].reshape(-1).tolist())) == list(range(len(out['v'])))      # every vertex is named
    if out['reached'] and len(f) > target:
        assert len(out['f']) in (target - 1, target)
    expected = {'tetrahedron': False, 'two_tetrahedra': False}
    if name in expected:                                                                     # no legal collapse exists
        assert not out['reached'] and np.array_equal(out['f'], f) and np.array_equal(out['v'], v)
    if name in C.CLOSED and name != 'tetrahedron':
        assert out['reached'] and len(out['f']) == target


@pytest.mark.parametrize("name", ['patch', 'folded_strip', 'two_tetrahedra', 'bad_input'])
def test_frozen_and_border_vertices_keep_their_exact_coordinates(name):
    (v, f), target = C.CASES[name]
    out, _ = C.restated(name)
    st = S.State(v, f)
    frozen = [i for i, fr in enumerate(st.edges()[2]) if fr and any(t is not None and i in t for t in st.face)]
    border = [i for i in C.border_vertices([t for t in st.face if t is not None])]
    assert set(border) <= set(frozen) and len(frozen) >= 4
    kept = set(np.ascontiguousarray(row).tobytes() for row in out['v'])
    for i in frozen:
        assert np.ascontiguousarray(v[i], np.float64).tobytes() in kept, (name, i)
    if name == 'bad_input':
        assert len(out['f']) < len(f) - 3 and np.isnan(out['v']).sum() == 1
    if name == 'patch':
        assert out['reached'] and len(out['f']) < len(f)


def test_a_mesh_at_or_under_its_target_comes_back_bit_for_bit():
    v, f = C.bad_input()
    out = S.simplify(v, f, len(f))
    assert np.array_equal(out['f'], f) and out['v'].tobytes() == v.tobytes() and out['reached'] and out['rounds'] == 0


# ------------------------------------------------------------------------------------------------ the cases bite ----
def test_without_the_flip_guard_the_folded_strip_comes_out_differently():
    (v, f), target = C.CASES['folded_strip']
    with_guard = C.restated('folded_strip')[0]
    without = S.simplify(v, f, target, flip_guard=False)

    def worst_turn(out):
        """the least cosine between a face's normal and the normal of the fold's side it lies on"""
        x = out['v'][out['f']]
        n = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        side = np.sign(x[:, :, 0].mean(1) - 0.4)
        want = np.stack([-0.5 * side, np.zeros_like(side), np.ones_like(side)], -1) / np.sqrt(1.25)
        return float((n * want).sum(1).min())
    assert not (with_guard['f'].shape == without['f'].shape and np.array_equal(with_guard['f'], without['f'])
                and np.array_equal(with_guard['v'], without['v']))
    print("least cosine to the fold's side: %.3f with the guard, %.3f without" % (worst_turn(with_guard), worst_turn(without)))
    assert worst_turn(with_guard) > 0 > worst_turn(without)              # without it a face is turned over


def test_without_the_link_condition_the_torus_is_pinched():
    v, f = C.torus()
    kept = S.simplify(v, f, 16)
    pinched = S.simplify(v, f, 16, link_condition=False)
    assert C.is_closed_oriented_manifold(kept['f']) and C.euler(kept['f']) == 0 and not kept['reached']
    assert not C.is_closed_oriented_manifold(pinched['f']) or C.euler(pinched['f']) != 0


# -------------------------------------------------------------------------------------------------------- guards ----
def test_the_guards_of_the_device_entry_need_no_gpu():
    from rfdnet_amd.iscnet.simplify import simplify_mesh, simplify_meshes
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="n_faces"):
        simplify_meshes(v, f, [0, 3], [0, 1], -1)
    with pytest.raises(ValueError, match="n_faces"):
        simplify_meshes(v, f, [0, 3], [0, 1], [1, 2])
    with pytest.raises(TypeError, match="n_faces"):
        simplify_meshes(v, f, [0, 3], [0, 1], 0.5)
    with pytest.raises(ValueError, match="vend"):
        simplify_meshes(v, f, [1, 3], [0, 1], 1)
    with pytest.raises(ValueError, match="meshes"):
        simplify_meshes(v, f, [0, 3], [0, 1, 1], 1)
    with pytest.raises(ValueError, match="max_rounds"):
        simplify_meshes(v, f, [0, 3], [0, 1], 1, max_rounds=-1)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        simplify_meshes(v, f, [0, 3], [0, 1], 0)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        simplify_mesh(v, f, 0)


def test_the_generator_switch_and_the_config_key():
    from rfdnet_amd.iscnet.config import DEFAULT_CONFIG, Config
    from rfdnet_amd.iscnet.generator import Generator3D
    from rfdnet_amd.iscnet.occupancy_net import ONet
    assert 'simplify_faces' not in DEFAULT_CONFIG['generation']         # every default is a key of the reference's file
    assert ONet(Config({})).generator.simplify_faces == 0
    g = ONet(Config({'generation': {'simplify_faces': 500}})).generator
    assert g.simplify_faces == 500 and g.simplify_nfaces is None
    assert g.set_simplification(None) is g and g.simplify_faces == 0
    assert g.set_simplification(80).simplify_faces == 80 and g.set_simplification(0).simplify_faces == 0
    assert g.set_decimation(8).set_simplification(80).decimate_cells == 8
    with pytest.raises(ValueError):
        g.set_simplification(-1)
    with pytest.raises(NotImplementedError):                             # the constructor's guard stays as it is
        Generator3D(None, simplify_nfaces=1000)


def test_the_demo_and_the_tool_have_the_flag():
    import demo
    assert demo.build_parser().parse_args(["--simplify_nfaces", "500"]).simplify_nfaces == 500
    assert demo.build_parser().parse_args([]).simplify_nfaces is None
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import simplify_mesh as tool
    args = tool.build_parser().parse_args(["in.off", "out.off"])
    assert (args.input, args.output, args.n_faces) == ("in.off", "out.off", 10000)
    assert tool.build_parser().parse_args(["a.obj", "b.off", "--n_faces", "64"]).n_faces == 64
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(["only_one.off"])


def test_the_tool_falls_back_to_its_input_when_the_result_is_not_watertight():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import simplify_mesh as tool
    v, f = (torch.from_numpy(a) for a in C.octahedron())
    open_v, open_f = v[:5], f[:4]                                        # the upper half only: four border edges
    (cv, cf), report = tool.choose(v, f, open_v, open_f)
    assert cv is v and cf is f and report["fallback"] and not report["watertight"]
    (cv, cf), report = tool.choose(open_v, open_f, v, f)
    assert cv is v and cf is f and not report["fallback"] and report["watertight"]
    assert report["faces_in"] == 4 and report["faces_out"] == 8


# ------------------------------------------------------------------------------------------------------- quality ----
def assert_quality(fx, name, v2, f2):
    """E = the RMS of the exact point-to-triangle distances from QUALITY_SAMPLES fixed points on the input to the result
    and from as many on the result to the input (float64 numpy).  E_r: of the reference's mesh_simplify, E_c: of the
    clustering decimation at the cell count whose face count is the target (both in the fixture, E_r < E_c), E_o: of
    (v2, f2).  No worse than what the project had, and closer to the reference than to that."""
    E_r, E_c = float(fx[name + "_E_r"]), float(fx[name + "_E_c"])
    assert E_r < E_c
    samples = C.surface_samples(v2, f2, QUALITY_SAMPLES, seed=7)
    E_o = C.two_sided_rms(fx[name + "_v"], fx[name + "_f"], fx[name + "_s_in"], v2, f2, samples)
    print("%s: %d -> %d faces (target %d): E_r %.6g  E_c %.6g  E_o %.6g" % (name, len(fx[name + "_f"]), len(f2),
                                                                          int(fx[name + "_target"]), E_r, E_c, E_o))
    assert len(f2) <= int(fx[name + "_target"])
    assert E_o <= E_c
    assert E_o <= (E_r + E_c) / 2


def test_quality_against_the_reference_and_the_clustering(golden_dir):
    fx = np.load(os.path.join(golden_dir, "F_SIMPLIFY.npz"))
    for name in [str(n) for n in fx["names"]]:
        out = S.simplify(fx[name + "_v"], fx[name + "_f"], int(fx[name + "_target"]))
        assert out['reached'] and C.is_closed_oriented_manifold(out['f'])
        assert_quality(fx, name, out['v'], out['f'])
