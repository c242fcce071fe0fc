"""CPU: vertex normals from the occupancy field's gradient (Generator3D(with_normals=True)) -- construction, binding,
config, PLY output, demo flag, and the F_NRM fixture against the float64 gradient (tests/normals_f64.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_with_normals_constructs_and_the_rest_still_raises():
    from rfdnet_amd.iscnet.generator import Generator3D
    g = Generator3D(None, with_normals=True)
    assert g.with_normals and g.last_normals is None
    with pytest.raises(NotImplementedError):
        Generator3D(None, with_normals=True, refinement_step=3)
    with pytest.raises(NotImplementedError):
        Generator3D(None, with_normals=True, simplify_nfaces=1000)


def test_normals_entry_point_is_declared_and_bound():
    from rfdnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "rfd_occ.h")).read()
    assert "int rfd_occ_normals_w8(" in src
    assert len(_lib.SIGNATURES["rfd_occ_normals_w8"]) == 15
    assert "rfd_occ_normals_w8" in _lib.exported_symbols()


def test_fixture_reference_normals_agree_with_the_float64_gradient():
    """F_NRM (the reference's estimate_normals, fp32 autograd on the CPU) vs the float64 restatement: the fixture and the
    helper check each other.  Vertices where fp32 itself is > 1e-4 from float64 are the contract's exception set."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from normals_f64 import input_grad, normals_of
    from seeded import decoder_arrays
    fx = np.load(os.path.join(ROOT, "tests", "golden", "F_NRM.npz"))
    sd = decoder_arrays(np.load(os.path.join(ROOT, "tests", "golden", "F_GEN.npz")), int(fx["seed"]))
    vend = fx["vend"]
    err = []
    for k in range(len(vend) - 1):
        v = fx["verts"][vend[k]:vend[k + 1]].astype(np.float32)[None]
        z = np.zeros((1, sd["fc_z.weight"].shape[1]), np.float32)
        c = fx["codes"][k][None]
        n64 = normals_of(input_grad(sd, v, z, c))[0]
        n32 = normals_of(input_grad(sd, v, z, c, dtype=__import__("torch").float32))[0]
        ref = fx["normals"][vend[k]:vend[k + 1]]
        d32 = np.abs(n32 - ref).max(-1)          # two fp32 evaluations: equal but where a ReLU sits on its kink
        assert (d32 > 1e-4).mean() < 0.01, (d32 > 1e-4).sum()
        err.append(np.abs(ref - n64).max(-1))
    err = np.concatenate(err)
    print("F_NRM: %d vertices, reference fp32 vs float64: max %.2e, %d above 1e-4, median %.2e"
          % (err.size, err.max(), int((err > 1e-4).sum()), np.median(err)))
    assert np.isfinite(err).all()
    assert (err > 1e-4).mean() < 0.01


def test_ply_round_trip_with_normals_and_byte_identical_without(tmp_path):
    from rfdnet_amd import io
    rng = np.random.default_rng(0)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    f = rng.integers(0, 50, size=(80, 3)).astype(np.int32)
    n = rng.normal(size=(50, 3)).astype(np.float32)
    p = str(tmp_path / "n.ply")
    io.write_mesh_ply(p, v, f, normals=n)
    head = open(p, "rb").read().split(b"end_header\n")[0].decode()
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face" in head
    v2, f2, n2 = io.read_mesh_ply(p, return_normals=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(n2, n)
    v3, f3 = io.read_mesh_ply(p)
    assert np.array_equal(v3, v) and np.array_equal(f3, f)
    # without normals: the writer's old byte layout, exactly
    q = str(tmp_path / "plain.ply")
    io.write_mesh_ply(q, v, f)
    header = ("ply\nformat binary_little_endian 1.0\ncomment rfdnet_amd\nelement vertex %d\n"
              "property float x\nproperty float y\nproperty float z\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (50, 80))
    rec = np.empty(80, dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    assert open(q, "rb").read() == header.encode("ascii") + v.astype('<f4').tobytes() + rec.tobytes()
    assert io.read_mesh_ply(q, return_normals=True)[2] is None


def test_save_visualization_writes_normals_when_a_mesh_has_them(tmp_path):
    from rfdnet_amd import io
    from rfdnet_amd.iscnet.generator import Mesh
    v = np.eye(3, dtype=np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    n = np.full((3, 3), 0.5, np.float32)
    io.save_visualization(str(tmp_path), np.zeros((1, 4, 3), np.float32), [4, 7], [Mesh(v, f, n), Mesh(v, f)])
    assert np.array_equal(io.read_mesh_ply(str(tmp_path / "proposal_4_mesh.ply"), return_normals=True)[2], n)
    assert io.read_mesh_ply(str(tmp_path / "proposal_7_mesh.ply"), return_normals=True)[2] is None


def test_onet_reads_generation_with_normals():
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.occupancy_net import ONet
    assert ONet(Config({'generation': {'with_normals': True}})).generator.with_normals is True
    assert ONet(Config({})).generator.with_normals is False          # the defaults table has no such key


def test_demo_with_normals_flag_parses():
    sys.path.insert(0, ROOT)
    import demo
    assert demo.build_parser().parse_args(["--synthetic", "10", "--with_normals"]).with_normals is True
    assert demo.build_parser().parse_args([]).with_normals is False
