"""CPU: the numpy restatements of include/rfd_sample.h (tests/mesh_sample_ref.py) give the reference's own answers
(tests/golden/F_SMP.npz, made by tests/golden/make_sample_fixture.py from the reference's compiled code) with zero
differing elements; the binvox writer gives the reference's bytes; every refusal of rfdnet_amd.mesh_sample is raised on
host-side inputs, before a device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sample_cases as cases  # noqa: E402
import mesh_sample_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(cases.GOLDEN))


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize("name", cases.MESHES)
def test_fixture_meshes_are_the_cases(golden, name):
    v, f = cases.normalised(name)
    assert np.array_equal(golden[name + "_v"], v) and np.array_equal(golden[name + "_f"], f)
    assert golden["jitter"].shape == (cases.GRID ** 3, 3) and golden["uniform"].shape == (2000, 3)
    assert np.abs(golden["uniform"]).max() <= 0.55 and np.abs(golden["jitter"]).max() <= 0.05


@pytest.mark.parametrize("res", cases.HASH_RESOLUTIONS)
@pytest.mark.parametrize("name", cases.MESHES)
def test_containment_restatement_equals_the_reference(golden, name, res):
    v, f = golden[name + "_v"], golden[name + "_f"]
    points = cases.query_points(v, f, golden["jitter"], golden["uniform"])
    got, n0, n1 = ref.contains(v, f, points, res)
    want = unpack(golden["%s_contains_%d" % (name, res)], (len(points),))
    assert int((got != want).sum()) == 0
    assert want.any() and not want.all() and not got[-2:].any()          # the NaN point and the point at 10


@pytest.mark.parametrize("R", cases.SURFACE_RESOLUTIONS)
@pytest.mark.parametrize("name", cases.MESHES)
def test_surface_voxel_restatement_equals_the_reference(golden, name, R):
    got = ref.voxelize_surface(golden[name + "_v"], golden[name + "_f"], R)
    assert int((got != unpack(golden["%s_surface_%d" % (name, R)], (R, R, R))).sum()) == 0


@pytest.mark.parametrize("name", cases.MESHES)
def test_interior_and_ray_restatement_equals_the_reference(golden, name):
    R = cases.GRID
    v, f = golden[name + "_v"], golden[name + "_f"]
    interior = ref.voxelize_interior(v, f, R, golden["jitter"])
    assert int((interior != unpack(golden[name + "_interior"], (R, R, R))).sum()) == 0
    ray = interior | ref.voxelize_surface(v, f, R)
    assert int((ray != unpack(golden[name + "_ray"], (R, R, R))).sum()) == 0


def test_binvox_bytes_and_round_trip(golden, tmp_path):
    from rfdnet_amd import io
    R = cases.GRID
    grid = unpack(golden["sphere_ray"], (R, R, R))
    path = str(tmp_path / "a.binvox")
    io.write_binvox(path, grid, cases.BINVOX_TRANSLATE, cases.BINVOX_SCALE)
    with open(path, "rb") as fh:
        assert fh.read() == golden["binvox"].tobytes()
    back, translate, scale = io.read_binvox(path)
    assert np.array_equal(back, grid) and np.array_equal(translate, cases.BINVOX_TRANSLATE) and scale == cases.BINVOX_SCALE
    # runs of exactly 255 and 510 voxels, a grid that is no cube, a run that ends the file
    rng = np.random.default_rng(0)
    odd = np.zeros((5, 51, 6), bool)
    flat = np.zeros(odd.size, bool)
    flat[255:765] = True
    flat[800:] = rng.random(odd.size - 800) < 0.3
    odd[:] = np.transpose(flat.reshape(5, 6, 51), (0, 2, 1))
    io.write_binvox(path, odd, (0, 0, 0), 1)
    assert np.array_equal(io.read_binvox(path)[0], odd)
    raw = open(path, "rb").read().split(b"data\n", 1)[1]
    assert raw[:6] == bytes([0, 255, 0, 0, 1, 255])


def test_npz_writers_have_the_reference_keys(tmp_path):
    from rfdnet_amd import io
    p, n = np.random.default_rng(1).normal(size=(2, 21, 3))
    occ = p[:, 0] > 0
    io.write_points_npz(str(tmp_path / "points.npz"), p, occ, np.zeros(3), 1., float16=True, packbits=True)
    d = np.load(str(tmp_path / "points.npz"))
    assert sorted(d.files) == ["loc", "occupancies", "points", "scale"]
    assert d["points"].dtype == np.float16 and d["occupancies"].dtype == np.uint8 and d["occupancies"].shape == (3,)
    assert np.array_equal(np.unpackbits(d["occupancies"])[:21].astype(bool), occ)
    io.write_pointcloud_npz(str(tmp_path / "pointcloud.npz"), p, n, np.ones(3), 2.)
    d = np.load(str(tmp_path / "pointcloud.npz"))
    assert sorted(d.files) == ["loc", "normals", "points", "scale"]
    assert d["points"].dtype == np.float32 and d["normals"].dtype == np.float32 and float(d["scale"]) == 2.


def test_abi_names_the_entry_points():
    from rfdnet_amd import _lib
    for name in ("rfd_sample_rescale", "rfd_sample_cells", "rfd_sample_contains", "rfd_sample_voxelize",
                 "rfd_sample_face_areas", "rfd_sample_surface"):
        assert name in _lib.ABI, name


def test_refusals_need_no_device():
    from rfdnet_amd import mesh_sample as ms
    v, f = (torch.from_numpy(a) for a in cases.cube())
    p = torch.zeros(4, 3, dtype=torch.float64)
    # host tensors are refused as everywhere else ...
    for call in (lambda: ms.MeshIntersector(v, f), lambda: ms.check_mesh_contains(v, f, p),
                 lambda: ms.voxelize_surface(v, f, 16), lambda: ms.voxelize_interior(v, f, 16),
                 lambda: ms.voxelize_ray(v, f, 16), lambda: ms.sample_surface(v, f, 10),
                 lambda: ms.sample_points(v, f, 10)):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            call()
    # ... but a bad parameter is named first
    for res in (1, 0, -3, ms.MAX_HASH_RESOLUTION + 1):
        with pytest.raises(ValueError, match="hash_resolution"):
            ms.MeshIntersector(v, f, hash_resolution=res)
        with pytest.raises(ValueError, match="hash_resolution"):
            ms.check_mesh_contains(v, f, p, hash_resolution=res)
    for fn in (ms.voxelize_surface, ms.voxelize_interior, ms.voxelize_ray):
        for R in (0, -1, ms.MAX_VOXEL_RESOLUTION + 1):
            with pytest.raises(ValueError, match="resolution"):
                fn(v, f, R)
    # the mesh check is plain tensor code: it runs wherever the tensors live, and never gathers through a bad index
    tri, lo, hi = ms.mesh_triangles(v, f)
    assert np.array_equal(tri.numpy(), cases.cube()[0][cases.cube()[1]]) and np.array_equal(lo, [0.2] * 3)
    assert np.array_equal(hi, [0.8] * 3)
    for bad in (8, -1, 1 << 40):
        g = f.clone()
        g[5, 1] = bad
        with pytest.raises(ValueError, match="face indices"):
            ms.mesh_triangles(v, g)
    with pytest.raises(ValueError, match="integer faces"):
        ms.mesh_triangles(v, f.double())
    with pytest.raises(ValueError, match="empty vertex array"):
        ms.mesh_triangles(v[:0], f)
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.clone()
        w[3, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            ms.mesh_triangles(w, f)
    w = v.clone()
    w[7, 0] = float("nan")                      # a vertex that no face names is not the mesh's business
    ms.mesh_triangles(w, f[(f != 7).all(1)])
    assert ms.mesh_triangles(v, f[:0])[1] is None
    flat = v.clone()
    flat[:, 1] = 0.25
    with pytest.raises(ValueError, match="no extent"):
        ms.rescale_constants(*ms.mesh_triangles(flat, f)[1:], 512)
    scale, translate = ms.rescale_constants(lo, hi, 512)
    want = ref.rescale_constants(*cases.cube(), 512)
    assert np.array_equal(scale, want[0]) and np.array_equal(translate, want[1])
    with pytest.raises(ValueError, match="total area"):
        ms.check_total_area(0., 5)
    with pytest.raises(ValueError, match="total area"):
        ms.check_total_area(float("nan"), 1)
    ms.check_total_area(0., 0)
    with pytest.raises(ValueError, match="2\\^31"):
        ms.check_sizes(cell_triangle_pairs=1 << 31)
    ms.check_sizes(cell_triangle_pairs=(1 << 31) - 1)
    with pytest.raises(ValueError, match="count"):
        ms.sample_surface(v, f, -1)


def test_is_watertight_on_host_tensors():
    from rfdnet_amd import mesh_sample as ms
    for name in cases.MESHES:
        assert ms.is_watertight(torch.from_numpy(cases.normalised(name)[1]))
    f = torch.from_numpy(cases.cube()[1])
    assert not ms.is_watertight(f[1:]) and not ms.is_watertight(torch.cat([f, f[:1]])) and not ms.is_watertight(f[:0])


def test_unit_cube_gives_the_bits_of_the_numpy_lines_it_replaces(tmp_path):
    from rfdnet_amd import mesh_sample as ms
    v = cases.cube()[0] * 3.7 + np.array([0.3, -1.7, 2.1])
    lo, hi = v.min(0), v.max(0)
    loc, scale = (lo + hi) / 2, float((hi - lo).max())
    want = (v - loc) * (1 / scale)
    got, got_loc, got_scale = ms.unit_cube(torch.from_numpy(v))
    assert got.dtype == torch.float64 and got_loc.dtype == torch.float64 and type(got_scale) is float
    assert got.numpy().tobytes() == want.tobytes()
    assert got_loc.numpy().tobytes() == loc.tobytes() and got_scale == scale
    from rfdnet_amd import io                                                   # and so the .off the tool writes
    io.write_off(str(tmp_path / "got.off"), got.numpy(), cases.cube()[1])
    io.write_off(str(tmp_path / "want.off"), want, cases.cube()[1])
    assert (tmp_path / "got.off").read_bytes() == (tmp_path / "want.off").read_bytes()
