"""CPU: the numpy restatement of the fusion's rules (tests/fuse_ref.py) against what the reference's CPU fusion wrote
(tests/golden/F_FUSE.npz, made by tests/golden/make_fuse_fixture.py), the view rotations, and the two mesh formats that
came with the watertight path (write_off, read_obj)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "F_FUSE.npz"))


@pytest.mark.parametrize("unknown_is_free", [0, 1])
def test_restatement_equals_the_reference_fusion(fixture, unknown_is_free):
    z = fixture
    tsdf, count = fuse_ref.fuse(z['depth'], z['K'], z['R'], z['T'], z['shape'], z['vx_size'], z['truncation'],
                                unknown_is_free, -z['truncation'])
    want, mask = z['tsdf_free%d' % unknown_is_free], z['mask_free%d' % unknown_is_free]
    assert tuple(z['shape']) == (11, 20, 15) and tsdf.shape == want.shape and tsdf.dtype == np.float32
    assert set(np.unique(count)) == set(range(6))                    # every count from no view to all five
    np.testing.assert_array_equal(tsdf.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(count > 0, mask > 0)
    # the merged field of the pipeline (tsdf[mask == 0] = truncation) is the same pass with the other fill value
    merged, _ = fuse_ref.fuse(z['depth'], z['K'], z['R'], z['T'], z['shape'], z['vx_size'], z['truncation'],
                              unknown_is_free, z['truncation'])
    np.testing.assert_array_equal(merged, np.where(mask > 0, want, z['truncation']))


def test_the_fixture_has_unknown_pixels_of_both_kinds(fixture):
    d = fixture['depth']
    assert d.shape == (5, 40, 56) and (d == -1).mean() > 0.01 and (d == 0).mean() > 0.01
    assert not np.array_equal(fixture['tsdf_free0'], fixture['tsdf_free1'])
    assert fixture['K'][0, 2] != fixture['K'][0, 5]                  # cx != cy


def test_views_on_sphere(fixture):
    from rfdnet_amd.watertight import views_on_sphere
    R = views_on_sphere(7)
    assert R.shape == (7, 3, 3) and R.dtype == np.float64
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), R.shape), atol=1e-14)
    np.testing.assert_allclose(np.linalg.det(R), 1., atol=1e-14)
    np.testing.assert_allclose(R[0].reshape(-1), fixture['R'][0], atol=1e-7)
    # the first view point of the spiral is (cos phi r, 2/7/2 - 1, sin phi r) with phi = the golden angle: its rotation
    # is R_y(-atan2(x, y)) R_x(atan2(z, |xy|)), written out here independently for that one point
    phi, y = np.pi * (3 - np.sqrt(5)), 1. / 7 - 1
    r = np.sqrt(1 - y * y)
    x, z = np.cos(phi) * r, np.sin(phi) * r
    lon, lat = -np.arctan2(x, y), np.arctan2(z, np.hypot(x, y))
    ry = np.array([[np.cos(lon), 0, np.sin(lon)], [0, 1, 0], [-np.sin(lon), 0, np.cos(lon)]])
    rx = np.array([[1, 0, 0], [0, np.cos(lat), -np.sin(lat)], [0, np.sin(lat), np.cos(lat)]])
    np.testing.assert_allclose(R[0], ry @ rx, atol=1e-15)
    assert views_on_sphere(200).shape == (200, 3, 3) and len({tuple(np.round(m.reshape(-1), 9)) for m in views_on_sphere(200)}) == 200


def test_erosion_is_the_edge_clamped_minimum():
    a = np.random.default_rng(0).normal(0, 1, (5, 7)).astype(np.float32)
    got = fuse_ref.erode3(a)
    for j in range(5):
        for i in range(7):
            assert got[j, i] == a[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].min()
    keys = np.array([[0, (np.float32(2.).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(5)],
                     [(np.float32(0.25).view(np.uint32).astype(np.uint64) << np.uint64(32)), 0]], np.uint64)
    np.testing.assert_array_equal(fuse_ref.key_depth(keys, 1.75), np.array([[1.75, 0.5], [1.75, 1.75]], np.float32))
    np.testing.assert_array_equal(fuse_ref.depth_from_keys(keys, 1.75, 0.125), np.full((2, 2), 0.375, np.float32))


def test_write_off_round_trips_through_read_off(tmp_path):
    from rfdnet_amd import io
    rng = np.random.default_rng(1)
    v = rng.normal(0, 1, (9, 3)) * 10. ** rng.integers(-8, 8, (9, 1))
    f = rng.integers(0, 9, (5, 3)).astype(np.int32)
    path = str(tmp_path / "m.off")
    io.write_off(path, v, f)
    v2, f2 = io.read_off(path)
    np.testing.assert_array_equal(v2, v)                              # float64, exactly
    assert f2 == f.tolist()
    io.write_off(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v2, f2 = io.read_off(path)
    assert v2.shape == (0, 3) and f2 == []


def test_read_obj(tmp_path):
    from rfdnet_amd import io
    path = str(tmp_path / "m.obj")
    with open(path, "w") as fh:
        fh.write("# a quad and a triangle\nmtllib none.mtl\nv 0 0 0\nv 1 0 0   # trailing comment\nv 1 1 0\nv 0 1 0\n"
                 "v 0.5 0.5 1e0\nvt 0 0\nvn 0 0 1\ng part\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf 1//1 2 5/1\n")
    v, f = io.read_obj(path)
    assert v.dtype == np.float64 and f.dtype == np.int32
    np.testing.assert_array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]])
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 1, 4]])
    with open(path, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 1 1 0\nf -3 -2 -1\n")
    with pytest.raises(ValueError, match="negative"):
        io.read_obj(path)
    with open(path, "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="names vertex"):
        io.read_obj(path)
