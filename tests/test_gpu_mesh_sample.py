"""GPU: rfdnet_amd.mesh_sample (csrc/mesh_sample.hip, the rules of include/rfd_sample.h).  Containment and the voxels are
compared by EQUALITY: with the reference's own answers (tests/golden/F_SMP.npz) and with the numpy restatement
tests/mesh_sample_ref.py, which tests/test_mesh_sample_cpu.py holds to that fixture."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sample_cases as cases  # noqa: E402
import mesh_sample_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(cases.GOLDEN))


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def device_contains(v, f, points, res=512, **kw):
    from rfdnet_amd.mesh_sample import MeshIntersector
    got = MeshIntersector(dev(v), dev(f), res).query(dev(points), return_counts=True, **kw)
    assert got[0].dtype == torch.bool and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in got)


def check_contains(v, f, points, res=512):
    """the device against the restatement, exactly: contains, n0, n1, sorted and unsorted -> the restatement's triple"""
    want = ref.contains(v, f, points, res)
    for sort_points in (False, True):
        got = device_contains(v, f, points, res, sort_points=sort_points)
        print("res %d sorted %d: differing contains %d, n0 %d, n1 %d of %d" % (
            res, sort_points, *[(g != w).sum() for g, w in zip(got, want)], len(points)))
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    return want


@pytest.mark.parametrize("name", cases.MESHES)
def test_containment_equals_the_reference(hip, golden, name):
    """1: all three meshes at all three hash resolutions; the crossing counts equal the restatement's"""
    v, f = golden[name + "_v"], golden[name + "_f"]
    points = cases.query_points(v, f, golden["jitter"], golden["uniform"])
    assert len(points) <= 11000 and len(f) <= 1052
    for res in cases.HASH_RESOLUTIONS:
        want = check_contains(v, f, points, res)
        fixture = unpack(golden["%s_contains_%d" % (name, res)], (len(points),))
        assert int((want[0] != fixture).sum()) == 0
    from rfdnet_amd.mesh_sample import check_mesh_contains
    got = check_mesh_contains(dev(v, torch.float32), dev(f), dev(points))      # f32 vertices are the same numbers as f64
    v32 = v.astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(got.cpu().numpy(), ref.contains(v32, f, points)[0])


def test_point_order_and_batch_independence(hip, golden):
    """2: permuted points, two halves, f32 points against the same values as f64"""
    from rfdnet_amd.mesh_sample import MeshIntersector
    v, f = golden["sphere_v"], golden["sphere_f"]
    points = cases.query_points(v, f, golden["jitter"], golden["uniform"])
    mi = MeshIntersector(dev(v), dev(f), 16)
    whole = [t.cpu().numpy() for t in mi.query(dev(points), return_counts=True)]
    perm = np.random.default_rng(5).permutation(len(points))
    half = len(points) // 2 + 1
    for sort_points in (False, True):
        shuffled = [t.cpu().numpy() for t in mi.query(dev(points[perm]), return_counts=True, sort_points=sort_points)]
        parts = [mi.query(dev(p), return_counts=True, sort_points=sort_points) for p in (points[:half], points[half:])]
        for k in range(3):
            np.testing.assert_array_equal(shuffled[k], whole[k][perm])
            np.testing.assert_array_equal(np.concatenate([part[k].cpu().numpy() for part in parts]), whole[k])
    p32 = points.astype(np.float32)
    got32 = [t.cpu().numpy() for t in mi.query(dev(p32), return_counts=True)]
    got64 = [t.cpu().numpy() for t in mi.query(dev(p32.astype(np.float64)), return_counts=True)]
    for a, b in zip(got32, got64):
        np.testing.assert_array_equal(a, b)


def test_degenerate_content(hip, golden):
    """3: zero-area and vertical faces, an open mesh, the cube's four all-covering triangles at 512, nothing to ask,
    nothing to ask about"""
    from rfdnet_amd.mesh_sample import MeshIntersector
    v, f = cases.cube()
    points = np.concatenate([cases.grid_centres(cases.GRID), cases.jittered_centres(cases.GRID, golden["jitter"]),
                             golden["uniform"] * 0.6 + 0.5, v, np.full((1, 3), np.nan)])
    # two zero-area faces (two corners equal) and a vertical face on top of the cube (n2 == 0; its projection is a
    # segment, so rule C4's det == 0 skips it before rule C5 could)
    v2 = np.concatenate([v, [[0.3, 0.3, 0.1], [0.3, 0.3, 0.9], [0.6, 0.5, 0.5]]])
    f2 = np.concatenate([f, [[8, 8, 10], [8, 9, 10], [0, 7, 7]]])
    check_contains(v2, f2, points, 16)
    # the cube minus one face: the two parities disagree for the points under the hole
    want = check_contains(v, f[2:], points, 16)
    assert ((want[1] % 2) != (want[2] % 2)).any()
    # hash_resolution 512: the four horizontal triangles cover all 262 144 cells each
    mi = MeshIntersector(dev(v), dev(f), 512)
    assert mi.n_pairs >= 4 * 512 * 512 // 2 and int(mi.offsets[-1]) == mi.n_pairs
    cells = mi.cells.cpu().numpy()
    assert cells.min() >= 0 and cells.max() < len(f)
    counts = np.bincount(cells, minlength=len(f))
    box = lambda t: np.clip(np.trunc(t).astype(int), 0, 511)
    scale, translate = ref.rescale_constants(v, f, 512)
    tri = (scale * v[f] + translate)[:, :, :2]
    want_counts = np.prod(box(tri.max(1)) - box(tri.min(1)) + 1, axis=1)
    np.testing.assert_array_equal(counts, want_counts)
    want = check_contains(v, f, points, 512)
    assert want[0].any() and want[1].max() >= 1
    # empty point list, empty mesh
    got = mi.query(dev(points[:0]), return_counts=True)
    assert [tuple(t.shape) for t in got] == [(0,)] * 3 and got[0].dtype == torch.bool
    empty = MeshIntersector(dev(v), dev(f[:0]), 512)
    got = empty.query(dev(points), return_counts=True)
    assert not got[0].any() and not got[1].any() and not got[2].any() and got[0].shape == (len(points),)


def test_surface_interior_and_ray_voxels(hip, golden):
    """4: the fixture at 7, 16 and 33; one triangle larger than the grid; a mesh partly outside the cube"""
    from rfdnet_amd import mesh_sample as ms
    R = cases.GRID
    jitter = dev(golden["jitter"])
    for name in cases.MESHES:
        v, f = dev(golden[name + "_v"]), dev(golden[name + "_f"])
        for S in cases.SURFACE_RESOLUTIONS:
            got = ms.voxelize_surface(v, f, S)
            assert got.dtype == torch.bool and tuple(got.shape) == (S, S, S)
            diff = int((got.cpu().numpy() != unpack(golden["%s_surface_%d" % (name, S)], (S, S, S))).sum())
            print(name, S, "differing voxels:", diff)
            assert diff == 0
        interior = ms.voxelize_interior(v, f, R, jitter=jitter).cpu().numpy()
        assert int((interior != unpack(golden[name + "_interior"], (R, R, R))).sum()) == 0
        ray = ms.voxelize_ray(v, f, R, jitter=jitter).cpu().numpy()
        assert int((ray != unpack(golden[name + "_ray"], (R, R, R))).sum()) == 0
    big_v = np.array([[-3., -2.5, -0.31], [4., -1.5, 0.2], [-0.5, 5., 0.4]])
    big_f = np.array([[0, 1, 2]])
    for S in (7, 33):
        want = ref.voxelize_surface(big_v, big_f, S)
        assert want.sum() > S * S // 2
        np.testing.assert_array_equal(ms.voxelize_surface(dev(big_v), dev(big_f), S).cpu().numpy(), want)
    v, f = golden["ellipsoid_v"] * 1.3 + [0.2, -0.15, 0.1], golden["ellipsoid_f"]
    assert v.max() > 0.5 and v.min() < -0.5
    for S in (16, 33):
        np.testing.assert_array_equal(ms.voxelize_surface(dev(v), dev(f), S).cpu().numpy(), ref.voxelize_surface(v, f, S))
    assert not ms.voxelize_surface(dev(v), dev(f[:0]), 5).any()
    assert tuple(ms.voxelize_ray(dev(v), dev(f[:0]), 5).shape) == (5, 5, 5)
    # the module's own jitter is 0.1 (rand - 0.5) from the generator
    v, f = dev(golden["sphere_v"]), dev(golden["sphere_f"])
    own = ms.voxelize_interior(v, f, R, generator=torch.Generator(device="cuda").manual_seed(3))
    drawn = 0.1 * (torch.rand(R ** 3, 3, dtype=torch.float64, device="cuda",
                              generator=torch.Generator(device="cuda").manual_seed(3)) - 0.5)
    assert torch.equal(own, ms.voxelize_interior(v, f, R, jitter=drawn))
    np.testing.assert_array_equal(own.cpu().numpy(), ref.voxelize_interior(golden["sphere_v"], golden["sphere_f"], R,
                                                                           drawn.cpu().numpy()))


@pytest.mark.parametrize("name", ["sphere", "unit_cube"])
def test_sample_surface(hip, golden, name):
    """5: the face within the summation bound of the sequential prefix, no case excluded; the point and the normal equal
    the restatement at that face bit for bit"""
    from rfdnet_amd.mesh_sample import sample_surface
    v, f = (golden[name + "_v"], golden[name + "_f"]) if name == "sphere" else cases.cube()
    F = len(f)
    u = np.random.default_rng(9).random((3000, 3))
    u[:4, 0] = [0., np.nextafter(1., 0.), 0.5, 0.25]
    u[4:8, 1:] = [[0., 0.], [0.999, 0.999], [0.5, 0.5], [1. / 3, 2. / 3]]
    for dtype in (torch.float64, torch.float32):
        p, face, normals = sample_surface(dev(v), dev(f), len(u), u=dev(u), return_normals=True, dtype=dtype)
        assert p.dtype == dtype and normals.dtype == dtype and face.dtype == torch.int32
        face = face.cpu().numpy().astype(np.int64)
        c = ref.sequential_prefix(ref.face_areas(v, f))
        delta = 3 * F * 2. ** -52 * c[-1]
        target = u[:, 0] * c[-1]
        below = np.where(face > 0, c[np.maximum(face - 1, 0)], -np.inf)
        assert face.min() >= 0 and face.max() < F
        assert (below - delta < target).all() and (target <= c[face] + delta).all()
        assert face[0] == 0                                   # u0 = 0: cum[0] >= 0 is the first that reaches the target
        want_p, want_n = ref.sample_at(v, f, face, u)
        npd = np.float64 if dtype == torch.float64 else np.float32
        np.testing.assert_array_equal(p.cpu().numpy().view(np.uint8), want_p.astype(npd).view(np.uint8))
        np.testing.assert_array_equal(normals.cpu().numpy().view(np.uint8), want_n.astype(npd).view(np.uint8))
    if name == "unit_cube":
        p = p.double().cpu().numpy()
        on_plane = np.minimum(np.abs(p - 0.2), np.abs(p - 0.8)).min(1)
        assert on_plane.max() < 1e-6 and p.min() > 0.2 - 1e-6 and p.max() < 0.8 + 1e-6
        assert len(np.unique(face)) == 12
    # a zero-area face gets the zero normal and no share of the samples; its own randomness comes from the generator
    v2, f2 = np.concatenate([v, v[:1]]), np.concatenate([[[0, len(v), 0]], f])
    p, face = sample_surface(dev(v2), dev(f2), 500, generator=torch.Generator(device="cuda").manual_seed(2))
    assert p.dtype == torch.float32 and int(face.min()) >= 1
    again = sample_surface(dev(v2), dev(f2), 500, generator=torch.Generator(device="cuda").manual_seed(2))
    assert torch.equal(p, again[0]) and torch.equal(face, again[1])
    assert tuple(sample_surface(dev(v), dev(f), 0)[0].shape) == (0, 3)
    with pytest.raises(ValueError, match="total area"):
        sample_surface(dev(v2), dev(f2[:1]), 3)
    with pytest.raises(ValueError, match="total area"):
        sample_surface(dev(v2), dev(f2[:0]), 3)


def test_is_watertight(hip, golden):
    """6"""
    from rfdnet_amd.mesh_sample import is_watertight
    for name in cases.MESHES:
        assert is_watertight(dev(golden[name + "_f"])) is True
    f = cases.cube()[1]
    assert is_watertight(dev(f[1:])) is False
    assert is_watertight(dev(np.concatenate([f, f[3:4]]))) is False


def test_sample_mesh_tool(hip, tmp_path):
    """7: the command line on the cube: the reference's keys, dtypes and shapes; the inside share of the uniform points;
    the voxels"""
    from rfdnet_amd import io, mesh_sample as ms
    v, f = cases.cube()
    src, out = str(tmp_path / "cube.off"), str(tmp_path / "out")
    io.write_off(src, v, f)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sample_mesh.py"), src, "--out", out, "--resize",
                          "--points_size", "4000", "--pointcloud_size", "1000", "--packbits", "--seed", "1"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    report = json.loads(run.stdout.strip().splitlines()[-1])
    assert report["watertight"] is True and sorted(report["written"]) == ["cube.off", "pointcloud.npz", "points.npz",
                                                                         "voxels_16.binvox"]
    np.testing.assert_allclose(report["loc"], [0.5] * 3, atol=1e-15)
    assert abs(report["scale"] - 0.6) < 1e-15
    pc = np.load(os.path.join(out, "pointcloud.npz"))
    assert sorted(pc.files) == ["loc", "normals", "points", "scale"]
    assert pc["points"].shape == (1000, 3) and pc["points"].dtype == np.float32
    assert pc["normals"].shape == (1000, 3) and pc["normals"].dtype == np.float32
    assert np.abs(np.abs(pc["points"]).max(1) - 0.5).max() < 1e-6 and np.abs(np.abs(pc["normals"]).sum(1) - 1).max() == 0
    pts = np.load(os.path.join(out, "points.npz"))
    assert sorted(pts.files) == ["loc", "occupancies", "points", "scale"]
    assert pts["points"].shape == (4000, 3) and pts["points"].dtype == np.float32
    assert pts["occupancies"].dtype == np.uint8 and pts["occupancies"].shape == (500,)
    occ = np.unpackbits(pts["occupancies"])[:4000].astype(bool)
    share = occ[:2000].mean()
    print("inside share of the uniform points: %.4f" % share)
    assert abs(share - 1 / 1.1 ** 3) < 5 * 0.0097
    inside = (np.abs(pts["points"][:2000].astype(np.float64)) < 0.5 - 1e-6).all(1)
    outside = (np.abs(pts["points"][:2000].astype(np.float64)) > 0.5 + 1e-6).any(1)
    assert occ[:2000][inside].all() and not occ[:2000][outside].any()
    assert np.abs(pts["points"][:2000]).max() <= 0.55 and np.abs(pts["points"][2000:]).max() < 0.6
    grid, translate, scale = io.read_binvox(os.path.join(out, "voxels_16.binvox"))
    w, _ = io.read_off(os.path.join(out, "cube.off"))
    want = ms.voxelize_ray(dev(w), dev(f), 16, generator=torch.Generator(device="cuda").manual_seed(1))
    np.testing.assert_array_equal(grid, want.cpu().numpy())
    assert grid.shape == (16, 16, 16) and grid.all() and scale == report["scale"]
    # an open mesh: a warning, the point cloud and the mesh, nothing else
    io.write_off(src, v, f[1:])
    out2 = str(tmp_path / "open")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sample_mesh.py"), src, "--out", out2,
                          "--pointcloud_size", "100"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "not watertight" in run.stderr
    assert sorted(os.listdir(out2)) == ["cube.off", "pointcloud.npz"]


def test_refusals_before_any_launch(hip):
    """8: a bad index, a flat mesh, a NaN vertex: each is a ValueError of the host-side check; no gather and no kernel
    ever sees the bad index"""
    from rfdnet_amd import mesh_sample as ms
    v, f = cases.cube()
    p = dev(np.zeros((4, 3)))
    calls = (lambda a, b: ms.MeshIntersector(a, b), lambda a, b: ms.check_mesh_contains(a, b, p),
             lambda a, b: ms.voxelize_surface(a, b, 8), lambda a, b: ms.voxelize_interior(a, b, 8),
             lambda a, b: ms.voxelize_ray(a, b, 8), lambda a, b: ms.sample_surface(a, b, 5),
             lambda a, b: ms.sample_points(a, b, 10))
    for bad in (8, -1, 1 << 33):
        g = f.copy()
        g[4, 2] = bad
        for call in calls:
            with pytest.raises(ValueError, match="face indices"):
                call(dev(v), dev(g))
    w = v.copy()
    w[5, 1] = np.nan
    for call in calls:
        with pytest.raises(ValueError, match="not finite"):
            call(dev(w), dev(f))
    flat = v.copy()
    flat[:, 2] = 0.5
    for call in (calls[0], calls[1], calls[3], calls[4], calls[6]):
        with pytest.raises(ValueError, match="no extent"):
            call(dev(flat), dev(f))
    assert ms.voxelize_surface(dev(flat), dev(f), 8).any()               # a flat mesh has a surface
    with pytest.raises(ValueError, match="hash_resolution"):
        ms.MeshIntersector(dev(v), dev(f), 1)
    with pytest.raises(ValueError, match="resolution"):
        ms.voxelize_surface(dev(v), dev(f), 0)
    with pytest.raises(ValueError, match="points are"):
        ms.MeshIntersector(dev(v), dev(f), 4).query(dev(np.zeros((4, 3), np.int64)))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ms.MeshIntersector(dev(v), dev(f), 4).query(torch.zeros(4, 3))
    torch.cuda.synchronize()
