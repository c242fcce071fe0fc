"""GPU: the watertight path (rfdnet_amd/watertight.py, csrc/tsdf_fusion.hip, the rules of include/rfd_fuse.h).  The fusion
is compared by EQUALITY: with the reference's own output (tests/golden/F_FUSE.npz) and with the numpy restatement
tests/fuse_ref.py, which tests/test_fuse_cpu.py holds to that fixture."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases  # noqa: E402
import fuse_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (0, 8)                    # the library's choice, and one launch per 8 views


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_fuse(depth, K, R, T, shape, vx_size, truncation, unknown_is_free, unobserved, view_chunk=0):
    from rfdnet_amd.watertight import fuse_depthmaps
    tsdf, count = fuse_depthmaps(torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda(), K, R, T, shape,
                                 truncation, voxel_size=vx_size, unknown_is_free=unknown_is_free, unobserved=unobserved,
                                 return_count=True, view_chunk=view_chunk)
    assert tsdf.dtype == torch.float32 and count.dtype == torch.int32 and tuple(tsdf.shape) == tuple(shape)
    return tsdf.cpu().numpy(), count.cpu().numpy()


def check(depth, K, R, T, shape, vx_size, truncation, unknown_is_free, unobserved, chunks=CHUNKS):
    """the device against the restatement, exactly, tsdf and count; -> the restatement's pair"""
    want, n = fuse_ref.fuse(depth, K, R, T, shape, vx_size, truncation, unknown_is_free, unobserved)
    for chunk in chunks:
        got, m = device_fuse(depth, K, R, T, shape, vx_size, truncation, unknown_is_free, unobserved, chunk)
        print("view_chunk %d: tsdf differing %d of %d, count differing %d"
              % (chunk, (bits(got) != bits(want)).sum(), want.size, (m != n).sum()))
        np.testing.assert_array_equal(m, n)
        np.testing.assert_array_equal(bits(got), bits(want))
    return want, n


@pytest.mark.parametrize("unknown_is_free", [0, 1])
def test_fixture(hip, golden_dir, unknown_is_free):
    """1: the reference's fusion_tsdf_cpu bit for bit, and its fusion_tsdfmask_cpu as count > 0"""
    z = np.load(os.path.join(golden_dir, "F_FUSE.npz"))
    t = float(z['truncation'])
    for chunk in (0, 2):
        got, count = device_fuse(z['depth'], z['K'], z['R'], z['T'], z['shape'], float(z['vx_size']), t, unknown_is_free,
                                 '-truncation', chunk)
        np.testing.assert_array_equal(bits(got), bits(z['tsdf_free%d' % unknown_is_free]))
        np.testing.assert_array_equal(count > 0, z['mask_free%d' % unknown_is_free] > 0)


def views(n, rows, cols, focal, seed, cx=None, cy=None):
    """n views on the sphere at distance 1 and depth maps around 1: noise wide enough for every branch of rule 4"""
    from rfdnet_amd.watertight import views_on_sphere
    rng = np.random.default_rng(seed)
    depth = (1. + 0.35 * rng.normal(0, 1, (n, rows, cols))).astype(np.float32)
    draw = rng.uniform(0, 1, depth.shape)
    depth[draw < 0.03], depth[draw > 0.97] = -1., 0.
    K = np.tile(np.array([focal, 0, cols / 2. if cx is None else cx, 0, focal, rows / 2. if cy is None else cy, 0, 0, 1],
                         np.float32), (n, 1))
    return depth, K, views_on_sphere(n).astype(np.float32).reshape(n, 9), np.tile(np.float32([0, 0, 1]), (n, 1))


def test_37_views_against_the_restatement(hip):
    """2: a prime number of views, more than a chunk and no multiple of the views in flight; a volume that is no multiple
    of the brick in any direction and reaches beyond what the views see"""
    depth, K, R, T = views(37, 33, 47, 30., 1)
    shape, vx, t = (9, 13, 22), 1. / 14, 0.12
    _, n = check(depth, K, R, T, shape, vx, t, 0, -t)
    assert n.min() == 0 and n.max() > 20
    check(depth, K, R, T, shape, vx, t, 1, t, chunks=(0, 8, 5, 36, 37, 100))


def test_edges(hip):
    """3"""
    depth, K, R, T = views(6, 12, 10, 9., 2)
    shape, vx, t = (6, 5, 7), 1. / 7, 0.2
    # no view at all
    want, n = check(depth[:0], K[:0], R[:0], T[:0], shape, vx, t, 0, 0.625)
    assert (want == 0.625).all() and (n == 0).all()
    # a view that no voxel sees: its principal point is far outside
    off = K.copy()
    off[2, 2] = 1e4
    want, n = check(depth[2:3], off[2:3], R[2:3], T[2:3], shape, vx, t, 0, -t)
    assert (n == 0).all()
    check(depth, off, R, T, shape, vx, t, 1, -t)
    # NaN and +inf in the depth maps: a NaN is never valid, +inf is (free space: the sample is +truncation)
    bad = depth.copy()
    draw = np.random.default_rng(3).uniform(0, 1, bad.shape)
    bad[draw < 0.2], bad[draw > 0.8] = np.nan, np.inf
    want, n = check(bad, K, R, T, shape, vx, t, 0, -t)
    assert np.isfinite(want).all() and 0 < (n > 0).sum()
    check(np.full_like(depth, np.nan), K, R, T, shape, vx, t, 1, t)
    # voxel centres on integers (vx_size = 1), R = 1, T = (0,0,-1): dd = z - 1 is -1, 0, 1, 2 by slice; where dd = 0,
    # u is +-inf, or NaN in the column x = 0.  None of them may be looked up.
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (2, 1))
    k2 = np.tile(np.float32([2, 0, 3, 0, 2, 3, 0, 0, 1]), (2, 1))
    d2 = np.random.default_rng(4).uniform(0.5, 3., (2, 12, 10)).astype(np.float32)
    want, n = check(d2, k2, eye, np.float32([[0, 0, -1], [0, 0, -1]]), (4, 3, 4), 1., 0.75, 0, -0.75)
    assert (n[1] == 0).all() and (n[2:] > 0).any()
    # pixels at the image's rim: dd = 1, u = 6 x + cx with x = 0, 1: tu = -0.25 (pixel 0) and 5.75 (pixel 5 of 6);
    # tu = -1 (off) and 5; tu = 0 and 6 = cols (off); the same along v through the rows
    k3 = np.stack([np.float32([6, 0, c, 0, 5, c, 0, 0, 1]) for c in (-0.75, -1.5, -0.5)])
    d3 = np.random.default_rng(5).uniform(0.5, 1.5, (3, 5, 6)).astype(np.float32)
    want, n = check(d3, k3, np.tile(eye[:1], (3, 1)), np.tile(np.float32([0, 0, 1]), (3, 1)), (1, 2, 2), 1., 1., 0, -1.)
    np.testing.assert_array_equal(n[0], [[2, 1], [1, 2]])
    # the smallest volume, and a line of 65 voxels: one more than a wave
    for small in ((1, 1, 1), (1, 1, 65), (65, 1, 1)):
        check(depth, K, R, T, small, 1. / 65, t, 0, -t)


def rasterised_keys(vertices, faces, W, H, focal):
    """the key buffer the rasteriser leaves for a camera at the origin that looks along +z"""
    from rfdnet_amd import _lib
    dev = torch.device("cuda")
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev)
    nv, nf = v.shape[0], f.shape[0]
    q, sxy = torch.empty(nv, dtype=torch.float64, device=dev), torch.empty(nv, 2, dtype=torch.int32, device=dev)
    valid, keys = torch.empty(nv, dtype=torch.uint8, device=dev), torch.empty(H, W, dtype=torch.int64, device=dev)
    cam = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, focal, focal, W / 2., H / 2.], np.float64)
    cam_p = cam.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    _lib.call("rfd_raster_project", dev, nv, 0, 3, v.data_ptr(), v.data_ptr(), cam_p, 0.25, q.data_ptr(), sxy.data_ptr(),
              valid.data_ptr())
    _lib.call("rfd_raster_triangles", dev, nv, nf, 0, W, H, 1, f.data_ptr(), q.data_ptr(), sxy.data_ptr(),
              valid.data_ptr(), keys.data_ptr())
    return keys


def test_depth_from_keys(hip):
    """4: a tilted cube that reaches over the upper and the left border of a 33 x 47 image, cut at far = 1"""
    from rfdnet_amd import _lib
    v, f = decimate_cases.unit_cube()
    a, b = 0.6, 0.4
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    v = (np.asarray(v, np.float64) - 0.5) @ rot.T + [-0.25, -0.2, 1.]
    H, W, far, offset = 33, 47, 1., np.float32(1.5 / 32)
    keys = rasterised_keys(v, f, W, H, 40.)
    host = keys.cpu().numpy().view(np.uint64)
    z = fuse_ref.key_depth(host, 10.)
    covered = host != 0
    assert covered.any() and not covered.all() and (z[covered] > far).any() and (z[covered] < far).any()
    assert covered[0].any() and covered[:, 0].any() and not covered[-1].any() and not covered[:, -1].any()
    depth = torch.full((H, W), -7., dtype=torch.float32, device="cuda")
    _lib.call("rfd_depth_from_keys", keys.device, W, H, keys.data_ptr(), far, float(offset), depth.data_ptr())
    np.testing.assert_array_equal(bits(depth.cpu().numpy()), bits(fuse_ref.depth_from_keys(host, far, offset)))
    one = torch.empty(1, 1, dtype=torch.float32, device="cuda")                     # a 1 x 1 image: no neighbour at all
    _lib.call("rfd_depth_from_keys", keys.device, 1, 1, keys[:1, :1].contiguous().data_ptr(), far, 0.25, one.data_ptr())
    assert one.item() == fuse_ref.depth_from_keys(host[:1, :1], far, 0.25)[0, 0]


def test_refusals(hip):
    """5: what the entries cannot index is refused before anything is launched (the buffers here are far too small
    for any of these sizes)"""
    from rfdnet_amd import _lib
    dev = torch.device("cuda")
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    p = buf.data_ptr()

    def fuse(V=1, rows=2, cols=2, D=2, H=2, W=2, chunk=0, tsdf=p):
        _lib.call("rfd_tsdf_fuse", dev, V, rows, cols, p, p, p, p, D, H, W, 0.5, 0.5, 0, -0.5, chunk, tsdf, cnt.data_ptr())
    for bad in (dict(V=-1), dict(D=-1), dict(H=-1), dict(W=-1), dict(chunk=-1), dict(rows=0), dict(cols=0),
                dict(rows=8193), dict(cols=8193), dict(D=2048, H=2048, W=2048), dict(D=65536, H=65536, W=1),
                dict(D=1, H=1, W=2 ** 31 - 1, tsdf=None), dict(V=33, rows=8192, cols=8192), dict(tsdf=None)):
        with pytest.raises(_lib.RfdHipError, match=r"rfd_tsdf_fuse failed \(hipError 1\)"):        # hipErrorInvalidValue
            fuse(**bad)
    for W, H in ((0, 4), (4, 0), (8193, 4), (4, 8193), (-1, -1)):
        with pytest.raises(_lib.RfdHipError, match=r"rfd_depth_from_keys failed \(hipError 1\)"):
            _lib.call("rfd_depth_from_keys", dev, W, H, p, 1., 0., p)
    torch.cuda.synchronize()
    assert (buf == 0).all() and (cnt == 0).all()                     # nothing ran
    fuse()                                                           # and the entry still works
    fuse(D=0)                                                        # an empty volume is valid: nothing to do
    torch.cuda.synchronize()


def uv_sphere(radius, centre, n_lat=12, n_lon=24):
    lat = np.pi * np.arange(1, n_lat) / n_lat
    lon = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)),
                     np.outer(np.cos(lat), np.ones(n_lon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.]], ring, [[0, 0, -1.]]]) * radius + np.asarray(centre)
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    south = 1 + (n_lat - 1) * n_lon
    f = [[0, idx(0, j), idx(0, j + 1)] for j in range(n_lon)]
    f += [[south, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)] for j in range(n_lon)]
    for i in range(n_lat - 2):
        for j in range(n_lon):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v, np.asarray(f, np.int32)


def test_watertight_end_to_end(hip):
    """6"""
    from rfdnet_amd.watertight import views_on_sphere, watertight
    centre = np.array([1., -2., 3.])
    v, f = uv_sphere(0.4, centre)
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    kw = dict(resolution=32, n_views=12, image_size=96, focal=96., truncation_factor=3)
    res = watertight(dv, df, return_tsdf=True, **kw)
    assert res.vertices.is_cuda and res.vertices.dtype == torch.float64 and res.faces.dtype == torch.int32
    depth = res.depth.cpu().numpy()
    assert depth.shape == (12, 96, 96) and depth.max() == np.float32(1.75) - np.float32(1.5 / 32) and depth.min() > 0.45
    K = np.tile(np.float32([96, 0, 48, 0, 96, 48, 0, 0, 1]), (12, 1))
    want, n = fuse_ref.fuse(depth, K, views_on_sphere(12).astype(np.float32), np.tile(np.float32([0, 0, 1]), (12, 1)),
                            (32, 32, 32), 1. / 32, 3. / 32, 0, 3. / 32)
    np.testing.assert_array_equal(bits(res.tsdf.cpu().numpy()), bits(want))
    assert (n > 0).mean() > 0.5 and (want < 0).any()
    verts, faces = res.vertices.cpu().numpy(), res.faces.cpu().numpy().astype(np.int64)
    assert faces.shape[0] > 500 and faces.min() == 0 and faces.max() == verts.shape[0] - 1
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    _, uses = np.unique(edges, axis=0, return_counts=True)
    assert (uses == 2).all()                                          # closed, and a manifold along every edge
    scale = 0.8 / 0.9                                                 # the largest extent / (1 - padding)
    # inside the normalisation cube.  Where the field is still negative in the volume's first layer (far corners take
    # the background at znf[1] for a surface) the pad closes it: that crossing lies a |value| / 1e6 <= truncation / 1e6
    # of a voxel outside the layer, 3e-9 of the cube's side here.
    unit = (verts - centre) / scale
    print("vertices %d, faces %d, unit range %.12f .. %.12f" % (verts.shape[0], faces.shape[0], unit.min(), unit.max()))
    assert unit.min() >= -0.5 - 3e-9 and unit.max() <= 0.5
    v2, f2 = watertight(dv, df, **kw)
    assert torch.equal(v2, res.vertices) and torch.equal(f2, res.faces)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        watertight(dv.cpu(), df, **kw)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        watertight(dv, df.cpu(), **kw)


def test_make_watertight_tool(hip, tmp_path):
    """7"""
    from rfdnet_amd import io
    v, f = uv_sphere(0.4, (0., 0., 0.), 6, 10)
    src, out = str(tmp_path / "in.off"), str(tmp_path / "out.off")
    io.write_off(src, v, f)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_watertight.py"), src, out, "--resolution", "16",
                           "--views", "6", "--image_size", "48", "--decimate_cells", "8"], cwd=ROOT, timeout=600,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode()[-2000:]
    said = json.loads(done.stdout.decode().strip().splitlines()[-1])
    got_v, got_f = io.read_off(out)
    assert said["input"] == {"vertices": len(v), "faces": len(f)}
    assert 0 < said["decimated"]["faces"] <= said["watertight"]["faces"]
    assert (got_v.shape[0], len(got_f)) == (said["decimated"]["vertices"], said["decimated"]["faces"])
    assert all(len(face) == 3 and 0 <= min(face) and max(face) < got_v.shape[0] for face in got_f)
