"""Watertight meshes on the device: the stage of the reference that makes the CAD shapes everything else consumes
(utils/shapenet/1_fuse_shapenetv2.py).  A triangle soup is rendered to depth maps from views on a sphere, the depth maps
are fused into a truncated signed distance field, and marching cubes on the field gives a closed surface.

The depth maps come from this project's own rasteriser (csrc/raster.hip, the rules of include/rfd_render.h; its host
driver and the camera's 16 doubles are render.rasterise and render.camera_params), which is not
the reference's OpenGL renderer: they are NOT the reference's depth maps pixel for pixel, and neither is the mesh its
mesh vertex for vertex.  The fusion (csrc/tsdf_fusion.hip, the rules of include/rfd_fuse.h) is the reference's: given the
same depth maps it returns the reference's field bit for bit (tests/golden/F_FUSE.npz), and marching cubes is PyMCubes'
face for face.  Everything is queued on the current stream; the one host synchronisation is marching cubes' own.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from .iscnet.mcubes import marching_cubes_batch
from .render import camera_params, rasterise

WatertightResult = collections.namedtuple("WatertightResult", "vertices faces tsdf depth")


def views_on_sphere(n):
    """-> (n,3,3) float64: the rotations of the reference's get_views(n).  The view points are the golden-angle spiral of
    get_points (with its rnd = 1): y_i = (2 i + 1) / n - 1, phi_i = ((i + 1) mod n) pi (3 - sqrt 5); the rotation of a
    view is R_y(longitude) R_x(latitude) with longitude = -atan2(x, y) and latitude = atan2(z, sqrt(x^2 + y^2))."""
    n = int(n)
    if n < 1:
        return np.zeros((0, 3, 3))
    i = np.arange(n, dtype=np.float64)
    step = 2. / n
    y = (i * step - 1) + step / 2
    r = np.sqrt(1 - y ** 2)
    phi = ((i + 1.) % n) * (math.pi * (3. - math.sqrt(5.)))
    x, z = np.cos(phi) * r, np.sin(phi) * r
    lon, lat = -np.arctan2(x, y), np.arctan2(z, np.sqrt(x ** 2 + y ** 2))
    one, zero = np.ones(n), np.zeros(n)
    r_x = np.stack([one, zero, zero, zero, np.cos(lat), -np.sin(lat), zero, np.sin(lat), np.cos(lat)], 1).reshape(n, 3, 3)
    r_y = np.stack([np.cos(lon), zero, np.sin(lon), zero, one, zero, -np.sin(lon), zero, np.cos(lon)], 1).reshape(n, 3, 3)
    return r_y @ r_x


def _rows(a, dev, width):
    """(n,width) f32 on `dev` out of anything with n * width numbers"""
    a = _lib.as_tensor(a, dev, torch.float32)
    return a.reshape(a.numel() // width, width).contiguous()


@torch.no_grad()
def fuse_depthmaps(depth, K, R, T, resolution, truncation, voxel_size=None, unknown_is_free=False,
                   unobserved='-truncation', return_count=False, view_chunk=0):
    """depth (V,rows,cols) f32 on the GPU, K (V,3,3) or (3,3), R (V,3,3), T (V,3) (tensors or numpy), resolution: n or
    (D,H,W), voxel_size: default 1 / the largest of D, H, W (the volume is the reference's cube [-0.5, 0.5) along that axis)
    -> tsdf (D,H,W) f32 [, count (D,H,W) i32]: the reference's pyfusion.tsdf_gpu.  unobserved: the value of a voxel that no
    view gave a valid sample: '-truncation' (tsdf_gpu's), '+truncation' (the field after the reference's tsdfmask_gpu
    pass: `tsdf[mask == 0] = truncation`) or a number.  view_chunk: include/rfd_fuse.h (0: the library's choice)."""
    _lib.need_gpu(depth)
    dev = depth.device
    D, H, W = (int(resolution),) * 3 if np.ndim(resolution) == 0 else (int(s) for s in resolution)
    if depth.dim() != 3:
        raise ValueError("fuse_depthmaps: depth is (V,rows,cols), got %s" % (tuple(depth.shape),))
    V, rows, cols = (int(s) for s in depth.shape)
    depth = depth.float().contiguous()
    K, R, T = _rows(K, dev, 9), _rows(R, dev, 9), _rows(T, dev, 3)
    K = K.expand(V, 9).contiguous() if K.shape[0] == 1 else K
    if K.shape[0] != V or R.shape[0] != V or T.shape[0] != V:
        raise ValueError("fuse_depthmaps: %d depth maps, but %d K, %d R, %d T" % (V, K.shape[0], R.shape[0], T.shape[0]))
    truncation = float(truncation)
    value = {'-truncation': -truncation, '+truncation': truncation}.get(unobserved, unobserved)
    if voxel_size is None:
        voxel_size = 1. / max(D, H, W, 1)
    tsdf = torch.empty(max(D, 0), max(H, 0), max(W, 0), dtype=torch.float32, device=dev)   # the library refuses sizes < 0
    count = torch.empty_like(tsdf, dtype=torch.int32) if return_count or view_chunk else None
    _lib.call("rfd_tsdf_fuse", dev, V, rows, cols, depth.data_ptr(), K.data_ptr(), R.data_ptr(), T.data_ptr(), D, H, W,
              float(voxel_size), truncation, int(bool(unknown_is_free)), float(value), int(view_chunk), tsdf.data_ptr(),
              _lib.ptr(count))
    return (tsdf, count) if return_count else tsdf


@torch.no_grad()
def render_depthmaps(vertices, faces, rotations, image_size, focal, znf, offset):
    """vertices (V,3) f32 and faces (F,3) i32 on the GPU, in the frame the views look at (the reference's normalised cube),
    rotations (n,3,3) float64 on the host -> (n,image_size,image_size) f32: per view render.rasterise (projection and
    depth-tested triangles, no scan points) on the first view's scratch, then rfd_depth_from_keys into the view's slot
    of the stack.

    The camera's world-to-view is [R | (0,0,1)] and its principal point (c + 0.5, c + 0.5) with c = image_size / 2: the
    rasteriser's pixel (i, j) has its centre at (i + 0.5, j + 0.5), the fusion looks a projected voxel up at the pixel whose
    INTEGER coordinates are nearest to (u, v) under a principal point of (c, c); the half pixel makes the two agree."""
    dev, S, n = vertices.device, int(image_size), len(rotations)
    stack = torch.empty(n, max(S, 0), max(S, 0), dtype=torch.float32, device=dev)
    scratch = None
    for v in range(n):
        cam = camera_params(np.concatenate([np.asarray(rotations[v], np.float64), [[0.], [0.], [1.]]], 1),
                            focal, focal, S / 2. + 0.5, S / 2. + 0.5)
        scratch = rasterise(vertices, faces, cam, float(znf[0]), S, S, scratch=scratch)
        _lib.call("rfd_depth_from_keys", dev, S, S, scratch.keys.data_ptr(), float(znf[1]), float(offset),
                  stack[v].data_ptr())
    return stack


def normalisation(vertices, padding):
    """-> centre (3,), scale (): the reference's: the centre of the bounding box, the largest extent / (1 - padding)"""
    lo, hi = vertices.amin(0), vertices.amax(0)
    return (hi + lo) / 2., (hi - lo).max() / (1. - padding)


@torch.no_grad()
def watertight(vertices, faces, resolution=256, n_views=200, image_size=640, focal=640., padding=0.1,
               truncation_factor=10, depth_offset_voxels=1.5, znf=(0.25, 1.75), return_tsdf=False):
    """vertices (V,3) float and faces (F,3) integer tensors on the GPU: any triangle soup -> (vertices (V',3) f64,
    faces (F',3) i32) on the same device: a closed surface around it, in the input's frame.  The defaults are the reference's.

      1 the soup is moved into the cube [-0.5, 0.5]^3: centred on its bounding box, divided by largest extent / (1 - padding);
      2 per view of views_on_sphere(n_views), from the distance 1: a depth map of image_size^2 (render_depthmaps), cut at
        znf[1], pulled depth_offset_voxels voxels towards the camera and eroded by 3x3 (thin parts survive the fusion);
      3 one fusion into resolution^3 with truncation = truncation_factor voxels; unobserved voxels count as outside;
      4 marching cubes at 0 on the negated field, padded so that the surface closes at the volume's border;
      5 the vertices go back to the input's frame (with the reference's half-voxel shift, which is part of its output).

    return_tsdf: -> WatertightResult(vertices, faces, tsdf (D,H,W) f32, depth (n_views,image_size,image_size) f32).
    The depth maps are this rasteriser's, not OpenGL's: the result is not the reference's mesh vertex for vertex (module
    docstring).  The truncated field has a second zero crossing one truncation behind every surface that is seen from one
    side only, so a closed thick shape gets an inner shell, as it does in the reference."""
    _lib.need_gpu(vertices, faces)
    resolution = int(resolution)
    voxel = 1. / resolution
    v64 = vertices.double().reshape(-1, 3)
    centre, scale = normalisation(v64, padding)
    unit = ((v64 - centre) / scale).float().contiguous()
    depth = render_depthmaps(unit, faces.reshape(-1, 3).to(torch.int32).contiguous(), views_on_sphere(n_views),
                             image_size, focal, znf, np.float32(depth_offset_voxels * voxel))
    c = int(image_size) / 2.
    tsdf = fuse_depthmaps(depth, np.array([focal, 0., c, 0., focal, c, 0., 0., 1.]), views_on_sphere(n_views),
                          np.tile([0., 0., 1.], (int(n_views), 1)), resolution, truncation_factor * voxel,
                          voxel_size=voxel, unobserved='+truncation')
    # the reference: np.pad(tsdf transposed to (W,H,D), 1, constant_values=1e6), then marching_cubes(-tsdf, 0)
    v, f = marching_cubes_batch((-tsdf.permute(2, 1, 0))[None], 0., pad_value=-1e6)[0]
    v = ((v - 1.) / resolution - 0.5) * scale + centre
    return WatertightResult(v, f, tsdf, depth) if return_tsdf else (v, f)
