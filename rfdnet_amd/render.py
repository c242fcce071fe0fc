"""Headless render of the placed scene: the second half of the reference's `visualize` (demo.py:373-377 hands scan,
meshes and boxes to VTK and saves pred.png).  Here the picture is rasterised on the device the meshes live on
(csrc/raster.hip; the rules are in include/rfd_render.h and restated in tests/render_f64.py): one clear and three
launches per image, queued on the current stream, no host synchronisation.  Box wireframes, anti-aliasing and a
pixel-for-pixel match of VTK's picture are not attempted.

This module is the rasteriser's one host driver: camera_params() lays out the 16 doubles the library takes and
rasterise() owns the scratch buffers and the projection and triangle launches.  render_scene() shades its keys into a
picture; watertight.render_depthmaps() turns them into depth maps, one view after another on the same scratch.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

RenderResult = collections.namedtuple("RenderResult", "image depth ids")
RasterScratch = collections.namedtuple("RasterScratch", "q sxy valid keys")

# one colour per semantic class (the tab20 table's saturated half, then its light half); a class beyond it takes the last colour
DEFAULT_PALETTE = (
    (0.122, 0.467, 0.706), (1.000, 0.498, 0.055), (0.173, 0.627, 0.173), (0.839, 0.153, 0.157), (0.580, 0.404, 0.741),
    (0.549, 0.337, 0.294), (0.890, 0.467, 0.761), (0.498, 0.498, 0.498), (0.737, 0.741, 0.133), (0.090, 0.745, 0.812),
    (0.682, 0.780, 0.910), (1.000, 0.733, 0.471), (0.596, 0.875, 0.541), (1.000, 0.596, 0.588), (0.773, 0.690, 0.835),
    (0.769, 0.612, 0.580), (0.969, 0.714, 0.824), (0.780, 0.780, 0.780), (0.859, 0.859, 0.553), (0.620, 0.855, 0.898))
_palettes = {}


class Camera(object):
    """A pinhole camera, built in numpy float64.  View frame: x right, y down, z forward; pixel (i, j) has its centre at
    (i + 0.5, j + 0.5).  world_to_view (3,4), fx = fy from the vertical field of view, the principal point at the image
    centre; `params`: the 16 doubles the rasteriser takes (the matrix in row order, fx, fy, cx, cy)."""

    def __init__(self, eye, look_at, up=(0., 0., 1.), fov_y_deg=60., width=1024, height=768, near=0.05):
        eye, look_at, up = (np.asarray(a, np.float64).reshape(3) for a in (eye, look_at, up))
        fwd = look_at - eye
        fwd = fwd / np.linalg.norm(fwd)
        right = np.cross(fwd, up)
        right = right / np.linalg.norm(right)
        down = np.cross(fwd, right)
        rot = np.stack([right, down, fwd])
        self.eye, self.width, self.height, self.near = eye, int(width), int(height), float(near)
        self.fov_y_deg = float(fov_y_deg)
        self.world_to_view = np.concatenate([rot, -(rot @ eye)[:, None]], 1)
        self.fy = self.fx = 0.5 * self.height / np.tan(np.radians(self.fov_y_deg) / 2.)
        self.cx, self.cy = self.width / 2., self.height / 2.
        self.params = camera_params(self.world_to_view, self.fx, self.fy, self.cx, self.cy)

    @classmethod
    def fit(cls, points, width=1024, height=768, fov_y_deg=60.):
        """The default view of a scan (points (N,3+), numpy or a tensor): it looks at the centre of the scan's bounding
        box from the direction (0,-1,1)/sqrt(2), as the reference looks down on the scene from (0,-3,3), from the distance
        at which the box's bounding sphere fills the narrower field of view.  Every corner of the box is inside the image."""
        if torch.is_tensor(points):
            p = points.reshape(-1, points.shape[-1])[:, :3]
            lo, hi = p.amin(0).double().cpu().numpy(), p.amax(0).double().cpu().numpy()
        else:
            p = np.asarray(points, np.float64).reshape(-1, np.shape(points)[-1])[:, :3]
            lo, hi = p.min(0), p.max(0)
        centre, radius = (lo + hi) / 2., max(float(np.linalg.norm(hi - lo)) / 2., 1e-3)
        half_y = np.radians(fov_y_deg) / 2.
        half = min(half_y, np.arctan(np.tan(half_y) * width / height))
        distance = radius / np.sin(half)
        eye = centre + distance * np.array([0., -1., 1.]) / np.sqrt(2.)
        return cls(eye, centre, fov_y_deg=fov_y_deg, width=width, height=height, near=0.5 * (distance - radius))

    def project(self, points):
        """points (N,3) float64 -> screen (N,2) and z_view (N): the rasteriser's projection (for tests and callers)"""
        p = np.asarray(points, np.float64)
        v = p @ self.world_to_view[:, :3].T + self.world_to_view[:, 3]
        return np.stack([self.fx * v[:, 0] / v[:, 2] + self.cx, self.fy * v[:, 1] / v[:, 2] + self.cy], 1), v[:, 2]


def camera_params(world_to_view, fx, fy, cx, cy):
    """-> the contiguous (16,) float64 array the rasteriser takes: world_to_view (3,4) in row order, fx, fy, cx, cy"""
    return np.concatenate([np.asarray(world_to_view, np.float64).reshape(-1), [fx, fy, cx, cy]])


def _doubles(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def rasterise(verts, faces, params, near, W, H, points=None, point_px=1, scratch=None):
    """verts (V,3) f32 and faces (F,3) i32, contiguous on the GPU, params: camera_params(), points: None or (tensor, N,
    stride) -- N scan points of 3 f32, `stride` floats apart -- drawn as squares of point_px pixels, scratch: a
    RasterScratch of an earlier call with the same V + N, W and H, or None: allocated here
    -> RasterScratch(q f64 (V+N), sxy i32 (V+N,2), valid u8 (V+N), keys i64 (H,W)): the projection and the depth-tested
    triangles and points, two launches queued on the current stream.  keys holds the winner of every pixel."""
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    pc, N, stride = (verts, 0, 3) if points is None else points
    if scratch is None:
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
        scratch = RasterScratch(new(torch.float64, V + N), new(torch.int32, V + N, 2), new(torch.uint8, V + N),
                                new(torch.int64, max(H, 0), max(W, 0)))   # the library refuses sizes outside 1..8192
    q, sxy, valid, keys = (t.data_ptr() for t in scratch)
    cam, cam_p = _doubles(params)
    _lib.call("rfd_raster_project", dev, V, N, stride, verts.data_ptr(), pc.data_ptr(), cam_p, near, q, sxy, valid)
    _lib.call("rfd_raster_triangles", dev, V, F, N, W, H, int(point_px), faces.data_ptr(), q, sxy, valid, keys)
    return scratch


def render_scene(scene_mesh, point_cloud, camera, palette=None, point_px=3):
    """scene_mesh: iscnet.scene.SceneMesh (place_objects) on the GPU, point_cloud: (N,3+) or (1,N,3+) f32 on the same
    device, or None, camera: Camera, palette (C,3) f32 in 0..1 by semantic class (default DEFAULT_PALETTE), point_px: odd
    -> RenderResult(image (H,W,3) u8, depth (H,W) f32: z_view, +inf on the background, ids (H,W) i32: -1 background,
    [0, F) a face of scene_mesh, F + n scan point n).  Queued on the current stream; nothing is waited for."""
    verts, faces = scene_mesh.vertices, scene_mesh.faces
    _lib.need_gpu(verts, *(() if point_cloud is None else (point_cloud,)))
    dev = verts.device
    K, W, H = int(scene_mesh.obj_class.shape[0]), camera.width, camera.height
    points = None
    if point_cloud is not None:
        pc = point_cloud[0] if point_cloud.dim() == 3 else point_cloud
        if pc.dtype != torch.float32 or (pc.shape[0] and pc.stride(1) != 1) or (pc.shape[0] > 1 and pc.stride(0) < 3):
            pc = pc.float().contiguous()
        N = int(pc.shape[0])
        points = (pc, N, int(pc.stride(0)) if N > 1 else int(pc.shape[1]))
    if palette is None:
        palette = _lib.build_once(_palettes, dev, 'default', lambda: torch.tensor(DEFAULT_PALETTE, dtype=torch.float32,
                                                                                  device=dev), dev)
    else:
        palette = _lib.as_tensor(palette, dev, torch.float32).reshape(-1, 3).contiguous()
    verts, faces = verts.float().contiguous(), faces.to(torch.int32).contiguous()
    face_obj, obj_class = scene_mesh.face_obj.to(torch.int32).contiguous(), scene_mesh.obj_class.to(torch.int32).contiguous()
    keys = rasterise(verts, faces, camera.params, camera.near, W, H, points, point_px).keys
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    (h, w), F = keys.shape, int(faces.shape[0])
    out = RenderResult(new(torch.uint8, h, w, 3), new(torch.float32, h, w), new(torch.int32, h, w))
    eye, eye_p = _doubles(camera.eye)
    _lib.call("rfd_raster_shade", dev, F, K, int(palette.shape[0]), W, H, verts.data_ptr(), faces.data_ptr(),
              face_obj.data_ptr(), obj_class.data_ptr(), palette.data_ptr(), eye_p, keys.data_ptr(),
              out.ids.data_ptr(), out.depth.data_ptr(), out.image.data_ptr())
    return out
