"""Occupancy samples from a closed mesh on the device: the stage of the reference that turns a watertight CAD mesh into
what the completion network trains and is scored on (utils/shapenet/2_sample_mesh.py): surface points with normals,
query points with inside / outside labels, and a voxel grid.

  MeshIntersector / check_mesh_contains   external/libmesh/inside_mesh.py: is a point inside the mesh
  voxelize_surface / _interior / _ray     external/voxels.py
  sample_surface                          trimesh's mesh.sample, by this project's own rules
  sample_points                           2_sample_mesh.py's export_points
  is_watertight                           every edge in exactly two faces
  unit_cube                               2_sample_mesh.py's --resize: loc, scale and the moved vertices

The kernels are csrc/mesh_sample.hip, the rules are written out in include/rfd_sample.h and restated in numpy in
tests/mesh_sample_ref.py.  Containment and the surface voxels follow the reference's arithmetic operation by operation:
they return its bits (tests/golden/F_SMP.npz).  unit_cube is the one copy of the tools' "move the mesh into the unit
cube"; the GPU guard is _lib.need_gpu.  Everything is queued on the current stream.  A mesh is checked BEFORE any
kernel or gather touches it (one read-back): an index outside the vertex array or a coordinate that is not finite is a
ValueError here, never a fault on the device.
"""
import numpy as np
import torch

from . import _lib, ragged

MAX_HASH_RESOLUTION = 32768      # the cells are a flat int32 array
MAX_VOXEL_RESOLUTION = 1024


def unit_cube(vertices):
    """vertices (V,3) f64 on any device -> (vertices', loc (3,) f64, scale float): the mesh moved into the unit cube as
    the sampling tools store it, loc = the centre of the bounding box, scale = its largest extent, vertices' =
    (vertices - loc) * (1 / scale).  loc and scale go into every output file, so the arithmetic stays in this form: the
    reciprocal, then the product (a division gives other bits).  One read-back, for scale."""
    lo, hi = vertices.amin(0), vertices.amax(0)
    loc, scale = (lo + hi) / 2, float((hi - lo).max())
    return (vertices - loc) * (1 / scale), loc, scale


def check_sizes(**sizes):
    """ValueError for a flat size (or a number of pairs) that an int32 offset cannot hold"""
    for name, size in sizes.items():
        try:
            ragged.offsets([int(size)])
        except ValueError:
            raise ValueError("%s = %d: must stay below 2^31" % (name, size)) from None


def mesh_triangles(vertices, faces):
    """vertices (V,3) float, faces (F,3) integer tensors (any one device) -> (tri (F,3,3) f64, lo (3,), hi (3,) numpy
    f64: the bounding box of the referenced corners; None, None for F = 0).  The one place a mesh is validated, in ONE
    read-back before the gather's result is used: ValueError for an index outside [0, V) (the gather itself runs on
    clamped indices, so it cannot leave the array) and for a bounding box that is not finite."""
    if not vertices.dtype.is_floating_point or faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise ValueError("mesh: float vertices and integer faces, got %s and %s" % (vertices.dtype, faces.dtype))
    v = vertices.reshape(-1, 3).double()
    f = faces.reshape(-1, 3).long()
    V, F = int(v.shape[0]), int(f.shape[0])
    check_sizes(vertex_coordinates=3 * V, face_corners=9 * F)
    if F == 0:
        return v.new_zeros(0, 3, 3), None, None
    if V == 0:
        raise ValueError("mesh: %d faces index an empty vertex array" % F)
    tri = v[f.clamp(0, V - 1)]
    flat = tri.reshape(-1, 3)
    host = torch.cat([torch.stack([f.amin(), f.amax()]).double(), flat.amin(0), flat.amax(0)]).cpu().numpy()
    if host[0] < 0 or host[1] >= V:
        raise ValueError("mesh: face indices in [%d, %d], but %d vertices" % (host[0], host[1], V))
    lo, hi = host[2:5].copy(), host[5:8].copy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("mesh: the bounding box of the triangles is not finite (%s .. %s)" % (lo, hi))
    return tri.contiguous(), lo, hi


def rescale_constants(lo, hi, resolution):
    """rule C1 -> scale (3,), translate (3,) numpy f64; ValueError for a box without extent on an axis (the reference
    divides by zero there)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if not (hi - lo > 0).all():
        raise ValueError("mesh: the triangles' bounding box has no extent on an axis (%s .. %s)" % (lo, hi))
    scale = (resolution - 1) / (hi - lo)
    translate = 0.5 - scale * lo
    if not (np.isfinite(scale).all() and np.isfinite(translate).all()):
        raise ValueError("mesh: the triangles' bounding box is too thin to rescale (%s .. %s)" % (lo, hi))
    return scale, translate


def check_hash_resolution(resolution):
    resolution = int(resolution)
    if resolution < 2 or resolution > MAX_HASH_RESOLUTION:
        raise ValueError("hash_resolution = %d: 2 .. %d" % (resolution, MAX_HASH_RESOLUTION))
    return resolution


def check_voxel_resolution(resolution):
    resolution = int(resolution)
    if resolution < 1 or resolution > MAX_VOXEL_RESOLUTION:
        raise ValueError("resolution = %d: 1 .. %d" % (resolution, MAX_VOXEL_RESOLUTION))
    return resolution


def check_total_area(total, count):
    if count > 0 and not (total > 0 and np.isfinite(total)):
        raise ValueError("sample_surface: %d samples of a mesh of total area %s" % (count, total))


class MeshIntersector(object):
    """The reference's MeshIntersector: built once per mesh (rescale constants, rescaled triangles, cell lists as a CSR
    on the device), queried any number of times.  Two host synchronisations in the build: the mesh check with the
    bounding box, and the number of (cell, triangle) pairs."""

    @torch.no_grad()
    def __init__(self, vertices, faces, hash_resolution=512):
        self.resolution = res = check_hash_resolution(hash_resolution)
        _lib.need_gpu(vertices, faces)
        self.device = dev = vertices.device
        tri, lo, hi = mesh_triangles(vertices, faces)
        self.n_faces = F = int(tri.shape[0])
        self.n_pairs = 0
        if F == 0:
            return
        self.scale, self.translate = rescale_constants(lo, hi, res)
        self._constants = tuple(float(x) for x in self.scale) + tuple(float(x) for x in self.translate)
        self.triangles = torch.empty_like(tri)
        box = torch.empty(F, 4, dtype=torch.int32, device=dev)
        _lib.call("rfd_sample_rescale", dev, F, tri.data_ptr(), *self._constants, res, self.triangles.data_ptr(),
                  box.data_ptr())
        wide = box.long()
        self.n_pairs = int(((wide[:, 1] - wide[:, 0] + 1) * (wide[:, 3] - wide[:, 2] + 1)).sum())
        check_sizes(cell_triangle_pairs=self.n_pairs)
        count = torch.zeros(res * res, dtype=torch.int32, device=dev)
        _lib.call("rfd_sample_cells", dev, F, box.data_ptr(), res, count.data_ptr(), None)
        self.offsets = torch.zeros(res * res + 1, dtype=torch.int32, device=dev)
        self.offsets[1:] = torch.cumsum(count, 0)
        cursor = self.offsets[:-1].clone()
        self.cells = torch.empty(self.n_pairs, dtype=torch.int32, device=dev)
        _lib.call("rfd_sample_cells", dev, F, box.data_ptr(), res, cursor.data_ptr(), self.cells.data_ptr())

    def cell_order(self, points):
        """-> the permutation that orders points (n,3) f64 by cell (points that are no candidates last).  Only the
        launch's memory traffic depends on it, never a result."""
        res = self.resolution
        st = torch.tensor(self._constants, dtype=torch.float64, device=points.device)
        q = points[:, :2] * st[:2] + st[3:5]
        inside = ((q >= 0) & (q < res)).all(1)
        cell = q.clamp(0, res - 1).nan_to_num(0.).long()
        key = torch.where(inside, cell[:, 0] * res + cell[:, 1], torch.full_like(cell[:, 0], res * res))
        return torch.sort(key)[1]

    @torch.no_grad()
    def query(self, points, return_counts=False, sort_points=False):
        """points (n,3) f64 or f32 on the device -> contains (n,) bool [, n0, n1 (n,) i32: the crossings at or above and
        below every point].  sort_points: walk the points in the order of their cells, so that a wave reads one list.  Off by
        default: on MI355X the sort costs more than the walk saves ("Occupancy samples"); the result is the
        same either way."""
        _lib.need_gpu(points)
        if points.dtype not in (torch.float32, torch.float64) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("query: points are (n,3) float32 or float64, got %s %s" % (points.dtype, tuple(points.shape)))
        n, dev = int(points.shape[0]), points.device
        check_sizes(point_coordinates=3 * n)
        contains = torch.zeros(n, dtype=torch.uint8, device=dev)
        n0, n1 = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)) if return_counts else (None, None)
        if n > 0 and self.n_faces > 0:
            p = points.double().contiguous()
            order = self.cell_order(p) if sort_points else None
            out = (contains, n0, n1)
            if order is not None:
                p = p[order]
                out = [None if t is None else torch.empty_like(t) for t in out]
            _lib.call("rfd_sample_contains", dev, n, p.data_ptr(), *self._constants, self.resolution, self.n_faces,
                      self.triangles.data_ptr(), self.offsets.data_ptr(), self.cells.data_ptr(), out[0].data_ptr(),
                      _lib.ptr(out[1]), _lib.ptr(out[2]))
            if order is not None:
                for dst, src in zip((contains, n0, n1), out):
                    if dst is not None:
                        dst[order] = src
        contains = contains.bool()
        return (contains, n0, n1) if return_counts else contains


def check_mesh_contains(vertices, faces, points, hash_resolution=512):
    """The reference's function: builds an intersector, queries once -> (n,) bool"""
    return MeshIntersector(vertices, faces, hash_resolution).query(points)


@torch.no_grad()
def voxelize_surface(vertices, faces, resolution):
    """-> (R,R,R) bool: the voxels of the cube [-0.5, 0.5]^3 that a triangle overlaps (the reference's voxelize_surface)"""
    R = check_voxel_resolution(resolution)
    _lib.need_gpu(vertices, faces)
    dev = vertices.device
    check_sizes(voxels=R ** 3)
    grid = torch.zeros(R, R, R, dtype=torch.uint8, device=dev)
    tri, _, _ = mesh_triangles(vertices, faces)                      # the check; rule V1 scales the vertices first
    F = int(tri.shape[0])
    if F > 0:
        scaled = (vertices.reshape(-1, 3).double() + 0.5) * R
        tri32 = scaled[faces.reshape(-1, 3).long()].float().contiguous()
        _lib.call("rfd_sample_voxelize", dev, F, tri32.data_ptr(), R, grid.data_ptr())
    return grid.bool()


def grid_points(resolution, jitter):
    """-> (R^3,3) f64: (centre + jitter) / R - 0.5 with the centres i + 0.5 in make_3d_grid's order (x slowest)"""
    R = resolution
    c = torch.arange(R, dtype=torch.float64, device=jitter.device) + 0.5
    grid = torch.stack(torch.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    return (grid + jitter) / R - 0.5


@torch.no_grad()
def voxelize_interior(vertices, faces, resolution, jitter=None, generator=None):
    """-> (R,R,R) bool: is the (jittered) centre of every voxel inside the mesh.  jitter: (R^3,3) f64 on the device, or
    None: 0.1 (rand - 0.5) from `generator`, the reference's symmetry breaker."""
    R = check_voxel_resolution(resolution)
    _lib.need_gpu(vertices, faces)
    dev = vertices.device
    check_sizes(voxel_coordinates=3 * R ** 3)
    if jitter is None:
        jitter = 0.1 * (torch.rand(R ** 3, 3, dtype=torch.float64, device=dev, generator=generator) - 0.5)
    else:
        _lib.need_gpu(jitter)
        if jitter.dtype != torch.float64 or tuple(jitter.shape) != (R ** 3, 3):
            raise ValueError("voxelize_interior: jitter is (%d,3) float64, got %s %s" % (R ** 3, jitter.dtype, tuple(jitter.shape)))
    return check_mesh_contains(vertices, faces, grid_points(R, jitter)).reshape(R, R, R)


def voxelize_ray(vertices, faces, resolution, jitter=None, generator=None):
    """surface OR interior (the reference's voxelize_ray)"""
    return voxelize_surface(vertices, faces, resolution) | voxelize_interior(vertices, faces, resolution, jitter, generator)


@torch.no_grad()
def sample_surface(vertices, faces, count, u=None, generator=None, return_normals=False, dtype=torch.float32, cum=None):
    """-> points (count,3) `dtype`, face_index (count,) i32 [, normals (count,3) `dtype`]: points uniform on the surface.
    u (count,3) f64 in [0,1) on the device is the randomness: u0 picks the face by area, u1 and u2 the point in it
    (include/rfd_sample.h, rules S1 - S4); None: torch.rand from `generator`.  cum (F) f64 on the device: the inclusive
    prefix of the areas to draw with (rule S2 leaves its summation order open); None: torch.cumsum of the areas."""
    count = int(count)
    if count < 0:
        raise ValueError("sample_surface: count = %d" % count)
    _lib.need_gpu(vertices, faces)
    dev = vertices.device
    check_sizes(sample_coordinates=3 * count)
    points = torch.empty(count, 3, dtype=torch.float64, device=dev)
    face = torch.empty(count, dtype=torch.int32, device=dev)
    normals = torch.empty_like(points) if return_normals else None
    if count > 0:
        tri, _, _ = mesh_triangles(vertices, faces)
        F = int(tri.shape[0])
        if cum is None:
            area = torch.empty(F, dtype=torch.float64, device=dev)
            _lib.call("rfd_sample_face_areas", dev, F, tri.data_ptr(), area.data_ptr())
            cum = torch.cumsum(area, 0)
        else:
            _lib.need_gpu(cum)
            if cum.dtype != torch.float64 or tuple(cum.shape) != (F,):
                raise ValueError("sample_surface: cum is (%d,) float64, got %s %s" % (F, cum.dtype, tuple(cum.shape)))
            cum = cum.contiguous()
        check_total_area(float(cum[-1]) if F else 0., count)
        if u is None:
            u = torch.rand(count, 3, dtype=torch.float64, device=dev, generator=generator)
        else:
            _lib.need_gpu(u)
            if u.dtype != torch.float64 or tuple(u.shape) != (count, 3):
                raise ValueError("sample_surface: u is (%d,3) float64, got %s %s" % (count, u.dtype, tuple(u.shape)))
            u = u.contiguous()
        _lib.call("rfd_sample_surface", dev, count, F, tri.data_ptr(), cum.data_ptr(), u.data_ptr(), points.data_ptr(),
                  face.data_ptr(), _lib.ptr(normals))
    points = points.to(dtype)
    return (points, face, normals.to(dtype)) if return_normals else (points, face)


@torch.no_grad()
def sample_points(vertices, faces, size=100000, uniform_ratio=0.5, sigma=0.01, padding=0.1, generator=None):
    """The reference's export_points -> points (size,3) f64, occupancies (size,) bool: int(size * uniform_ratio) points
    uniform in the cube of side 1 + padding, the rest on the surface plus sigma * randn, each labelled by
    check_mesh_contains.  (The cast to f32 / f16 and packbits belong to the tool that writes the file.)"""
    _lib.need_gpu(vertices, faces)
    dev = vertices.device
    n_uniform = int(size * uniform_ratio)
    n_surface = int(size) - n_uniform
    uniform = (1 + padding) * (torch.rand(n_uniform, 3, dtype=torch.float64, device=dev, generator=generator) - 0.5)
    surface = sample_surface(vertices, faces, n_surface, generator=generator, dtype=torch.float64)[0]
    surface = surface + sigma * torch.randn(n_surface, 3, dtype=torch.float64, device=dev, generator=generator)
    points = torch.cat([uniform, surface])
    return points, check_mesh_contains(vertices, faces, points)


def is_watertight(faces):
    """faces (F,3) integer tensor -> bool: every undirected edge lies in exactly two faces.  Torch glue, no kernel."""
    f = faces.reshape(-1, 3).long()
    if f.shape[0] == 0:
        return False
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    lo, hi = e.amin(1), e.amax(1)
    width = hi.max() + 1
    counts = torch.unique(lo * width + hi, return_counts=True)[1]
    return bool((counts == 2).all())
