"""place_objects: the generated meshes, each in its predicted box, in the scan's frame -- the first half of the
reference's `visualize` (demo.py:329-377; the second half, the picture, is rfdnet_amd/render.py); place_in_corners: the
same placement for given boxes (the reference's fit_shapenet_obj_to_votenet_box, ap_helper.py:404-426, is the same six steps).

The decoder leaves every mesh in its canonical cube.  The reference reads the meshes back from their files and, per
object (demo.py:351-360), in float64:
  1. subtracts the per-axis (max + min) / 2,
  2. multiplies by TRANSFORM_SHAPENET transposed,
  3. divides by the per-axis extent of the permuted points,
  4. multiplies by the box sizes,
  5. multiplies by [[cos t, sin t, 0], [-sin t, cos t, 0], [0, 0, 1]],
  6. adds the centre,
with centre, sizes and t (depth frame) derived from the box's corners (demo.py:297-310: box_params_from_corners).  Here
the same six operations run on the concatenated vertices of all objects at once (steps 1-3 are
fit.normalise_mesh_points_ragged), on whatever device the meshes are on, and are rounded to float32 once at the end.
Torch glue, no kernel: a few element-wise passes over some 10^5-10^6 vertices.

Step 5 is written out as the nine products of the matrix product, zeros included, so that a non-finite coordinate spreads
to the other axes exactly as it does in numpy's `dot`: an axis of zero extent (step 3 divides 0 by 0) leaves the whole
object NaN, and the rasteriser drops its triangles (include/rfd_render.h, rule 2).

Normals are covectors: steps 3 and 4 scale axis a by sizes_a / extent_a, so a normal is scaled by extent_a / sizes_a;
the permutation and the rotation are orthogonal and apply as they are; the result is renormalised (NaN stays NaN).
"""
import numpy as np
import torch

from .. import _lib, ragged
from .box_util import box_params_from_corners
from .fit import TRANSFORM_SHAPENET, normalise_mesh_points_ragged


class SceneMesh(object):
    """The placed objects as one ragged mesh (DESIGN.md "Ragged batches"): vertices (V,3) f32 in scan coordinates,
    faces (F,3) i32 into `vertices`, face_obj (F) i32: the object of every face, obj_off / face_off (K'+1) i32: object k owns the vertex rows
    obj_off[k] .. obj_off[k+1] and the face rows face_off[k] .. face_off[k+1], obj_class (K') i32: its semantic class,
    normals (V,3) f32 or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def place_objects(meshes, proposal_ids, parsed_predictions, with_normals=False):
    """meshes: the K' meshes of generate / evaluate (objects with .vertices (V_k,3), .faces (F_k,3) and, for with_normals,
    .vertex_normals), proposal_ids (1,K',1) or (K',1): their proposals, parsed_predictions: 'pred_corners_3d_upright_camera'
    (1,K,8,3) (after fit_mesh_to_scan: the refined corners) and 'pred_sem_cls' (1,K) (absent: class 0) -> SceneMesh on the meshes' device.  One scene, as the demo has it.
    A mesh without vertices contributes nothing (its offsets repeat)."""
    ids = np.asarray(proposal_ids.cpu() if torch.is_tensor(proposal_ids) else proposal_ids).astype(np.int64)
    ids = ids.reshape(-1) if ids.ndim < 3 else ids[0].reshape(-1)
    K = len(meshes)
    if len(ids) != K:
        raise ValueError("place_objects: %d meshes for %d proposal ids" % (K, len(ids)))
    corners_all = parsed_predictions['pred_corners_3d_upright_camera']
    dev = _mesh_device(meshes, corners_all)
    sem = parsed_predictions.get('pred_sem_cls')
    rows = torch.from_numpy(ids).to(dev)
    obj_class = torch.zeros(K, dtype=torch.int32, device=dev) if sem is None else \
        _lib.as_tensor(sem, dev, torch.int64)[0][rows].to(torch.int32)
    corners = _lib.as_tensor(corners_all, dev, torch.float64)[0][rows]
    return place_in_corners(meshes, corners, obj_class, with_normals)


_as_t = lambda a: a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _mesh_device(meshes, corners):
    return _as_t(meshes[0].vertices).device if len(meshes) else corners.device if torch.is_tensor(corners) else torch.device('cpu')


def place_in_corners(meshes, corners, obj_class, with_normals=False):
    """The placement itself, for given boxes: meshes as for place_objects, corners (K',8,3): the box of every mesh (upright
    camera frame), obj_class (K') -> SceneMesh on the meshes' device.  place_objects places the generated meshes in their
    predicted boxes with it, mesh_eval the ground-truth meshes in the ground-truth boxes."""
    K, as_t = len(meshes), _as_t
    verts = [as_t(m.vertices).reshape(-1, 3) for m in meshes]
    faces = [as_t(m.faces).reshape(-1, 3) for m in meshes]
    dev = _mesh_device(meshes, corners)
    obj_class = _lib.as_tensor(obj_class, dev, torch.int32)
    n_v = np.asarray([v.shape[0] for v in verts], np.int64)
    n_f = np.asarray([f.shape[0] if v.shape[0] else 0 for v, f in zip(verts, faces)], np.int64)
    obj_off, face_off = ragged.offsets(n_v), ragged.offsets(n_f)
    out = SceneMesh(obj_off=ragged.to_int32(obj_off, dev), face_off=ragged.to_int32(face_off, dev), obj_class=obj_class,
                    normals=None)
    if obj_off[-1] == 0:
        out.vertices = torch.zeros(0, 3, dtype=torch.float32, device=dev)
        out.faces = torch.zeros(0, 3, dtype=torch.int32, device=dev)
        out.face_obj = torch.zeros(0, dtype=torch.int32, device=dev)
        if with_normals:
            out.normals = torch.zeros(0, 3, dtype=torch.float32, device=dev)
        return out

    corners = _lib.as_tensor(corners, dev, torch.float64)
    centre, sizes, theta = box_params_from_corners(corners)
    seg = torch.from_numpy(ragged.owners(n_v)).to(dev)
    v = torch.cat([x.to(dev, torch.float64) for x in verts])
    v = normalise_mesh_points_ragged(v, seg, K) * sizes[seg]                    # steps 1-4
    c, s = torch.cos(theta)[seg], torch.sin(theta)[seg]
    zero, one = torch.zeros_like(c), torch.ones_like(c)

    def rotate(p):                                                              # step 5: p @ [[c, s, 0], [-s, c, 0], [0, 0, 1]]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        return torch.stack([(x * c + y * -s) + z * zero, (x * s + y * c) + z * zero, (x * zero + y * zero) + z * one], 1)
    out.vertices = (rotate(v) + centre[seg]).float().contiguous()               # step 6
    face_obj = ragged.owners(n_f)
    shift = torch.from_numpy(obj_off[face_obj]).to(dev)
    out.faces = (torch.cat([f.to(dev, torch.int64) for f, n in zip(faces, n_f) if n]) + shift[:, None]).to(torch.int32) \
        if face_off[-1] else torch.zeros(0, 3, dtype=torch.int32, device=dev)
    out.face_obj = ragged.to_int32(face_obj, dev)
    if with_normals:
        n = torch.cat([as_t(m.vertex_normals).reshape(-1, 3).to(dev, torch.float64) for m, k in zip(meshes, n_v) if k])
        n = n @ torch.tensor(TRANSFORM_SHAPENET, dtype=torch.float64, device=dev).t()
        # step 3's extent: that of the permuted points (the centring does not change it)
        p = torch.cat([x.to(dev, torch.float64) for x in verts]) @ \
            torch.tensor(TRANSFORM_SHAPENET, dtype=torch.float64, device=dev).t()
        idx = seg[:, None].expand(-1, 3)
        lo = torch.full((K, 3), np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, idx, p, 'amin')
        hi = torch.full((K, 3), -np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, idx, p, 'amax')
        n = rotate(n * ((hi - lo) / sizes)[seg])
        out.normals = (n / n.norm(dim=1, keepdim=True)).float().contiguous()
    return out
