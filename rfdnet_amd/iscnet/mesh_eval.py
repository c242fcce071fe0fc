"""Mesh mAP: per-object voxel grids and the mesh IoU of every (prediction, ground truth) pair on the device -- the
counterpart of the mesh half of the reference's `--mode test` sweep:

  voxelize_objects    batch_load_pred_data / batch_load_gt_data (net_utils/ap_helper.py:429-478) without binvox
  mesh_iou            compute_mesh_iou (net_utils/eval_det.py:27-83), one call per pair over a process pool there
  scene_mesh_iou      the mesh half of assembly_pred_map_cls / assembly_gt_map_cls (:267-323, :371-401)
  MeshAPCalculator    compute_metrics_w_mesh (:84-122)
  load_gt_meshes      the ShapeNet meshes of a scene's ground-truth rows (:380-384)

The rules M1 - M5 are written out in include/rfd_mesh_eval.h and restated in numpy in tests/mesh_iou_f64.py; the
kernels are csrc/mesh_iou.hip.  Everything downstream of the voxel grids returns the reference's own results
(tests/golden/F_MIOU.npz); the grids themselves are this project's contract.

Deviations from the reference: the surface and interior grids of mesh_sample (pinned to the reference's libmesh /
voxels libraries) stand in for binvox's `exact` and `wireframe + dilated_carving` grids -- binvox is an external
program and its carving is not reproduced; a world point is looked up with `floor`, not trimesh's `round` about the
voxel centre (they differ only exactly on a cell boundary); a detection that takes part but has no mesh has mesh IoU 0
with everything, where the reference raises ValueError.

voxelize_objects has two paths that give the same bits.  'batched' (the default; rules B1 - B7 of the header,
csrc/objgrid.hip) voxelises all objects of a scene in one ragged batch: five launches and two read-backs whatever their
number.  'per_object' voxelises each object on its own by mesh_sample's voxelisers, a few host synchronisations per
object (MeshIntersector), and packs it; it is the cross-check.  tools/mesh_eval_cost.py measures both beside the IoU
kernel.
"""
import os

import numpy as np
import torch

from .. import _lib, mesh_sample
from . import scene as scene_module
from .evaluation import APCalculator
from .generator import Mesh

VOXEL_SIZE = 0.047       # ap_helper.py:267, :371
MAX_DIM = 256
MAX_PRED, MAX_GT = 1024, 256     # rfd_ap_match's limits
MAX_OBJECTS = 65535              # one batch of rfd_objgrid_*
HASH_RESOLUTION, BINS = 512, 32  # rules B3 and B6


def object_frame(lo, hi, voxel_size=VOXEL_SIZE):
    """Rule M1 on the host, float64: the per-axis extent lo, hi (3,) of an object's placed vertices ->
    (lo (3,) f64, L, cell, D), or None where the object has no grid (L not finite or 0).  D > 256: ValueError."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        L = np.max(hi - lo)
    if not np.isfinite(L) or L == 0:
        return None
    D = max(int(L / voxel_size), 2)
    if D > MAX_DIM:
        raise ValueError("mesh IoU: an object of extent %g needs a %d^3 grid at voxel size %g; at most %d^3"
                         % (L, D, voxel_size, MAX_DIM))
    return lo, float(L), float(L / D), D


def words_of(D):
    return D * D * ((D + 63) // 64)


class ObjectGrids(object):
    """The object table of include/rfd_mesh_eval.h plus the packed words, on one device: frame (N,4) f64 (lo, cell),
    dim (N) i32 (0: no grid), off (N) i64, cnt (N,2) i32 (|U|, |S|), words (n_words) i64 (the bit words).  `dims` is
    the host's copy of dim."""

    def __init__(self, frame, dim, off, cnt, words, dims):
        self.frame, self.dim, self.off, self.cnt, self.words, self.dims = frame, dim, off, cnt, words, dims

    def __len__(self):
        return len(self.dims)

    @property
    def n_words(self):
        return int(self.words.numel())

    @property
    def device(self):
        return self.words.device

    def grid(self, i):
        """-> U of object i as a (D,D,D) bool tensor, unpacked on the device; None for an object without a grid"""
        D = int(self.dims[i])
        if D == 0:
            return None
        W = (D + 63) // 64
        # the host's offsets are those of the table: assigned in object order
        at = sum(words_of(int(d)) for d in self.dims[:i])
        w = self.words[at:at + D * D * W].view(D, D, W, 1)
        bits = (w >> torch.arange(64, device=w.device)) & 1
        return bits.reshape(D, D, W * 64)[:, :, :D].bool()


@torch.no_grad()
def pack_grids(objects, device):
    """objects: per object None (no grid) or (S, I, lo, cell) with S, I (D,D,D) bool / u8 tensors on `device` (or
    numpy), lo (3,) and cell floats -> ObjectGrids: one rfd_objgrid_pack launch per object into one shared buffer."""
    device = torch.device(device)
    N = len(objects)
    dims = np.zeros(N, np.int32)
    frame = np.zeros((N, 4), np.float64)
    off = np.zeros(N, np.int64)
    total = 0
    for i, o in enumerate(objects):
        if o is None:
            continue
        S, I, lo, cell = o
        D = int(S.shape[0])
        if tuple(S.shape) != (D, D, D) or tuple(I.shape) != (D, D, D):
            raise ValueError("pack_grids: S and I are (D,D,D), got %s and %s" % (tuple(S.shape), tuple(I.shape)))
        if D > MAX_DIM:
            raise ValueError("pack_grids: D = %d, at most %d" % (D, MAX_DIM))
        dims[i], off[i] = D, total
        frame[i, :3], frame[i, 3] = np.asarray(lo, np.float64), float(cell)
        total += words_of(D)
    words = torch.zeros(max(total, 1), dtype=torch.int64, device=device)
    cnt = torch.zeros(N, 2, dtype=torch.int32, device=device)
    for i, o in enumerate(objects):
        if o is None:
            continue
        S = _lib.as_tensor(o[0], device, torch.uint8).contiguous()
        I = _lib.as_tensor(o[1], device, torch.uint8).contiguous()
        _lib.call("rfd_objgrid_pack", device, int(dims[i]), S.data_ptr(), I.data_ptr(), words.data_ptr(), int(off[i]),
                  int(words.numel()), cnt[i].data_ptr())
    up = lambda a: torch.from_numpy(a).to(device)
    return ObjectGrids(up(frame), up(dims), up(off), cnt, words, dims)


@torch.no_grad()
def object_grids(scene_mesh, voxel_size=VOXEL_SIZE):
    """Rules M1 and M2 for every object of a SceneMesh -> the list pack_grids takes: None or (S, I, lo, cell).
    One read-back for all frames, then per object the two voxelisers of mesh_sample."""
    _lib.need_gpu(scene_mesh.vertices)
    dev = scene_mesh.vertices.device
    obj_off = scene_mesh.obj_off.cpu().numpy().astype(np.int64)
    face_off = scene_mesh.face_off.cpu().numpy().astype(np.int64)
    N = len(obj_off) - 1
    if N == 0:
        return []
    v = scene_mesh.vertices.double()
    seg = torch.repeat_interleave(torch.arange(N, device=dev), torch.from_numpy(np.diff(obj_off)).to(dev))
    idx = seg[:, None].expand(-1, 3)
    # amin / amax let a NaN through (an object of zero extent is NaN after the placement): it then has no grid
    lo = torch.full((N, 3), np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, idx, v, 'amin')
    hi = torch.full((N, 3), -np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, idx, v, 'amax')
    L = (hi - lo).amax(1)
    unit = (v - lo[seg]) / L[seg, None] - 0.5                                      # M2's map, for all objects at once
    # the extent of what the faces reference, in the unit cube: a flat object has no interior (and the intersector
    # refuses it)
    faces = scene_mesh.faces.long()
    fobj = scene_mesh.face_obj.long()[:, None, None].expand(-1, 3, 3).reshape(-1, 3)
    corner = unit[faces.clamp(0, max(int(v.shape[0]) - 1, 0))].reshape(-1, 3) if faces.numel() else unit[:0]
    tlo = torch.full((N, 3), np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, fobj, corner, 'amin')
    thi = torch.full((N, 3), -np.inf, dtype=torch.float64, device=dev).scatter_reduce(0, fobj, corner, 'amax')
    host = torch.cat([lo, hi, tlo, thi], 1).cpu().numpy()
    out = []
    for k in range(N):
        n_f = int(face_off[k + 1] - face_off[k])
        fr = object_frame(host[k, 0:3], host[k, 3:6], voxel_size) if obj_off[k + 1] > obj_off[k] and n_f else None
        if fr is None:
            out.append(None)
            continue
        lo_k, _, cell, D = fr
        vk = unit[obj_off[k]:obj_off[k + 1]]
        fk = faces[face_off[k]:face_off[k + 1]] - int(obj_off[k])
        S = mesh_sample.voxelize_surface(vk, fk, D)
        if (host[k, 9:12] - host[k, 6:9] > 0).all():
            centres = mesh_sample.grid_points(D, torch.zeros(1, 3, dtype=torch.float64, device=dev))   # no jitter
            I = mesh_sample.check_mesh_contains(vk, fk, centres).reshape(D, D, D)
        else:
            I = torch.zeros_like(S)
        out.append((S, I, lo_k, cell))
    return out


class BatchedWords(object):
    """What batched_words leaves on the device before the union: the table (frame (N,4) f64, dims (N) i32 and off (N)
    i64 as numpy, dim / off their device copies) and the surface and interior words S, I (n_words) i64."""

    def __init__(self, frame, dims, off, dim, off_dev, S, I):
        self.frame, self.dims, self.off, self.dim, self.off_dev, self.S, self.I = frame, dims, off, dim, off_dev, S, I

    def table(self):
        """the table arguments of the rfd_objgrid_* launchers: N, the host copy, the device copy, n_words"""
        return (len(self.dims), self.dims.ctypes.data, self.off.ctypes.data, self.dim.data_ptr(), self.off_dev.data_ptr(),
                int(self.S.numel()))


def _extents(values, owner, N, spread=256):
    """values (n,C) f64, owner (n) i64 in [0, N) -> (lo, hi) (N,C): the minimum and maximum of every owner's rows, +inf /
    -inf for an owner without rows; a NaN goes through.  scatter_reduce's atomics serialise on one address, and a scene
    has few objects and millions of rows, so every owner's rows are dealt over `spread` slots first."""
    n, C = values.shape
    slot = (owner * spread + torch.arange(n, device=values.device) % spread)[:, None].expand(-1, C)
    start = lambda sign: torch.full((N * spread, C), sign * np.inf, dtype=values.dtype, device=values.device)
    return (start(1).scatter_reduce(0, slot, values, 'amin').view(N, spread, C).amin(1),
            start(-1).scatter_reduce(0, slot, values, 'amax').view(N, spread, C).amax(1))


@torch.no_grad()
def batched_words(scene_mesh, voxel_size=VOXEL_SIZE):
    """Rules B1 - B6 of include/rfd_mesh_eval.h for every object of a SceneMesh at once -> BatchedWords.  Two read-backs
    whatever the number of objects: the frames (with the offsets, the bounding boxes of the referenced corners and the
    range of every object's face indices: everything the host decides on), and the number of (bin, triangle) pairs.
    At most four launches: the surface, the two passes of the bins, the interior."""
    _lib.need_gpu(scene_mesh.vertices)
    dev = scene_mesh.vertices.device
    N = int(scene_mesh.obj_off.numel()) - 1
    V, F = int(scene_mesh.vertices.shape[0]), int(scene_mesh.faces.shape[0])
    if N > MAX_OBJECTS:
        raise ValueError("mesh IoU: %d objects in one batch, at most %d" % (N, MAX_OBJECTS))
    up = lambda a: torch.from_numpy(a).to(dev)
    if N <= 0:
        empty = torch.zeros(1, dtype=torch.int64, device=dev)
        return BatchedWords(np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros(0, np.int64), up(np.zeros(0, np.int32)),
                            up(np.zeros(0, np.int64)), empty, empty.clone())
    v = scene_mesh.vertices.double()
    seg = torch.bucketize(torch.arange(V, device=dev), scene_mesh.obj_off[1:].long(), right=True).clamp(max=N - 1)
    # amin / amax let a NaN through (an object of zero extent is NaN after the placement): it then has no grid
    lo, hi = _extents(v, seg, N)
    L = (hi - lo).amax(1)
    unit = (v - lo[seg]) / L[seg, None] - 0.5                                      # B1's map, for all objects at once
    faces = scene_mesh.faces.long().reshape(-1, 3)
    face_obj = scene_mesh.face_obj.long()
    # the gathers run on clamped indices: they cannot leave the vertex array, whatever the faces hold
    tri = unit[faces.clamp(0, max(V - 1, 0))] if F and V else unit.new_zeros(F, 3, 3)
    # per face first (the minimum of minima is the minimum), then per object
    tlo, thi = _extents(tri.amin(1), face_obj, N)[0], _extents(tri.amax(1), face_obj, N)[1]
    flo, fhi = _extents(faces.amin(1, keepdim=True).double(), face_obj, N)[0], \
        _extents(faces.amax(1, keepdim=True).double(), face_obj, N)[1]
    host = torch.cat([torch.cat([lo, hi, tlo, thi, flo, fhi], 1).reshape(-1),
                      scene_mesh.obj_off.double(), scene_mesh.face_off.double()]).cpu().numpy()      # THE read-back
    stats = host[:14 * N].reshape(N, 14)
    obj_off = host[14 * N:14 * N + N + 1].astype(np.int64)
    face_off = host[14 * N + N + 1:].astype(np.int64)
    dims, off, frame, consts = np.zeros(N, np.int32), np.zeros(N, np.int64), np.zeros((N, 4)), np.zeros((N, 6))
    total = 0
    for k in range(N):
        n_v, n_f = int(obj_off[k + 1] - obj_off[k]), int(face_off[k + 1] - face_off[k])
        fr = object_frame(stats[k, 0:3], stats[k, 3:6], voxel_size) if n_v > 0 and n_f > 0 else None
        if fr is None:
            continue
        first, last = stats[k, 12] - obj_off[k], stats[k, 13] - obj_off[k]
        if first < 0 or last >= n_v:
            raise ValueError("mesh: face indices in [%d, %d], but %d vertices" % (first, last, n_v))
        lo_k, _, cell, D = fr
        dims[k], off[k] = D, total
        frame[k, :3], frame[k, 3] = lo_k, cell
        total += words_of(D)
        if (stats[k, 9:12] - stats[k, 6:9] > 0).all():                             # else: flat, no interior (B3)
            consts[k, :3], consts[k, 3:] = mesh_sample.rescale_constants(stats[k, 6:9], stats[k, 9:12], HASH_RESOLUTION)
    S = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    I = torch.zeros_like(S)
    out = BatchedWords(frame, dims, off, up(dims), up(off), S, I)
    if total == 0:
        return out
    fo32 = scene_mesh.face_obj.to(torch.int32).contiguous()
    # rule B2 / V1: ((u + 0.5) * D_k)[faces] in f64, rounded once to f32
    tri32 = ((unit + 0.5) * up(dims.astype(np.float64))[seg, None])[faces.clamp(0, V - 1)].float().contiguous()
    _lib.call("rfd_objgrid_surface", dev, F, tri32.data_ptr(), fo32.data_ptr(), *out.table(), S.data_ptr())
    if not consts.any():
        return out
    tri, consts_dev = tri.contiguous(), up(consts)
    count = torch.zeros(N * BINS * BINS, dtype=torch.int32, device=dev)
    bins = lambda cursor, lst, n: _lib.call("rfd_objgrid_bins", dev, F, tri.data_ptr(), fo32.data_ptr(), N, dims.ctypes.data,
                                            out.dim.data_ptr(), consts_dev.data_ptr(), cursor.data_ptr(), _lib.ptr(lst), n)
    bins(count, None, 0)
    offsets = torch.zeros(N * BINS * BINS + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    n_pairs = int(offsets[-1])                                                      # the second read-back
    mesh_sample.check_sizes(bin_triangle_pairs=n_pairs)                             # before anything is allocated
    if n_pairs == 0:
        return out
    offsets = offsets.to(torch.int32)
    lst = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    bins(offsets[:-1].clone(), lst, n_pairs)
    _lib.call("rfd_objgrid_interior", dev, F, tri.data_ptr(), *out.table(), consts_dev.data_ptr(), offsets.data_ptr(),
              lst.data_ptr(), n_pairs, I.data_ptr())
    return out


@torch.no_grad()
def voxelize_batched(scene_mesh, voxel_size=VOXEL_SIZE):
    """batched_words, then rule B7 (one rfd_objgrid_finish launch) -> ObjectGrids"""
    b = batched_words(scene_mesh, voxel_size)
    dev = b.S.device
    cnt = torch.zeros(len(b.dims), 2, dtype=torch.int32, device=dev)
    _lib.call("rfd_objgrid_finish", dev, *b.table(), b.S.data_ptr(), b.I.data_ptr(), cnt.data_ptr())
    return ObjectGrids(torch.from_numpy(b.frame).to(dev), b.dim, b.off_dev, cnt, b.S, b.dims)


def voxelize_objects(scene_mesh, voxel_size=VOXEL_SIZE, method='batched'):
    """SceneMesh (scene.place_objects / place_in_corners) -> ObjectGrids, one row per object.  method: 'batched' (all
    objects in one ragged batch: csrc/objgrid.hip, launches and read-backs independent of their number) or
    'per_object' (one object at a time through mesh_sample's voxelisers and rfd_objgrid_pack); the same bits."""
    if method == 'batched':
        return voxelize_batched(scene_mesh, voxel_size)
    if method == 'per_object':
        return pack_grids(object_grids(scene_mesh, voxel_size), scene_mesh.vertices.device)
    raise ValueError("voxelize_objects: method is 'batched' or 'per_object', got %r" % (method,))


def _check_counts(P, G):
    if P > MAX_PRED or G > MAX_GT:
        raise ValueError("mesh IoU: %d predictions x %d ground truths; at most %d x %d" % (P, G, MAX_PRED, MAX_GT))


@torch.no_grad()
def mesh_iou_counts(pred_grids, gt_grids):
    """-> counts (P,G,2) i32 on the device: a_AB, a_BA of every pair (one rfd_mesh_iou_counts launch)"""
    P, G = len(pred_grids), len(gt_grids)
    dev = pred_grids.device
    counts = torch.zeros(P, G, 2, dtype=torch.int32, device=dev)
    a, b = pred_grids, gt_grids
    _lib.call("rfd_mesh_iou_counts", dev, P, G, a.frame.data_ptr(), a.dim.data_ptr(), a.off.data_ptr(),
              a.words.data_ptr(), a.n_words, b.frame.data_ptr(), b.dim.data_ptr(), b.off.data_ptr(), b.words.data_ptr(),
              b.n_words, counts.data_ptr())
    return counts


@torch.no_grad()
def scatter_iou(pred_grids, gt_grids, counts, iou, rows_p=None, rows_g=None):
    """Rule M5 into iou (K,G') f64 at (rows_p[p], rows_g[g]) (None: the identity); one rfd_mesh_iou_finalize launch"""
    dev = iou.device
    as_rows = lambda r: None if r is None else _lib.as_tensor(r, dev, torch.int32).contiguous()
    rows_p, rows_g = as_rows(rows_p), as_rows(rows_g)
    _lib.call("rfd_mesh_iou_finalize", dev, len(pred_grids), len(gt_grids), counts.data_ptr(), pred_grids.cnt.data_ptr(),
              gt_grids.cnt.data_ptr(), _lib.ptr(rows_p), _lib.ptr(rows_g), iou.shape[0], iou.shape[1], iou.data_ptr())
    return iou


def mesh_iou(pred_grids, gt_grids):
    """-> (iou (P,G) f64, counts (P,G,2) i32) on the device"""
    counts = mesh_iou_counts(pred_grids, gt_grids)
    iou = torch.zeros(len(pred_grids), len(gt_grids), dtype=torch.float64, device=counts.device)
    return scatter_iou(pred_grids, gt_grids, counts, iou), counts


def _on(a, device, dtype):
    """a tensor as it is (its own float / integer type), anything else through numpy as `dtype`, on `device`"""
    return a.to(device) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).to(device, dtype)


def _as_mesh(m, device):
    if m is None:
        return Mesh(torch.zeros(0, 3, dtype=torch.float64, device=device), torch.zeros(0, 3, dtype=torch.int64, device=device))
    v, f = (m.vertices, m.faces) if hasattr(m, 'vertices') else m
    return Mesh(_on(v, device, torch.float64), _on(f, device, torch.int64))


@torch.no_grad()
def scene_mesh_iou(meshes, proposal_ids, parsed_predictions, parsed_gts, gt_meshes, voxel_size=VOXEL_SIZE,
                   method='batched'):
    """The mesh IoU matrix of ONE scene (the reference asserts bsize == 1 too) -> (1,K,G) f64 on the device, what
    evaluation.scene_records takes as `mesh_iou`.
    meshes, proposal_ids: the generated meshes and their proposals (ISCNet.generate); they are placed in
    parsed_predictions['pred_corners_3d_upright_camera'] (1,K,8,3), the boxes that are scored.
    gt_meshes: one (vertices, faces) (or an object with these attributes) per ground-truth row with
    box_label_mask == 1, in row order; None for a missing mesh.  They are placed in the ground-truth corners.
    A proposal without a generated mesh, and a ground truth without one, keep IoU 0 with everything.
    method: voxelize_objects' ('batched' or 'per_object')."""
    corners = parsed_predictions['pred_corners_3d_upright_camera']
    _lib.need_gpu(corners)
    dev = corners.device
    if corners.shape[0] != 1:
        raise ValueError("mesh IoU runs on one scene at a time, got a batch of %d" % corners.shape[0])
    K = corners.shape[1]
    gt_corners = _lib.as_tensor(parsed_gts['gt_corners_3d_upright_camera'], dev, torch.float64)
    G = gt_corners.shape[1]
    iou = torch.zeros(1, K, G, dtype=torch.float64, device=dev)
    rows_g = torch.nonzero(_lib.as_tensor(parsed_gts['box_label_mask'], dev, torch.float32)[0] == 1)[:, 0]
    if len(gt_meshes) != rows_g.numel():
        raise ValueError("gt_meshes: %d meshes for %d ground-truth boxes" % (len(gt_meshes), rows_g.numel()))
    ids = proposal_ids.reshape(-1).to(dev) if torch.is_tensor(proposal_ids) else \
        torch.as_tensor(np.asarray(proposal_ids).reshape(-1), device=dev)
    _check_counts(int(ids.numel()), int(rows_g.numel()))
    if ids.numel() == 0 or rows_g.numel() == 0:
        return iou
    pred = scene_module.place_objects([_as_mesh(m, dev) for m in meshes], ids.view(1, -1, 1), parsed_predictions)
    gt_cls = _lib.as_tensor(parsed_gts['sem_cls_label'], dev, torch.int32)[0][rows_g]
    gt = scene_module.place_in_corners([_as_mesh(m, dev) for m in gt_meshes], gt_corners[0][rows_g], gt_cls)
    pg, gg = voxelize_objects(pred, voxel_size, method), voxelize_objects(gt, voxel_size, method)
    scatter_iou(pg, gg, mesh_iou_counts(pg, gg), iou[0], ids, rows_g)
    return iou


METRIC_KEYS = ('accuracy', 'completeness', 'chamfer_l1', 'chamfer_sq', 'precision', 'recall', 'fscore',
               'normal_consistency', 'rms')


@torch.no_grad()
def scene_mesh_distance(meshes, proposal_ids, parsed_predictions, parsed_gts, gt_meshes, pairs, count=10000,
                        thresholds=(0.05, 0.10), u_a=None, u_b=None, generator=None):
    """The surface metrics of ONE scene's (proposal, ground truth) pairs -> mesh_distance.mesh_metrics' dict, one row per
    pair, f64 on the device.  The generated meshes and the ground-truth meshes are placed exactly as scene_mesh_iou places
    them (same arguments); pairs (P,2) or (P,3) integers: (proposal id, ground-truth row[, class]), the rows of
    evaluation.proposal_to_gt for the scene.  The predictions are mesh_metrics' A, the ground truths its B: `precision`
    is the share of the predicted surface near the true one, `recall` the share of the true surface that is covered.
    A pair whose proposal has no mesh (not among proposal_ids, or generated empty), or whose ground truth is None or not
    a labelled row, gets NaN in every metric.  u_a (K',count,3) / u_b (G',count,3): the randomness of the samples, one
    slab per mesh in `meshes` / `gt_meshes` order."""
    from .. import mesh_distance
    corners = parsed_predictions['pred_corners_3d_upright_camera']
    _lib.need_gpu(corners)
    dev = corners.device
    if corners.shape[0] != 1:
        raise ValueError("mesh distance runs on one scene at a time, got a batch of %d" % corners.shape[0])
    gt_corners = _lib.as_tensor(parsed_gts['gt_corners_3d_upright_camera'], dev, torch.float64)
    rows_g = torch.nonzero(_lib.as_tensor(parsed_gts['box_label_mask'], dev, torch.float32)[0] == 1)[:, 0]
    ids = proposal_ids.reshape(-1).to(dev) if torch.is_tensor(proposal_ids) else \
        torch.as_tensor(np.asarray(proposal_ids).reshape(-1), device=dev)
    if len(meshes) != ids.numel():
        raise ValueError("meshes: %d meshes for %d proposal ids" % (len(meshes), ids.numel()))
    if len(gt_meshes) != rows_g.numel():
        raise ValueError("gt_meshes: %d meshes for %d ground-truth boxes" % (len(gt_meshes), rows_g.numel()))
    pairs = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, np.int64)
    pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim > 1 else 2)[:, :2]
    P, T = len(pairs), len(thresholds)
    nan = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    out = {k: nan(P, T) if k in ('precision', 'recall', 'fscore') else nan(P) for k in METRIC_KEYS}
    host = torch.cat([ids.long(), rows_g.long()]).cpu().numpy()                # the one copy: who has a mesh
    ids_h, rows_h = host[:ids.numel()], host[ids.numel():]
    mesh_of = {int(p): m for m, p in reversed(list(enumerate(ids_h)))}         # the first mesh of a proposal
    gt_of = {int(g): j for j, g in enumerate(rows_h) if gt_meshes[j] is not None}
    known = np.array([int(p) in mesh_of and int(g) in gt_of for p, g in pairs], bool)
    if not known.any():
        if T > mesh_distance.MAX_THRESHOLDS:
            raise ValueError("%d thresholds: at most %d" % (T, mesh_distance.MAX_THRESHOLDS))
        return out
    local = np.array([[mesh_of[int(p)], gt_of[int(g)]] for p, g in pairs[known]], np.int64)
    pred = scene_module.place_objects([_as_mesh(m, dev) for m in meshes], ids.view(1, -1, 1), parsed_predictions)
    gt_cls = _lib.as_tensor(parsed_gts['sem_cls_label'], dev, torch.int32)[0][rows_g]
    gt = scene_module.place_in_corners([_as_mesh(m, dev) for m in gt_meshes], gt_corners[0][rows_g], gt_cls)
    got = mesh_distance.mesh_metrics(pred, gt, local, count, thresholds, u_a, u_b, generator)
    at = torch.from_numpy(np.nonzero(known)[0]).to(dev)
    for k in METRIC_KEYS:
        out[k][at] = got[k]
    return out


def class_means(metrics, classes, key='chamfer_l1'):
    """metrics: scene_mesh_distance's dict (or several, concatenated by the caller), classes (P) integers -> {class: the
    mean of metrics[key] over the class's pairs that have a number}; what demo.py and tools/eval_sweep.py print."""
    values = metrics[key].detach().cpu().numpy()
    classes = np.asarray(classes.cpu() if torch.is_tensor(classes) else classes).reshape(-1)
    out = {}
    for c in np.unique(classes):
        x = values[classes == c]
        x = x[np.isfinite(x).reshape(len(x), -1).all(1)]
        if len(x):
            out[int(c)] = x.mean(0).tolist() if x.ndim > 1 else float(x.mean())
    return out


class MeshAPCalculator(APCalculator):
    """compute_metrics_w_mesh (ap_helper.py:84-122) on records with mesh flags (scene_records(mesh_iou=...)):
    compute_metrics() returns the box dict of APCalculator plus '<cls> Average Precision_mesh', 'mAP_mesh',
    '<cls> Recall_mesh', 'AR_mesh' from the same curve code on 'tp_mesh'."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None):
        super(MeshAPCalculator, self).__init__(ap_iou_thresh, class2type_map)
        self.evaluate_mesh = True

    def compute_metrics(self, use_07_metric=True):
        """VOC07 by default, as eval_det_multiprocessing_w_mesh has it"""
        from .evaluation import merge_records
        if self.records and 'tp_mesh' not in merge_records(self.records, self.ap_iou_thresh):
            raise ValueError("MeshAPCalculator: the records carry no mesh flags (scene_records(mesh_iou=...))")
        flags = 'tp_mesh' if self.records else 'tp'
        rets = []
        for ti in range(len(self.ap_iou_thresh)):
            ret = self.metrics_of(self.class_curves(ti, use_07_metric))
            ret.update(self.metrics_of(self.class_curves(ti, use_07_metric, flags), '_mesh'))
            rets.append(ret)
        return rets[0] if self.single else rets


def load_gt_meshes(shapenet_path, catids, ids):
    """<shapenet_path>/<catid>/<id>.off for every ground-truth row -> [(vertices (V,3) f64, faces (F,3) i32 numpy)];
    None for a file that does not exist"""
    from ..io import read_mesh
    out = []
    for cat, name in zip(catids, ids):
        path = os.path.join(shapenet_path, str(cat), str(name) + '.off')
        out.append(read_mesh(path) if os.path.exists(path) else None)
    return out
