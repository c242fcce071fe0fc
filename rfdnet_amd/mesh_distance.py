"""Exact point-to-mesh distance on the device and the surface metrics built on it: how far a predicted surface is from
the true one (Chamfer distance, F-score, normal consistency, point coverage), for one mesh or a ragged batch of them.

  MeshDistance            built once per batch (valid faces, frames, cell lists), queried any number of times
  point_mesh_distance     the single-mesh case
  sample_surface_ragged   `count` points (with normals) on every object of a batch
  mesh_metrics            accuracy, completeness, Chamfer, precision / recall / F-score, normal consistency, RMS per pair

The kernels are csrc/mesh_dist.hip, the rules D1 - D8 are written out in include/rfd_mesh_dist.h and restated in numpy
float64 in tests/mesh_dist_f64.py.  The answer of a query is the least key (squared distance, face row) over the valid
faces of its object: a total order, so the cells, the batch and the order of the queries only decide the cost.  A face
with an index out of range, a corner that is not finite or no area takes no part (rule D1): nothing is refused for its
data, nothing leaves its arrays.  Everything is queued on the current stream; the number of launches and read-backs
depends on neither the number of objects nor the number of pairs."""
import numpy as np
import torch

from . import _lib, mesh_batch, ragged
from .mesh_sample import check_sizes

MAX_CELLS = 64
MAX_THRESHOLDS = 8
_SPREAD = 256


def default_cells(n_valid):
    """R = clamp(ceil(cbrt(F_valid / 8)), 1, 64): about eight faces per cell of a filled frame.  A choice, not a tuned
    value: no result depends on it."""
    return np.clip(np.ceil(np.cbrt(np.asarray(n_valid, np.float64) / 8.)), 1, MAX_CELLS).astype(np.int64)


def _extents(values, owner, N):
    """values (n,3) f64, owner (n) i64 in [0, N) -> (lo, hi) (N,3): +inf / -inf for an owner without rows.  The rows of an
    owner are dealt over _SPREAD slots first, so that scatter_reduce's atomics do not serialise on one address."""
    n = values.shape[0]
    slot = (owner * _SPREAD + torch.arange(n, device=values.device) % _SPREAD)[:, None].expand(-1, 3)
    start = lambda sign: torch.full((N * _SPREAD, 3), sign * np.inf, dtype=values.dtype, device=values.device)
    return (start(1).scatter_reduce(0, slot, values, 'amin').view(N, _SPREAD, 3).amin(1),
            start(-1).scatter_reduce(0, slot, values, 'amax').view(N, _SPREAD, 3).amax(1))


def _unpack(vertices, faces, vert_off, face_off):
    """a SceneMesh, one mesh, or a flat batch -> (vertices, faces with indices LOCAL to their object, vend, tend, K)"""
    if hasattr(vertices, 'obj_off'):                                  # a SceneMesh: global indices, offsets on the device
        sm = vertices
        mesh_batch.check_tensors(sm.vertices, sm.faces)
        off = torch.cat([sm.obj_off.reshape(-1), sm.face_off.reshape(-1)]).cpu().numpy()      # the one copy
        vend, tend, K = mesh_batch.check_offsets(off[:len(off) // 2], off[len(off) // 2:])
        faces = sm.faces.reshape(-1, 3).long() - sm.obj_off.long()[sm.face_obj.long()][:, None]
        return sm.vertices, faces, vend, tend, K
    mesh_batch.check_tensors(vertices, faces)
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise TypeError("faces must be integers, not %s" % faces.dtype)
    vertices, faces = vertices.reshape(-1, 3), faces.reshape(-1, 3)
    if vert_off is None and face_off is None:
        vert_off, face_off = [0, vertices.shape[0]], [0, faces.shape[0]]
    elif vert_off is None or face_off is None:
        raise ValueError("vert_off and face_off come together")
    to_host = lambda o: o.cpu().numpy() if torch.is_tensor(o) else o
    vend, tend, K = mesh_batch.check_offsets(to_host(vert_off), to_host(face_off))
    if vend[-1] != vertices.shape[0] or tend[-1] != faces.shape[0]:
        raise ValueError("the offsets end at %d vertices and %d faces, the batch has %d and %d"
                         % (vend[-1], tend[-1], vertices.shape[0], faces.shape[0]))
    return vertices, faces, vend, tend, K


class MeshDistance(object):
    """MeshDistance(vertices (V,3) f32 / f64, faces (F,3) integers[, vert_off, face_off (K + 1): the objects' vertex and
    face rows, face indices local to their object][, cells]) or MeshDistance(scene_mesh[, cells=]): the valid faces
    (rule D1), the frames (D2) and the cell lists (D3) of a ragged batch, built once.  cells: 1 .. 64 cells per axis for
    every object, None: default_cells of every object's valid faces.  Two read-backs, whatever K: the frames, and the
    number of (cell, triangle) pairs."""

    @torch.no_grad()
    def __init__(self, vertices, faces=None, vert_off=None, face_off=None, cells=None):
        if cells is not None and not 1 <= int(cells) <= MAX_CELLS:
            raise ValueError("cells = %s: 1 .. %d" % (cells, MAX_CELLS))
        v, f, vend, tend, K = _unpack(vertices, faces, vert_off, face_off)
        self.device = dev = v.device
        self.K, self.vend, self.tend = K, vend, tend
        self.V, self.F = V, F = int(vend[-1]), int(tend[-1])
        ragged.offsets([9 * F])
        ragged.offsets([3 * V])
        self.vend_dev, self.tend_dev = ragged.to_int32(np.stack([vend, tend]), dev)
        v = v.double().contiguous()
        f = f.to(torch.int32).contiguous()
        self.tri = torch.zeros(F, 3, 3, dtype=torch.float64, device=dev)
        self.valid = torch.zeros(F, dtype=torch.uint8, device=dev)
        self.fobj = torch.zeros(F, dtype=torch.int32, device=dev)
        self._faces_pass(v, f, None)
        # rule D2 on the host, from one read-back: the corners' extents and the valid faces of every object
        lo, hi, n_valid = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K, np.int64)
        if F > 0:
            owner = self.fobj.long()
            corner_owner = owner.repeat_interleave(3)
            keep = self.valid.bool().repeat_interleave(3)
            elo, ehi = _extents(self.tri.reshape(-1, 3)[keep], corner_owner[keep], K)
            count = torch.zeros(K, dtype=torch.float64, device=dev).index_add_(0, owner, self.valid.double())
            host = torch.cat([elo, ehi, count[:, None]], 1).cpu().numpy()
            n_valid = host[:, 6].astype(np.int64)
            some = n_valid > 0
            lo[some], hi[some] = host[some, 0:3], host[some, 3:6]
        self.n_valid = n_valid
        self.res = res = default_cells(n_valid) if cells is None else np.full(K, int(cells), np.int64)
        ext = hi - lo
        with np.errstate(all='ignore'):
            inv_h = np.where(ext > 0, res[:, None] / ext, 0.)
            h = np.where(ext > 0, ext / res[:, None], 0.)
        slack = 2. ** -30 * np.max(np.concatenate([ext, np.abs(lo), np.abs(hi)], 1), 1) if K else np.zeros(0)
        cbase = ragged.offsets(res ** 3)
        self.n_cells = int(cbase[-1])
        self.lo, self.hi = lo, hi
        self.frame = torch.from_numpy(np.stack([lo, hi, inv_h, h])).to(dev)          # (4,K,3): four (K,3) arrays
        self.slack = torch.from_numpy(np.ascontiguousarray(slack)).to(dev)
        self.res_dev = ragged.to_int32(res, dev)
        self.cbase_dev = ragged.to_int32(cbase, dev)
        # rule D3: count, prefix, fill
        self.offsets = torch.zeros(self.n_cells + 1, dtype=torch.int32, device=dev)
        self.cells = torch.zeros(0, dtype=torch.int32, device=dev)
        self.n_pairs = 0
        if F > 0:
            box = torch.empty(F, 8, dtype=torch.int32, device=dev)
            self._faces_pass(v, f, box)
            span = (box[:, 1:6:2] - box[:, 0:6:2] + 1).clamp(min=0).long()
            self.n_pairs = int(span.prod(1).sum())
            check_sizes(cell_triangle_pairs=self.n_pairs)
            count = torch.zeros(self.n_cells, dtype=torch.int32, device=dev)
            _lib.call("rfd_mdist_cells", dev, F, box.data_ptr(), self.n_cells, count.data_ptr(), None)
            self.offsets[1:] = torch.cumsum(count, 0)
            cursor = self.offsets[:-1].clone()
            self.cells = torch.empty(max(self.n_pairs, 1), dtype=torch.int32, device=dev)
            _lib.call("rfd_mdist_cells", dev, F, box.data_ptr(), self.n_cells, cursor.data_ptr(), self.cells.data_ptr())

    def _faces_pass(self, v, f, box):
        frame = (None, None, None, None) if box is None else \
            (self.frame[0].data_ptr(), self.frame[2].data_ptr(), self.res_dev.data_ptr(), self.cbase_dev.data_ptr())
        _lib.call("rfd_mdist_faces", self.device, self.F, self.K, self.V, v.data_ptr(), f.data_ptr(),
                  self.vend_dev.data_ptr(), self.tend_dev.data_ptr(), *frame, self.tri.data_ptr(), self.valid.data_ptr(),
                  self.fobj.data_ptr(), _lib.ptr(box))

    def cell_order(self, points, obj):
        """-> the permutation that orders the queries by (object, cell).  Only the launch's memory traffic depends on
        it, never a result, so the cells are computed here in plain torch."""
        K = self.K
        k = obj.long().clamp(0, K - 1)
        res = self.res_dev.long()[k]
        t = ((points - self.frame[0][k]) * self.frame[2][k]).nan_to_num(0., 0., 0.)
        c = torch.minimum(t.clamp(min=0).long(), (res - 1)[:, None])
        key = self.cbase_dev.long()[k] + (c[:, 0] * res + c[:, 1]) * res + c[:, 2]
        return torch.sort(key, stable=True)[1]

    @torch.no_grad()
    def query(self, points, obj=None, return_closest=False, sort_points=True):
        """points (n,3) f32 / f64 on the device, obj (n) integers: the object of every point (None: the batch's only
        object) -> d2 (n) f64: the squared distance to the closest valid face of the object, face (n) i32: its row in
        the batch's face array [, closest (n,3) f64: the point on it].  +inf, -1 for an object without valid faces;
        NaN, -1 for a point with a coordinate that is not finite (rule D5).  One read-back, to refuse an object outside
        the batch."""
        _lib.need_gpu(points)
        if points.dtype not in (torch.float32, torch.float64) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("query: points are (n,3) float32 or float64, got %s %s" % (points.dtype, tuple(points.shape)))
        n = int(points.shape[0])
        if obj is None:
            if self.K != 1:
                raise ValueError("query: a batch of %d objects needs `obj`" % self.K)
            obj = torch.zeros(n, dtype=torch.int32, device=points.device)
        else:
            _lib.need_gpu(obj)
            if obj.dtype.is_floating_point or tuple(obj.shape) != (n,):
                raise ValueError("query: obj is (%d,) integers, got %s %s" % (n, obj.dtype, tuple(obj.shape)))
            if n > 0:
                first, last = (int(x) for x in torch.stack([obj.amin(), obj.amax()]).cpu())
                if first < 0 or last >= self.K:
                    raise ValueError("query: objects in [%d, %d], but the batch has %d" % (first, last, self.K))
        return self._query(points, obj, return_closest, sort_points)

    def _query(self, points, obj, return_closest=False, sort_points=True):
        n, dev = int(points.shape[0]), self.device
        ragged.offsets([3 * n])
        d2 = torch.empty(n, dtype=torch.float64, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev)
        closest = torch.empty(n, 3, dtype=torch.float64, device=dev) if return_closest else None
        if n > 0:
            p, k = points.double().contiguous(), obj.to(torch.int32).contiguous()
            order = self.cell_order(p, k) if sort_points and self.K > 0 else None
            out = (d2, face, closest)
            if order is not None:
                p, k = p[order], k[order]
                out = [None if t is None else torch.empty_like(t) for t in out]
            fr = self.frame
            _lib.call("rfd_mdist_query", dev, n, p.data_ptr(), k.data_ptr(), self.K, self.F, fr[0].data_ptr(),
                      fr[1].data_ptr(), fr[2].data_ptr(), fr[3].data_ptr(), self.slack.data_ptr(), self.res_dev.data_ptr(),
                      self.cbase_dev.data_ptr(), self.offsets.data_ptr(), self.cells.data_ptr(), self.tri.data_ptr(),
                      out[0].data_ptr(), out[1].data_ptr(), _lib.ptr(out[2]))
            if order is not None:
                for dst, src in zip((d2, face, closest), out):
                    if dst is not None:
                        dst[order] = src
        return (d2, face, closest) if return_closest else (d2, face)

    def area_prefix(self):
        """-> cum (F) f64: every object's own inclusive prefix of its faces' areas (rule S1; 0 for a face that is not
        valid).  One cumsum over the batch, less what came before the object: the summation order is not part of the
        contract (rule D7), the sampler and whoever checks it read this array."""
        dev, F = self.device, self.F
        area = torch.zeros(F, dtype=torch.float64, device=dev)
        if F > 0:
            _lib.call("rfd_sample_face_areas", dev, F, self.tri.data_ptr(), area.data_ptr())
            area = torch.where(self.valid.bool(), area, torch.zeros_like(area))
        total = torch.cat([area.new_zeros(1), torch.cumsum(area, 0)])
        before = total[self.tend_dev.long()[:-1]]                                 # (K): the sum up to the object's first face
        return (total[1:] - before[self.fobj.long()]).clamp(min=0.) if F > 0 else area


def _as_distance(m, cells=None):
    return m if isinstance(m, MeshDistance) else MeshDistance(m, cells=cells)


def point_mesh_distance(vertices, faces, points, return_closest=False, cells=None):
    """one mesh, one call -> (d2 (n) f64, face (n) i32[, closest (n,3) f64]): MeshDistance(vertices, faces).query(points)"""
    _lib.need_gpu(vertices, faces, points)
    return MeshDistance(vertices, faces, cells=cells).query(points, return_closest=return_closest)


@torch.no_grad()
def sample_surface_ragged(scene_mesh, count, u=None, generator=None, return_normals=True):
    """scene_mesh: a SceneMesh or a MeshDistance of K objects -> points (K,count,3) f64, face (K,count) i32: rows of the
    batch's face array [, normals (K,count,3) f64]: `count` points uniform on the surface of every object (rule D7).
    u (K,count,3) f64 in [0,1) on the device is the randomness (mesh_sample.sample_surface's); None: torch.rand from
    `generator`.  An object without faces gives NaN points, face -1 and zero normals."""
    count = int(count)
    if count < 0:
        raise ValueError("sample_surface_ragged: count = %d" % count)
    md = _as_distance(scene_mesh)
    K, dev = md.K, md.device
    ragged.offsets([3 * K * count])
    if u is None:
        u = torch.rand(K, count, 3, dtype=torch.float64, device=dev, generator=generator)
    else:
        _lib.need_gpu(u)
        if u.dtype != torch.float64 or tuple(u.shape) != (K, count, 3):
            raise ValueError("sample_surface_ragged: u is (%d,%d,3) float64, got %s %s" % (K, count, u.dtype, tuple(u.shape)))
        u = u.contiguous()
    points = torch.empty(K, count, 3, dtype=torch.float64, device=dev)
    face = torch.empty(K, count, dtype=torch.int32, device=dev)
    normals = torch.empty_like(points) if return_normals else None
    cum = md.area_prefix()
    _lib.call("rfd_mdist_sample", dev, K, count, md.F, md.tri.data_ptr(), md.tend_dev.data_ptr(), cum.data_ptr(),
              u.data_ptr(), points.data_ptr(), face.data_ptr(), _lib.ptr(normals))
    return (points, face, normals) if return_normals else (points, face)


def segment_sums(md, seg, d2, face, normals=None, thresholds=()):
    """Rule D8 over the segments seg (S + 1) i32 on the device of queries against `md` -> sums (S,3) f64: sum d, sum d^2,
    sum |n_s . n_f|;  counts (S, 1 + T) i32: the entries left out (d not finite), then those with d <= tau_t."""
    tau = [float(t) for t in thresholds]
    if len(tau) > MAX_THRESHOLDS:
        raise ValueError("%d thresholds: at most %d" % (len(tau), MAX_THRESHOLDS))
    _lib.need_gpu(seg, d2, face)
    dev, S, n = md.device, int(seg.numel()) - 1, int(d2.numel())
    sums = torch.zeros(max(S, 0), 3, dtype=torch.float64, device=dev)
    counts = torch.zeros(max(S, 0), 1 + len(tau), dtype=torch.int32, device=dev)
    tau_dev = torch.tensor(tau, dtype=torch.float64, device=dev)
    if normals is not None:
        normals = normals.reshape(-1, 3).double().contiguous()
    _lib.call("rfd_mdist_sums", dev, S, n, md.F, seg.to(torch.int32).contiguous().data_ptr(), d2.contiguous().data_ptr(),
              face.contiguous().data_ptr(), _lib.ptr(normals), md.tri.data_ptr(), len(tau), tau_dev.data_ptr(),
              sums.data_ptr(), counts.data_ptr())
    return sums, counts


@torch.no_grad()
def mesh_metrics(A, B, pairs, count=10000, thresholds=(0.05, 0.10), u_a=None, u_b=None, generator=None):
    """A, B: two batches of meshes (SceneMesh or MeshDistance), A the predictions, B the ground truth; pairs (P,2): object
    a of A against object b of B.  Every object is sampled once (`count` points, rule D7; u_a (K_A,count,3) / u_b
    (K_B,count,3) f64 or torch.rand from `generator`), every sample of a pair asks the other mesh for its closest face.
    -> a dict of f64 tensors on the device, one row per pair:
      accuracy            (P)    mean distance of A's samples to B
      completeness        (P)    mean distance of B's samples to A
      chamfer_l1          (P)    (accuracy + completeness) / 2
      chamfer_sq          (P)    half the sum of the two mean squared distances
      precision           (P,T)  the share of A's samples within tau_t of B
      recall              (P,T)  the share of B's samples within tau_t of A: the point coverage ratio
      fscore              (P,T)  2 precision recall / (precision + recall), 0 where both are 0
      normal_consistency  (P)    the mean |n_s . n_f| of a sample's normal and its closest face's, averaged over both sides
      rms                 (P)    the two-sided RMS distance
    The thresholds (at most 8) are in the meshes' own units; the defaults are a choice.  A distance is exact (float64,
    closest point on the closest triangle), d <= tau counts as within.  A sample whose distance is not finite (the
    other object has no valid face; its own has no face) is left out of every mean; a mean over nothing is NaN.  The
    final divisions are torch float64 on the (P,) sums; the number of launches does not depend on P or K."""
    tau = [float(t) for t in thresholds]
    if len(tau) > MAX_THRESHOLDS:
        raise ValueError("%d thresholds: at most %d" % (len(tau), MAX_THRESHOLDS))
    A, B = _as_distance(A), _as_distance(B)
    dev = A.device
    pairs_host = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, np.int64).reshape(-1, 2)
    P = len(pairs_host)
    if P and (pairs_host.min() < 0 or pairs_host[:, 0].max() >= A.K or pairs_host[:, 1].max() >= B.K):
        raise ValueError("mesh_metrics: a pair names an object outside its batch (%d and %d objects)" % (A.K, B.K))
    count = int(count)
    ragged.offsets([3 * P * count])
    pa, pb = (torch.from_numpy(np.ascontiguousarray(pairs_host[:, c])).to(dev) for c in range(2))
    sa, _, na = sample_surface_ragged(A, count, u_a, generator)
    sb, _, nb = sample_surface_ragged(B, count, u_b, generator)
    seg = torch.arange(P + 1, dtype=torch.int32, device=dev) * count

    def one_way(points, normals, rows, target, target_rows):
        d2, face = target._query(points[rows].reshape(-1, 3), target_rows.repeat_interleave(count))
        sums, counts = segment_sums(target, seg, d2, face, normals[rows], tau)
        return sums, counts.double()
    s_ab, c_ab = one_way(sa, na, pa, B, pb)
    s_ba, c_ba = one_way(sb, nb, pb, A, pa)
    n_ab, n_ba = count - c_ab[:, 0], count - c_ba[:, 0]
    accuracy, completeness = s_ab[:, 0] / n_ab, s_ba[:, 0] / n_ba
    precision, recall = c_ab[:, 1:] / n_ab[:, None], c_ba[:, 1:] / n_ba[:, None]
    both = precision + recall
    return {
        'accuracy': accuracy, 'completeness': completeness, 'chamfer_l1': (accuracy + completeness) / 2,
        'chamfer_sq': (s_ab[:, 1] / n_ab + s_ba[:, 1] / n_ba) / 2,
        'precision': precision, 'recall': recall,
        'fscore': torch.where(both == 0, torch.zeros_like(both), 2 * precision * recall / both),
        'normal_consistency': (s_ab[:, 2] / n_ab + s_ba[:, 2] / n_ba) / 2,
        'rms': torch.sqrt((s_ab[:, 1] + s_ba[:, 1]) / (n_ab + n_ba)),
    }
