"""Exact k nearest neighbours among points on the device, for one point set or a ragged batch of them, and what is built
on it: a stand-in for pykdtree's KDTree, the two helpers of the reference's external/common.py, and the surface metrics of
point clouds (the ground truth of tools/sample_mesh.py is a pointcloud.npz, not a mesh).

  PointSets                            built once per batch (valid points, frames, cell lists), queried any number of times
  KDTree                               pykdtree.kdtree.KDTree's interface: numpy in, numpy out
  get_nearest_neighbors_indices_batch  external/common.py's, one ragged build and one query for the whole batch
  chamfer_distance_kdtree              external/common.py's, its torch arithmetic after the search evaluated on the device
  pointcloud_metrics                   mesh_distance.mesh_metrics' dictionary for point sets with normals

The kernels are csrc/knn.hip, the rules N1 - N7 are written out in include/rfd_knn.h and restated in numpy float64 in
tests/knn_f64.py.  The answer of a query is the k least keys (squared distance, local row) over the valid points of its
set that are not masked and lie within the bound: a total order, so the cells, the batch and the order of the queries only
decide the cost.  A point with a coordinate that is not finite takes no part (rule N1): nothing is refused for its data.
Everything is queued on the current stream; the number of launches and read-backs depends on neither the number of sets
nor the number of pairs.

Deviation from pykdtree, which computes float32 trees in float32: float32 inputs are upcast (exactly) and compared in
float64, and the reported distance is float32(sqrt_f64(d2)), or float32(d2) with sqr_dists.  pykdtree's float32 arithmetic
could order near-ties differently."""
import numpy as np
import torch

from . import _lib, mesh_batch, ragged
from .mesh_distance import MAX_CELLS, MAX_THRESHOLDS, _extents, default_cells

MAX_K = 32


def _offsets(offsets, N):
    """None, a host sequence or a tensor of K + 1 ascending offsets -> (pend int64 (K + 1), K)"""
    if offsets is None:
        return np.array([0, N], np.int64), 1
    if torch.is_tensor(offsets):
        offsets = offsets.cpu().numpy()
    pend = mesh_batch._ascending(offsets, "offsets")
    if pend[-1] != N:
        raise ValueError("the offsets end at %d points, the batch has %d" % (pend[-1], N))
    return pend, len(pend) - 1


class PointSets(object):
    """PointSets(points (N,3) f32 / f64 on the device[, offsets (K + 1): set k owns the rows offsets[k] .. offsets[k+1]-1]
    [, cells]): the valid points (rule N1), the frames (N2) and the cell lists (N3) of a ragged batch, built once.
    cells: 1 .. 64 cells per axis for every set, None: default_cells of every set's valid points.  At most two
    read-backs, whatever K: the offsets if they are a device tensor, and the frames."""

    @torch.no_grad()
    def __init__(self, points, offsets=None, cells=None):
        if cells is not None and not 1 <= int(cells) <= MAX_CELLS:
            raise ValueError("cells = %s: 1 .. %d" % (cells, MAX_CELLS))
        _lib.need_gpu(points)
        if points.dtype not in (torch.float64, torch.float32):
            raise TypeError("points must be float64 or float32, not %s" % points.dtype)
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points are (N,3), got %s" % (tuple(points.shape),))
        self.device = dev = points.device
        self.N = N = int(points.shape[0])
        ragged.offsets([3 * N])
        self.pend, self.K = pend, K = _offsets(offsets, N)
        self.pend_dev = ragged.to_int32(pend, dev)
        self.points = p = points.double().contiguous()
        self.valid = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.pobj = torch.zeros(N, dtype=torch.int32, device=dev)
        self._points_pass(None)
        # rule N2 on the host, from one read-back: the extents and the number of the valid points of every set
        lo, hi, n_valid = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K, np.int64)
        if N > 0:
            owner, keep = self.pobj.long(), self.valid.bool()
            elo, ehi = _extents(p[keep], owner[keep], K)
            count = torch.zeros(K, dtype=torch.float64, device=dev).index_add_(0, owner, self.valid.double())
            host = torch.cat([elo, ehi, count[:, None]], 1).cpu().numpy()
            n_valid = host[:, 6].astype(np.int64)
            some = n_valid > 0
            lo[some], hi[some] = host[some, 0:3], host[some, 3:6]
        self.n_valid = n_valid
        self.M = M = int(n_valid.sum())
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
        # rule N3: count, prefix, fill (with the coordinates in list order)
        self.offsets = torch.zeros(self.n_cells + 1, dtype=torch.int32, device=dev)
        self.list = torch.zeros(max(M, 1), dtype=torch.int32, device=dev)
        self.sorted = torch.zeros(max(M, 1), 3, dtype=torch.float64, device=dev)
        if N > 0:
            cell = torch.empty(N, dtype=torch.int32, device=dev)
            self._points_pass(cell)
            count = torch.zeros(self.n_cells, dtype=torch.int32, device=dev)
            _lib.call("rfd_knn_cells", dev, N, cell.data_ptr(), self.n_cells, count.data_ptr(), None, M, None, None)
            self.offsets[1:] = torch.cumsum(count, 0)
            cursor = self.offsets[:-1].clone()
            _lib.call("rfd_knn_cells", dev, N, cell.data_ptr(), self.n_cells, cursor.data_ptr(), self.list.data_ptr(), M,
                      p.data_ptr(), self.sorted.data_ptr())

    def _points_pass(self, cell):
        frame = (None, None, None, None) if cell is None else \
            (self.frame[0].data_ptr(), self.frame[2].data_ptr(), self.res_dev.data_ptr(), self.cbase_dev.data_ptr())
        _lib.call("rfd_knn_points", self.device, self.N, self.K, self.points.data_ptr(), self.pend_dev.data_ptr(), *frame,
                  self.valid.data_ptr(), self.pobj.data_ptr(), _lib.ptr(cell))

    def cell_order(self, points, obj):
        """-> the permutation that orders the queries by (object, cell), as MeshDistance.cell_order.  Only the launch's
        memory traffic depends on it, never a result, so the cells are computed here in plain torch."""
        K = self.K
        k = obj.long().clamp(0, K - 1)
        res = self.res_dev.long()[k]
        t = ((points - self.frame[0][k]) * self.frame[2][k]).nan_to_num(0., 0., 0.)
        c = torch.minimum(t.clamp(min=0).long(), (res - 1)[:, None])
        key = self.cbase_dev.long()[k] + (c[:, 0] * res + c[:, 1]) * res + c[:, 2]
        return torch.sort(key, stable=True)[1]

    @torch.no_grad()
    def query(self, points, obj=None, k=1, distance_upper_bound=None, mask=None, sort_points=True):
        """points (n,3) f32 / f64 on the device, obj (n) integers: the set of every point (None: the batch's only set)
        -> d2 (n,k) f64: the squared distances to the k nearest valid points of the set, ascending, idx (n,k) i32: their
        rows LOCAL to the set.  A neighbour that does not exist (fewer than k candidates) is +inf, -1; a point with a
        coordinate that is not finite gives NaN, -1 (rule N5).  distance_upper_bound: only points CLOSER than it count
        (strict, as in pykdtree); mask (N) bool / u8 on the device: a non-zero value excludes that row of the batch for
        this call.  One read-back, to refuse an object outside the batch."""
        _lib.need_gpu(points)
        if points.dtype not in (torch.float32, torch.float64) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("query: points are (n,3) float32 or float64, got %s %s" % (points.dtype, tuple(points.shape)))
        n = int(points.shape[0])
        if obj is None:
            if self.K != 1:
                raise ValueError("query: a batch of %d sets needs `obj`" % self.K)
            obj = torch.zeros(n, dtype=torch.int32, device=points.device)
        else:
            _lib.need_gpu(obj)
            if obj.dtype.is_floating_point or tuple(obj.shape) != (n,):
                raise ValueError("query: obj is (%d,) integers, got %s %s" % (n, obj.dtype, tuple(obj.shape)))
            if n > 0:
                first, last = (int(x) for x in torch.stack([obj.amin(), obj.amax()]).cpu())
                if first < 0 or last >= self.K:
                    raise ValueError("query: objects in [%d, %d], but the batch has %d" % (first, last, self.K))
        return self._query(points, obj, k, distance_upper_bound, mask, sort_points)

    def _query(self, points, obj, k=1, distance_upper_bound=None, mask=None, sort_points=True, sorted_copy=True):
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("query: k = %d: 1 .. %d" % (k, MAX_K))
        limit2 = np.inf
        if distance_upper_bound is not None:
            bound = float(distance_upper_bound)
            if not bound >= 0:
                raise ValueError("query: distance_upper_bound must be non negative")
            limit2 = bound * bound
        if mask is not None:
            _lib.need_gpu(mask)
            if mask.numel() != self.N or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("query: mask is (%d,) bool or uint8, got %s %s" % (self.N, mask.dtype, tuple(mask.shape)))
            mask = mask.reshape(-1).to(torch.uint8).contiguous()
        n, dev = int(points.shape[0]), self.device
        ragged.offsets([3 * n])
        ragged.offsets([n * k])
        d2 = torch.empty(n, k, dtype=torch.float64, device=dev)
        idx = torch.empty(n, k, dtype=torch.int32, device=dev)
        if n > 0:
            p, o = points.double().contiguous(), obj.to(torch.int32).contiguous()
            order = self.cell_order(p, o) if sort_points and self.K > 0 else None
            out = (d2, idx)
            if order is not None:
                p, o = p[order], o[order]
                out = [torch.empty_like(t) for t in out]
            fr = self.frame
            _lib.call("rfd_knn_query", dev, n, p.data_ptr(), o.data_ptr(), k, limit2, _lib.ptr(mask), self.K, self.N,
                      self.points.data_ptr(), self.pend_dev.data_ptr(), fr[0].data_ptr(), fr[1].data_ptr(),
                      fr[2].data_ptr(), fr[3].data_ptr(), self.slack.data_ptr(), self.res_dev.data_ptr(),
                      self.cbase_dev.data_ptr(), self.offsets.data_ptr(), self.list.data_ptr(), self.M,
                      self.sorted.data_ptr() if sorted_copy else None, out[0].data_ptr(), out[1].data_ptr())
            if order is not None:
                d2[order], idx[order] = out[0], out[1]
        return d2, idx


def _as_sets(s, cells=None):
    return s if isinstance(s, PointSets) else PointSets(s, cells=cells)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("CPU not supported")
    return torch.device("cuda", torch.cuda.current_device())


def _device_search(data, queries, k, limit2_bound, mask):
    """KDTree's one device call (tests stub it): data (n,3) f64, queries (m,3) f64 numpy, bound a distance or None, mask
    (n) u8 or None -> d2 (m,k) f64, idx (m,k) i64 with -1 for missing, as numpy"""
    dev = _device()
    sets = PointSets(torch.from_numpy(data).to(dev))
    m = None if mask is None else torch.from_numpy(mask).to(dev)
    d2, idx = sets.query(torch.from_numpy(queries).to(dev), k=k, distance_upper_bound=limit2_bound, mask=m)
    return d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _pad3(a, ndim):
    """(n,ndim) -> (n,3) f64, the missing columns zero: they add exact zeros to d2"""
    out = np.zeros((a.shape[0], 3), np.float64)
    out[:, :ndim] = a.reshape(a.shape[0], ndim)
    return out


class KDTree(object):
    """KDTree(data_pts (n,) or (n,ndim) numpy, leafsize=16) with pykdtree.kdtree.KDTree's query(): the exact k nearest
    neighbours, searched on the device (one PointSets per query call).  ndim is 1 .. 3; eps is honoured by returning the
    exact answer, which satisfies every eps >= 0; leafsize is validated and ignored.  See the module's note on float32."""

    def __init__(self, data_pts, leafsize=16):
        if leafsize < 1:
            raise ValueError('leafsize must be greater than zero')
        data_pts = np.asarray(data_pts)
        if data_pts.ndim not in (1, 2):
            raise ValueError('data points are (n,) or (n, ndim)')
        ndim = 1 if data_pts.ndim == 1 else int(data_pts.shape[1])
        if not 1 <= ndim <= 3:
            raise ValueError('%d dimensions: this KDTree serves 1 to 3 dimensions' % ndim)
        dtype = np.float32 if data_pts.dtype == np.float32 else np.float64
        self.data_pts = np.ascontiguousarray(data_pts.ravel(), dtype=dtype)
        self.data = self.data_pts                                      # scipy interface compatibility, as pykdtree
        self.n, self.ndim, self.leafsize = int(data_pts.shape[0]), ndim, int(leafsize)

    def query(self, query_pts, k=1, eps=0, distance_upper_bound=None, sqr_dists=False, mask=None):
        """-> (distances, indices): (m,) for k = 1, (m,k) otherwise; indices uint32 with n for a missing neighbour,
        distances inf there; the square root unless sqr_dists; float32 iff data and queries are both float32."""
        if k < 1:
            raise ValueError('Number of neighbours must be greater than zero')
        elif eps < 0:
            raise ValueError('eps must be non-negative')
        elif distance_upper_bound is not None and distance_upper_bound < 0:
            raise ValueError('distance_upper_bound must be non negative')
        query_pts = np.asarray(query_pts)
        if query_pts.ndim not in (1, 2):
            raise ValueError('query points are (m,) or (m, ndim)')
        q_ndim = 1 if query_pts.ndim == 1 else query_pts.shape[1]
        if self.ndim != q_ndim:
            raise ValueError('Data and query points must have same dimensions')
        if self.data_pts.dtype == np.float32 and query_pts.dtype != np.float32:
            raise TypeError('Type mismatch. query points must be of type float32 when data points are of type float32')
        if mask is not None:
            mask = np.asarray(mask)
            if mask.size != self.n:
                raise ValueError('Mask must have the same size as data points')
            mask = np.ascontiguousarray(mask.ravel() != 0, dtype=np.uint8)
        k = int(k)
        if k > MAX_K:
            raise ValueError('k = %d: this KDTree serves 1 to %d neighbours' % (k, MAX_K))
        single = query_pts.dtype == np.float32 and self.data_pts.dtype == np.float32
        m = int(query_pts.shape[0])
        d2, idx = _device_search(_pad3(self.data_pts.reshape(self.n, self.ndim), self.ndim),
                                 _pad3(np.ascontiguousarray(query_pts), self.ndim), k, distance_upper_bound, mask)
        missing = idx < 0
        dist = np.where(missing, np.inf, d2)
        if not sqr_dists:
            dist = np.sqrt(dist)
        dist = dist.astype(np.float32 if single else np.float64)
        index = np.where(missing, self.n, idx).astype(np.uint32)
        if k == 1:
            return dist.reshape(m), index.reshape(m)
        return dist, index


def _batch_search(points_src, points_tgt, k):
    """(B,n,3) queries against (B,m,3) sets, tensors on the device -> d2 (B,n,k) f64, idx (B,n,k) i32: one ragged build
    and one query for the whole batch"""
    B, n, m = int(points_src.shape[0]), int(points_src.shape[1]), int(points_tgt.shape[1])
    sets = PointSets(points_tgt.reshape(-1, 3), np.arange(B + 1, dtype=np.int64) * m)
    obj = torch.arange(B, dtype=torch.int32, device=points_src.device).repeat_interleave(n)
    d2, idx = sets._query(points_src.reshape(-1, 3), obj, k)
    return d2.view(B, n, k), idx.view(B, n, k)


def _on_device(a):
    a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if a.dim() != 3 or a.shape[2] != 3 or a.dtype not in (torch.float32, torch.float64):
        raise ValueError("point batches are (B,n,3) float32 or float64, got %s %s" % (a.dtype, tuple(a.shape)))
    return a if a.is_cuda else a.to(_device())


def get_nearest_neighbors_indices_batch(points_src, points_tgt, k=1):
    """external/common.py's: for each pair of the two batches (B,n,3), (B,m,3) (numpy or tensors) the k nearest points of
    points_tgt[b] for every point of points_src[b] -> (indices, distances): two lists of B numpy arrays with pykdtree's
    shapes and types ((n,) for k = 1, else (n,k); uint32 with m for missing; distances, not squared)."""
    src, tgt = _on_device(points_src), _on_device(points_tgt)
    if src.shape[0] != tgt.shape[0]:
        raise ValueError("batches of %d and %d sets" % (src.shape[0], tgt.shape[0]))
    single = src.dtype == torch.float32 and tgt.dtype == torch.float32
    m = int(tgt.shape[1])
    d2, idx = _batch_search(src, tgt, k)
    dist = torch.sqrt(torch.where(idx < 0, torch.full_like(d2, np.inf), d2))
    dist = (dist.float() if single else dist).cpu().numpy()
    index = torch.where(idx < 0, torch.full_like(idx, m), idx).cpu().numpy().astype(np.uint32)
    if k == 1:
        dist, index = dist[:, :, 0], index[:, :, 0]
    return [i for i in index], [d for d in dist]


def chamfer_distance_kdtree(points1, points2, give_id=False):
    """external/common.py's: points1, points2 (B,T,3) tensors -> chamfer (B), or with give_id (chamfer1 (B), chamfer2 (B),
    idx_nn_12 (B,T) int64, idx_nn_21 (B,T) int64).  The search is one ragged build and one query per direction; what
    follows it is the reference's own torch expression, evaluated on the device in the inputs' dtype."""
    p1, p2 = _on_device(points1), _on_device(points2)
    batch_size = p1.size(0)
    idx_nn_12 = _batch_search(p1, p2, 1)[1][:, :, 0].long()
    idx_nn_21 = _batch_search(p2, p1, 1)[1][:, :, 0].long()
    points_12 = torch.gather(p2, dim=1, index=idx_nn_12.view(batch_size, -1, 1).expand_as(p1))
    points_21 = torch.gather(p1, dim=1, index=idx_nn_21.view(batch_size, -1, 1).expand_as(p2))
    chamfer1 = (p1 - points_12).pow(2).sum(2).mean(1)
    chamfer2 = (p2 - points_21).pow(2).sum(2).mean(1)
    if give_id:
        return chamfer1, chamfer2, idx_nn_12, idx_nn_21
    return chamfer1 + chamfer2


def segment_sums(sets, seg, d2, idx, obj, normals_src=None, normals_tgt=None, thresholds=()):
    """Rule N7 over the segments seg (S + 1) i32 on the device of query results d2, idx (n,k) against `sets` for the
    objects obj (n) -> sums (S,3) f64: sum d, sum d^2, sum |n_s . n_t| of the nearest neighbours (slot 0);  counts
    (S, 1 + T) i32: the entries left out (no neighbour, d not finite), then those with d <= tau_t.  normals_src (n,3),
    normals_tgt (N,3): either None and the third sum is 0."""
    tau = [float(t) for t in thresholds]
    if len(tau) > MAX_THRESHOLDS:
        raise ValueError("%d thresholds: at most %d" % (len(tau), MAX_THRESHOLDS))
    _lib.need_gpu(seg, d2, idx, obj)
    dev, S, n = sets.device, int(seg.numel()) - 1, int(obj.numel())
    stride = int(d2.shape[1]) if d2.dim() == 2 else 1
    if d2.numel() != n * stride or idx.numel() != n * stride:
        raise ValueError("segment_sums: d2 and idx are (%d,k), got %s and %s" % (n, tuple(d2.shape), tuple(idx.shape)))
    sums = torch.zeros(max(S, 0), 3, dtype=torch.float64, device=dev)
    counts = torch.zeros(max(S, 0), 1 + len(tau), dtype=torch.int32, device=dev)
    tau_dev = torch.tensor(tau, dtype=torch.float64, device=dev)
    if normals_src is not None:
        normals_src = normals_src.reshape(-1, 3).double().contiguous()
        if normals_src.shape[0] != n:
            raise ValueError("segment_sums: %d source normals for %d entries" % (normals_src.shape[0], n))
    if normals_tgt is not None:
        normals_tgt = normals_tgt.reshape(-1, 3).double().contiguous()
        if normals_tgt.shape[0] != sets.N:
            raise ValueError("segment_sums: %d target normals for %d points" % (normals_tgt.shape[0], sets.N))
    _lib.call("rfd_knn_sums", dev, S, n, stride, seg.to(torch.int32).contiguous().data_ptr(),
              d2.double().contiguous().data_ptr(), idx.to(torch.int32).contiguous().data_ptr(),
              obj.to(torch.int32).contiguous().data_ptr(), sets.K, sets.N, sets.pend_dev.data_ptr(),
              _lib.ptr(normals_src), _lib.ptr(normals_tgt), len(tau), tau_dev.data_ptr(), sums.data_ptr(),
              counts.data_ptr())
    return sums, counts


@torch.no_grad()
def pointcloud_metrics(A, B, pairs, normals_a=None, normals_b=None, thresholds=(0.05, 0.10)):
    """A, B: two batches of point sets (PointSets, or (N,3) tensors for one set each), A the predictions, B the ground
    truth; pairs (P,2): set a of A against set b of B; normals_a (N_A,3), normals_b (N_B,3): the points' normals, or
    None.  Every point of a pair's one set asks the other set for its nearest point.  -> mesh_distance.mesh_metrics'
    dictionary of f64 tensors on the device, one row per pair, with the same keys (accuracy, completeness, chamfer_l1,
    chamfer_sq, precision, recall, fscore, normal_consistency, rms) and the same left-out rule: a point without a
    neighbour (the other set has no valid point) or with a distance that is not finite is left out of every mean; a mean
    over nothing is NaN.  normal_consistency is 0 without both normals.  The final divisions are torch float64 on the
    (P,) sums; the number of launches does not depend on P or K."""
    tau = [float(t) for t in thresholds]
    if len(tau) > MAX_THRESHOLDS:
        raise ValueError("%d thresholds: at most %d" % (len(tau), MAX_THRESHOLDS))
    A, B = _as_sets(A), _as_sets(B)
    dev = A.device
    pairs_host = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, np.int64).reshape(-1, 2)
    P = len(pairs_host)
    if P and (pairs_host.min() < 0 or pairs_host[:, 0].max() >= A.K or pairs_host[:, 1].max() >= B.K):
        raise ValueError("pointcloud_metrics: a pair names a set outside its batch (%d and %d sets)" % (A.K, B.K))
    for sets, normals, name in ((A, normals_a, "normals_a"), (B, normals_b, "normals_b")):
        if normals is not None:
            _lib.need_gpu(normals)
            if normals.numel() != 3 * sets.N:
                raise ValueError("pointcloud_metrics: %s is (%d,3)" % (name, sets.N))
    if (normals_a is None) != (normals_b is None):
        normals_a = normals_b = None

    def one_way(src, src_sets, src_normals, tgt, tgt_sets, tgt_normals):
        # the rows of every pair's source set, pair after pair: all on the host, from the offsets
        counts = src.pend[src_sets + 1] - src.pend[src_sets]
        seg = ragged.offsets(counts)
        n = int(seg[-1])
        ragged.offsets([3 * n])
        owner = ragged.owners(counts)
        rows = torch.from_numpy(src.pend[src_sets][owner] + (np.arange(n) - seg[owner])).to(dev)
        obj = torch.from_numpy(np.ascontiguousarray(tgt_sets[owner])).to(dev)
        d2, idx = tgt._query(src.points[rows], obj, 1)
        ns = None if src_normals is None else src_normals.reshape(-1, 3)[rows]
        sums, left = segment_sums(tgt, ragged.to_int32(seg, dev), d2, idx, obj, ns, tgt_normals, tau)
        return sums, left.double(), torch.from_numpy(counts.astype(np.float64)).to(dev)
    s_ab, c_ab, m_ab = one_way(A, pairs_host[:, 0], normals_a, B, pairs_host[:, 1], normals_b)
    s_ba, c_ba, m_ba = one_way(B, pairs_host[:, 1], normals_b, A, pairs_host[:, 0], normals_a)
    n_ab, n_ba = m_ab - c_ab[:, 0], m_ba - c_ba[:, 0]
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
