"""fit_mesh_to_scan: refine the centre and heading of every detected box so that its generated
mesh lies on the scan points inside the (enlarged) box -- 100 Adam steps on a one-sided Chamfer
loss (models/iscnet/modules/network.py:182-303).  Everything stays on the device.

One set-up, two optimisers.  prepare_fit selects the proposals, cuts the scan at the 5th height percentile, tests the
points against the box at 1.2x its size, and normalises and scales the meshes, for all objects at once, into one ragged
FitProblem; finish_fit writes the best parameters back as corners.  Between them:
  method='autograd'   run_fit_autograd: padded_problem pads the ragged rows to the reference's 10 000 / 50 000 and Adam
                      runs on chamfer_loss, whose searches and gradients are the kernels of csrc/chamfer.hip
                      (rfdnet_amd.chamfer_distance); the gradient is summed with fp32 atomics;
  method='device'     run_fit: the same optimisation without the padding, without autograd and without a host round
                      trip inside the loop (csrc/fit_pose.hip, include/rfd_fit.h).

Reference quirks reproduced on purpose:
  * mesh points and scan points are zero-padded to 10 000 / 50 000 rows and the PADDED mesh
    rows take part in the search (they sit at the box centre after the transform); only the
    scan side is masked in the loss (`mean(dist2 * mask) * 1e3` over all objects at once);
  * the parameters kept are those of the iteration with the lowest loss BEFORE its update;
  * scan points below the 5th height percentile are dropped, a box needs >= 5 points.
Differences: meshes with more than 10 000 vertices are subsampled with a fixed stride (the
reference would fail on the copy), the in-box test is an exact oriented-box test instead of a
Delaunay hull query (identical except for points exactly on a face).

The ragged problem keeps the same quirks, restated:
  * the padded scan rows are masked in the loss, so they are simply left out; the mean's denominator stays the padded
    count (loss_scale = 1e3 / (P * 50 000));
  * the padded mesh rows are all the zero row, which the transform puts on the box centre; they follow the real rows, so
    with the search's strict '<' in index order only the FIRST of them can ever be the nearest neighbour.  One extra zero
    row after the real rows of a mesh with fewer than 10 000 of them therefore stands for all of them (a mesh with 10 000
    rows has no padding and gets none; padded_problem leaves that row out and pads with zeros again);
  * the nearest neighbour is piecewise constant in the parameters, so the gradient autograd builds is four sums over an
    object's scan points (rfd_fit.h), summed in f64 in a fixed order instead of with fp32 atomics: two runs are
    bitwise equal.

The two methods share their set-up, so their agreement says nothing about it.  What checks the set-up is independent of
prepare_fit: the per-object loop `per_object_setup` of tests/test_fit_device_cpu.py, built from the single-object forms
points_in_box and normalise_mesh_points below and compared with prepare_fit (and padded_problem) bit for bit, and the
fixture F_FIT, which is the reference's own function's run.  Keep that loop a loop: calling prepare_fit from it would
compare the batched code with itself.
"""
import numpy as np
import torch

from ..chamfer_distance import ChamferDistanceFunction
from .. import _lib, ragged
from .box_util import box_params_from_corners, flip_axis_to_camera, flip_axis_to_depth, get_3d_box  # noqa: F401

MAX_OBJ_POINTS = 10000          # network.py:194
MAX_PC_IN_BOX = 50000           # network.py:195
TRANSFORM_SHAPENET = ((0., 0., -1.), (-1., 0., 0.), (0., 1., 0.))      # network.py:191


def points_in_box(points, corners):
    """points (N,3), corners (8,3) of a box in get_3d_box order -> bool mask (N)."""
    o = corners[2]
    axes = torch.stack([corners[1] - corners[2], corners[3] - corners[2], corners[6] - corners[2]])   # (3,3)
    t = (points - o) @ axes.t()                      # projections scaled by the edge lengths
    l2 = (axes * axes).sum(1)
    return ((t >= 0) & (t <= l2)).all(dim=1)


def normalise_mesh_points(vertices):
    """network.py:207-211: centre at the bounding-box centre, permute to the ShapeNet frame,
    scale every axis to unit extent."""
    v = vertices.double()
    v = v - (v.max(0)[0] + v.min(0)[0]) / 2.
    v = v @ torch.tensor(TRANSFORM_SHAPENET, dtype=torch.float64, device=v.device).t()
    return v / (v.max(0)[0] - v.min(0)[0])


def chamfer_loss(obj_points, pc_in_box, pc_in_box_masks, centroid_params, orientation_params):
    """network.py:293-303."""
    b_s = obj_points.size(0)
    axis_rectified = torch.zeros(b_s, 3, 3, device=obj_points.device)
    axis_rectified[:, 2, 2] = 1
    axis_rectified[:, 0, 0] = torch.cos(orientation_params)
    axis_rectified[:, 0, 1] = torch.sin(orientation_params)
    axis_rectified[:, 1, 0] = -torch.sin(orientation_params)
    axis_rectified[:, 1, 1] = torch.cos(orientation_params)
    obj_points_after = torch.bmm(obj_points, axis_rectified) + centroid_params.unsqueeze(-2)
    _, dist2 = ChamferDistanceFunction.apply(obj_points_after, pc_in_box)
    return torch.mean(dist2 * pc_in_box_masks) * 1e3


METHODS = ('autograd', 'device')
RUN_WIDTH = 256                 # csrc/fit_pose.hip's WG: a run (tile) is RUN_WIDTH * points_per_thread scan rows of one object
PPT_SWITCH = 65536              # scan points of all objects together: up to here fit_nn_kernel takes one point per thread


def fit_method(fit):
    """evaluate()'s `fit` argument -> None (no refinement) or a name of METHODS; True is 'autograd'"""
    if fit is None or fit is False:
        return None
    if fit is True:
        return 'autograd'
    if fit not in METHODS:
        raise ValueError("fit method %r: one of %s" % (fit, ", ".join(METHODS)))
    return fit


def points_in_boxes(points, corners):
    """points (N,3), corners (K,8,3) -> bool mask (K,N): points_in_box's operations on K boxes at once."""
    o = corners[:, 2]
    axes = torch.stack([corners[:, 1] - corners[:, 2], corners[:, 3] - corners[:, 2], corners[:, 6] - corners[:, 2]], 1)
    t = (points[None] - o[:, None]) @ axes.transpose(1, 2)
    l2 = (axes * axes).sum(2)
    return ((t >= 0) & (t <= l2[:, None])).all(dim=2)


def normalise_mesh_points_ragged(vertices, seg, n_obj):
    """normalise_mesh_points on the concatenated rows of n_obj meshes; seg (V) int64: the mesh of every row."""
    v = vertices.double()
    idx = seg[:, None].expand(-1, 3)

    def extent(x):
        hi = torch.full((n_obj, 3), -np.inf, dtype=x.dtype, device=x.device).scatter_reduce(0, idx, x, 'amax')
        lo = torch.full((n_obj, 3), np.inf, dtype=x.dtype, device=x.device).scatter_reduce(0, idx, x, 'amin')
        return hi, lo
    hi, lo = extent(v)
    v = v - ((hi + lo) / 2.)[seg]
    v = v @ torch.tensor(TRANSFORM_SHAPENET, dtype=torch.float64, device=v.device).t()
    hi, lo = extent(v)
    return v / (hi - lo)[seg]


class FitProblem(object):
    """The ragged problem of rfd_fit_pose_run (include/rfd_fit.h; DESIGN.md "Ragged batches") and what finish_fit needs
    beside it: obj (n_obj,3) f32, obj_off (P+1) i32, scan (n_scan,3) f32, scan_off (P+1) i32, tile_obj / tile_start (n_tiles) i32,
    scan_index (n_scan) i64: the row of its scene's input scan that every row of `scan` is,
    params0 (P,4) f32, sizes (P,3) f64, corners (B,K,8,3) f64: the boxes as they came in, index_list: the (scene,
    proposal) of every object, n_vertices / n_scan_points: per object, on the host, points_per_thread, loss_scale;
    result: the last run_fit's.  P = 0: nothing to fit, only `corners` and `index_list` are there."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def prepare_fit(meshes, proposal_ids, parsed_predictions, eval_dict, input_scan, dump_threshold, points_per_thread=None):
    """The set-up of fit_mesh_to_scan (same arguments, same selection rules) as one ragged FitProblem on input_scan's device
    (CPU tensors work too).  Per scene: one batched in-box test of the selected proposals, one nonzero; the vertices of
    all objects are normalised in one concatenation.  The host waits a fixed number of times per scene, whatever the
    number of proposals.  points_per_thread: 1 or 4 to force fit_nn_kernel's instantiation (default: by PPT_SWITCH)."""
    dev = input_scan.device
    corners_all = _lib.as_tensor(parsed_predictions['pred_corners_3d_upright_camera'], dev, torch.float64).clone()
    obj_prob = _lib.as_tensor(parsed_predictions['obj_prob'], dev, torch.float64)
    pred_mask = _lib.as_tensor(eval_dict['pred_mask'], dev, torch.int64)
    ids = _lib.as_tensor(proposal_ids, dev, torch.int64)
    bsize = obj_prob.shape[0]
    scan = input_scan.double()
    sel = ((pred_mask == 1) & (obj_prob > dump_threshold)).cpu().numpy()
    id_rows = ids[:, :, 0].cpu().tolist()

    index_list, n_scan_points, vert_list, scan_parts, row_parts, box_parts = [], [], [], [], [], []
    for i in range(bsize):
        js = np.nonzero(sel[i])[0]
        if len(js) == 0:
            continue
        height = torch.quantile(scan[i, :, 2], 0.05)                         # np.percentile(., 5)
        above = torch.nonzero(scan[i, :, 2] >= height)[:, 0]
        scene_scan = scan[i, above, :3]
        centroid, sizes, orientation = box_params_from_corners(corners_all[i, torch.as_tensor(js, device=dev)])
        larger = flip_axis_to_depth(get_3d_box(1.2 * sizes, -orientation, flip_axis_to_camera(centroid)))
        inside = points_in_boxes(scene_scan, larger)
        n_in = inside.sum(1).tolist()
        keep = [k for k, n in enumerate(n_in) if n >= 5]
        if not keep:
            continue
        kt = torch.as_tensor(keep, device=dev)
        row, col = torch.nonzero(inside[kt], as_tuple=True)                  # row-major: every object's points in scan order
        if max(n_in[k] for k in keep) > MAX_PC_IN_BOX:
            first = ragged.offsets([n_in[k] for k in keep])[:-1]
            rank = torch.arange(row.shape[0], device=dev) - torch.as_tensor(first, device=dev)[row]
            col = col[rank < MAX_PC_IN_BOX]
        scan_parts.append(scene_scan[col])
        row_parts.append(above[col])
        box_parts.append((centroid[kt], sizes[kt], orientation[kt]))
        for k in keep:
            index_list.append((i, int(js[k])))
            n_scan_points.append(min(n_in[k], MAX_PC_IN_BOX))
            vert_list.append(meshes[id_rows[i].index(int(js[k]))].vertices)
    if not index_list:
        return FitProblem(P=0, corners=corners_all, index_list=[], device=dev, result=None)

    P = len(index_list)
    n_vertices = []
    for k, verts in enumerate(vert_list):
        verts = verts if torch.is_tensor(verts) else torch.as_tensor(np.asarray(verts))
        if verts.shape[0] > MAX_OBJ_POINTS:
            stride = -(-verts.shape[0] // MAX_OBJ_POINTS)
            verts = verts[::stride]
        vert_list[k] = verts.to(dev, torch.float64)
        n_vertices.append(int(verts.shape[0]))
    centroid, sizes, orientation = (torch.cat([b[c] for b in box_parts]) for c in range(3))
    seg_host = ragged.owners(n_vertices)
    seg = torch.from_numpy(seg_host).to(dev)
    scaled = normalise_mesh_points_ragged(torch.cat(vert_list), seg, P) * sizes[seg]
    # one zero row after every mesh that the reference would pad: it stands for all its padded rows (module docstring)
    extra = np.asarray([v < MAX_OBJ_POINTS for v in n_vertices], np.int64)
    obj_off = ragged.offsets(np.asarray(n_vertices) + extra)
    scan_off = ragged.offsets(n_scan_points)
    obj = torch.zeros(int(obj_off[-1]), 3, dtype=torch.float32, device=dev)
    dest = np.arange(len(seg_host)) + ragged.offsets(extra)[seg_host]
    obj[torch.from_numpy(dest).to(dev)] = scaled.float()
    return ragged_problem(obj, obj_off, torch.cat(scan_parts).float().contiguous(), scan_off,
                          torch.cat([centroid.float(), orientation.float()[:, None]], 1).contiguous(),
                          1e3 / (P * MAX_PC_IN_BOX), points_per_thread, corners=corners_all, index_list=index_list,
                          n_vertices=n_vertices, sizes=sizes, scan_index=torch.cat(row_parts))


def ragged_problem(obj, obj_off, scan, scan_off, params0, loss_scale, points_per_thread=None, **more):
    """obj (n_obj,3), scan (n_scan,3), params0 (P,4): f32 tensors on the problem's device; obj_off, scan_off (P+1): host
    integer arrays -> FitProblem with the runs (tile_obj / tile_start, DESIGN.md "Ragged batches") of points_per_thread
    (default: 1 up to PPT_SWITCH scan points, else 4)"""
    dev = obj.device
    n_scan_points = [int(n) for n in np.diff(scan_off)]
    if points_per_thread is None:
        points_per_thread = 1 if scan_off[-1] <= PPT_SWITCH else 4
    tile_obj, tile_start = ragged.runs(n_scan_points, RUN_WIDTH * points_per_thread)
    return FitProblem(P=len(n_scan_points), device=dev, obj=obj, obj_off=ragged.to_int32(obj_off, dev), scan=scan,
                      scan_off=ragged.to_int32(scan_off, dev), n_scan_points=n_scan_points,
                      tile_obj=ragged.to_int32(tile_obj, dev), tile_start=ragged.to_int32(tile_start, dev),
                      points_per_thread=points_per_thread, params0=params0, loss_scale=loss_scale, result=None, **more)


def run_fit(problem, lr=0.01, iterations=100, history=False):
    """Enqueue the whole optimisation on the current stream (rfd_fit_pose_run: two launches per iteration) without waiting
    for anything.  -> problem.result = {'params', 'best_params' (P,4), 'best_loss' (1) f32, 'best_iter' (1) i32} and with
    history 'hist_loss' (iterations), 'hist_params' (iterations,P,4): the state before every update."""
    if problem.P == 0:
        return None
    dev, P, T = problem.device, problem.P, int(iterations)
    if dev.type != 'cuda':
        raise ValueError("run_fit needs the problem on the GPU (prepare_fit was given CPU tensors)")
    n_tiles = problem.tile_obj.shape[0]
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    res = {'params': problem.params0.clone(), 'best_params': f32(P, 4), 'best_loss': f32(1),
           'best_iter': torch.empty(1, dtype=torch.int32, device=dev)}
    if history:
        res['hist_loss'], res['hist_params'] = f32(T), f32(T, P, 4)
    work = torch.empty(_lib.lib().rfd_fit_pose_workspace_bytes(P, n_tiles) // 8, dtype=torch.float64, device=dev)
    _lib.call("rfd_fit_pose_run", dev, P, problem.obj.shape[0], problem.scan.shape[0], n_tiles,
              problem.points_per_thread, T, float(lr), float(problem.loss_scale), problem.obj.data_ptr(),
              problem.obj_off.data_ptr(), problem.scan.data_ptr(), problem.scan_off.data_ptr(),
              problem.tile_obj.data_ptr(), problem.tile_start.data_ptr(), res['params'].data_ptr(),
              res['best_params'].data_ptr(), res['best_loss'].data_ptr(), res['best_iter'].data_ptr(),
              _lib.ptr(res.get('hist_loss')), _lib.ptr(res.get('hist_params')), work.data_ptr())
    res['workspace'] = work                                      # lives until the result is dropped
    problem.result = res
    return res


def finish_fit(problem, parsed_predictions):
    """-> parsed_predictions with the refined 'pred_corners_3d_upright_camera', 'fit_loss' and 'fit_indices' (and
    'fit_history' = {'loss', 'params', 'best_iter'} if run_fit recorded one), as fit_mesh_to_scan returns them."""
    out = dict(parsed_predictions)
    corners_all = problem.corners.clone()
    if problem.P == 0:
        out['pred_corners_3d_upright_camera'] = corners_all
        return out
    res = problem.result
    best = res['best_params'].double()
    new_corners = get_3d_box(problem.sizes, -best[:, 3], flip_axis_to_camera(best[:, :3]))
    where = torch.as_tensor(problem.index_list, device=problem.device)
    corners_all[where[:, 0], where[:, 1]] = new_corners
    out['pred_corners_3d_upright_camera'] = corners_all
    out['fit_loss'] = float(res['best_loss'])
    out['fit_indices'] = list(problem.index_list)
    if 'hist_loss' in res:
        out['fit_history'] = {'loss': res['hist_loss'], 'params': res['hist_params'], 'best_iter': int(res['best_iter'])}
    return out


def padded_problem(problem):
    """The ragged problem in the reference's shapes (network.py:194-195, :246-269) -> obj_points (P,10000,3),
    pc_in_box (P,50000,3), pc_masks (P,50000): 1 on the real scan rows, centroid_params (P,3), orientation_params (P),
    all f32.  Only an object's real mesh rows are copied: the stand-in zero row is left to the padding."""
    P, dev = problem.P, problem.device
    obj_off, scan_off = problem.obj_off.tolist(), problem.scan_off.tolist()
    obj_points = torch.zeros(P, MAX_OBJ_POINTS, 3, dtype=torch.float32, device=dev)
    pc_in_box = torch.zeros(P, MAX_PC_IN_BOX, 3, dtype=torch.float32, device=dev)
    pc_masks = torch.zeros(P, MAX_PC_IN_BOX, dtype=torch.float32, device=dev)
    for p in range(P):
        V, S = problem.n_vertices[p], problem.n_scan_points[p]
        obj_points[p, :V] = problem.obj[obj_off[p]:obj_off[p] + V]
        pc_in_box[p, :S] = problem.scan[scan_off[p]:scan_off[p] + S]
        pc_masks[p, :S] = 1
    fresh = dict(memory_format=torch.contiguous_format)          # tensors of their own: the optimiser updates in place
    return obj_points, pc_in_box, pc_masks, problem.params0[:, :3].clone(**fresh), problem.params0[:, 3].clone(**fresh)


def run_fit_autograd(problem, lr=0.01, iterations=100):
    """The reference's loop (network.py:271-291) on the padded problem: Adam on chamfer_loss, whose gradient autograd
    builds from the Chamfer kernels (fp32 atomics: not run-to-run deterministic).  -> problem.result = {'best_params'
    (P,4) f32, 'best_loss'}: the state BEFORE the update of the iteration with the lowest loss."""
    if problem.P == 0:
        return None
    obj_points, pc_in_box, pc_masks, centroid_params, orientation_params = padded_problem(problem)
    centroid_params.requires_grad_(True)
    orientation_params.requires_grad_(True)
    optimizer = torch.optim.Adam([centroid_params, orientation_params], lr=lr)
    res = {'best_params': problem.params0.clone(), 'best_loss': 1e6}
    with torch.enable_grad():
        for _ in range(iterations):
            optimizer.zero_grad()
            loss = chamfer_loss(obj_points, pc_in_box, pc_masks, centroid_params, orientation_params)
            cur = float(loss.detach())
            if cur < res['best_loss']:
                res['best_params'] = torch.cat([centroid_params.detach(), orientation_params.detach()[:, None]], 1)
                res['best_loss'] = cur
            loss.backward()
            optimizer.step()
    problem.result = res
    return res


def fit_mesh_to_scan(meshes, proposal_ids, parsed_predictions, eval_dict, input_scan, dump_threshold,
                     lr=0.01, iterations=100, method='autograd', history=False):
    """meshes: list of objects with `.vertices` (V,3) for proposal_ids (B,K',1) in order;
    parsed_predictions / eval_dict as returned by predictions.parse_predictions (device tensors or
    numpy); input_scan (B,N,3+) -> parsed_predictions with refined
    'pred_corners_3d_upright_camera' (a copy; the input is not modified).
    method: 'autograd' (the reference's padded loop on the Chamfer kernels) or 'device' (module docstring);
    history (method='device' only): also return 'fit_history'."""
    if method not in METHODS:
        raise ValueError("fit method %r: one of %s" % (method, ", ".join(METHODS)))
    problem = prepare_fit(meshes, proposal_ids, parsed_predictions, eval_dict, input_scan, dump_threshold)
    if method == 'device':
        run_fit(problem, lr=lr, iterations=iterations, history=history)
    else:
        run_fit_autograd(problem, lr=lr, iterations=iterations)
    return finish_fit(problem, parsed_predictions)
