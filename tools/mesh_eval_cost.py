"""Cost of the mesh-IoU stage on one GPU -- a record, not a test.

    python tools/mesh_eval_cost.py [--out profiles/mesh_eval_cost.json] [--reps 20] [--warmup 3]

The two scenes of tools/render_cost.py (13 and 256 dented marching-cubes spheres of about 18 600 faces in the synthetic
scene's boxes) against 16 ground-truth objects of the same kind.  Per scene, for the three parts of
rfdnet_amd.iscnet.mesh_eval:
  voxelisation   method='per_object': object_grids of both sides (one object at a time through mesh_sample):
                 milliseconds between HIP events around the call -- the host waits inside it are part of the figure --
                 and the host synchronisations it makes, counted as read-backs of a device tensor through .cpu() /
                 .item() / int() / float() / bool() (implicit ones, e.g. of a boolean index, are not counted);
  pack           pack_grids of both sides (one rfd_objgrid_pack launch per object); voxelisation + pack is what
                 voxelize_objects(method='per_object') costs;
  voxelisation_batched   voxelize_objects(method='batched') of both sides (csrc/objgrid.hip): the same milliseconds,
                 the launches of mesh_eval's own kernels and the host synchronisations, counted the same way.  It is
                 timed in the same process as `voxelisation`, the two alternating call by call, and its words and
                 counts are compared with the per-object path's before anything is timed;
  counts         one rfd_mesh_iou_counts launch, and one rfd_mesh_iou_finalize launch.
Median, minimum and maximum of `reps` calls after `warmup` (the voxelisation: of 3 calls after 1), and beside them the
scene's reconstruction time from the benchmark records profiles/r06_bench_demo.json / r06_bench_headline.json."""
import argparse
import contextlib
import json
import os
import statistics
import types

import numpy as np
import torch

from cost_common import ROOT, emit, event_ms, need_gpu_or_exit, object_grids, placement_draws, timed

N_GT = 16


def placed(n_obj, seed, points=80000):
    """n_obj dented spheres in the synthetic scene's boxes (used again elsewhere as often as needed) -> SceneMesh"""
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet import box_util
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    from rfdnet_amd.iscnet.scene import place_in_corners
    _, boxes, _ = synthetic.synthetic_scene(seed=100, n_raw=int(points * 1.5), n_points=points, return_boxes=True)
    rng = np.random.default_rng(seed)
    again = np.arange(n_obj) >= len(boxes)
    boxes = boxes[np.arange(n_obj) % len(boxes)].astype(np.float64)
    offset, noise = placement_draws(rng, n_obj)
    centre = boxes[:, :3] + again[:, None] * offset * (1., 1., 0.)
    corners = box_util.box_corners_upright_camera(torch.from_numpy(centre), torch.from_numpy(boxes[:, 3:6]),
                                                  torch.from_numpy(boxes[:, 6] + noise)).cuda()
    meshes = [types.SimpleNamespace(vertices=v, faces=f) for v, f in marching_cubes_batch(object_grids(rng, n_obj), 0.)]
    return place_in_corners(meshes, corners, torch.zeros(n_obj, dtype=torch.int32))


@contextlib.contextmanager
def counted_readbacks(counter):
    names = ('cpu', 'item', 'tolist', '__int__', '__float__', '__bool__', '__index__')
    saved = {n: getattr(torch.Tensor, n) for n in names}
    depth = [0]

    def wrap(fn):
        def counted(self, *a, **k):
            if self.is_cuda and depth[0] == 0:
                counter[0] += 1
            depth[0] += 1                          # int() goes through item(): one read-back, counted once
            try:
                return fn(self, *a, **k)
            finally:
                depth[0] -= 1
        return counted
    for n in names:
        setattr(torch.Tensor, n, wrap(saved[n]))
    try:
        yield
    finally:
        for n in names:
            setattr(torch.Tensor, n, saved[n])


@contextlib.contextmanager
def counted_launches(log):
    """every launch the host modules make goes through _lib.call: its names, in order"""
    from rfdnet_amd import _lib
    call = _lib.call

    def counting(name, *a):
        log.append(name)
        return call(name, *a)
    _lib.call = counting
    try:
        yield
    finally:
        _lib.call = call


def alternating(fns, reps, warmup):
    """timed() for several callables in one loop, one call of each per round -> [the dict of each]"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for out, fn in zip(ms, fns):
            out.append(event_ms(fn))
    return [{"ms": statistics.median(m), "ms_min": min(m), "ms_max": max(m)} for m in ms]


def same_grids(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("frame", "dim", "off", "cnt", "words"))


def measure(label, n_obj, record, reps, warmup):
    from rfdnet_amd.iscnet import mesh_eval
    pred, gt = placed(n_obj, 5), placed(N_GT, 6)
    voxelise = lambda: (mesh_eval.object_grids(pred), mesh_eval.object_grids(gt))
    batched = lambda: (mesh_eval.voxelize_objects(pred, method='batched'), mesh_eval.voxelize_objects(gt, method='batched'))
    syncs = [0]
    with counted_readbacks(syncs):
        ep, eg = voxelise()
    pack = lambda: (mesh_eval.pack_grids(ep, "cuda"), mesh_eval.pack_grids(eg, "cuda"))
    pg, gg = pack()
    syncs_b, launches_b = [0], []
    with counted_readbacks(syncs_b), counted_launches(launches_b):
        bp, bg = batched()
    equal = same_grids(bp, pg) and same_grids(bg, gg)
    t_per_object, t_batched = alternating([voxelise, batched], 3, 1)
    counts = mesh_eval.mesh_iou_counts(pg, gg)
    iou = torch.zeros(n_obj, N_GT, dtype=torch.float64, device="cuda")
    mesh_eval.scatter_iou(pg, gg, counts, iou)
    overlap = int((counts.sum(-1) > 0).sum())
    row = {"scene": label, "objects": n_obj, "ground_truths": N_GT, "faces": int(pred.faces.shape[0] + gt.faces.shape[0]),
           "grid_dims": {"min": int(min(pg.dims.min(), gg.dims.min())), "max": int(max(pg.dims.max(), gg.dims.max()))},
           "grid_words": pg.n_words + gg.n_words, "pairs": n_obj * N_GT, "pairs_with_a_hit": overlap,
           "iou_max": float(iou.max()),
           "voxelisation": dict(t_per_object, method="per_object", host_synchronisations=syncs[0],
                                host_synchronisations_per_object=syncs[0] / float(n_obj + N_GT)),
           "voxelisation_batched": dict(t_batched, method="batched", launches=len(launches_b),
                                        host_synchronisations=syncs_b[0], equals_per_object=bool(equal)),
           "pack": dict(timed(pack, reps, warmup), launches=int((pg.dims > 0).sum() + (gg.dims > 0).sum()),
                        host_synchronisations=0),
           "counts": dict(timed(lambda: mesh_eval.mesh_iou_counts(pg, gg), reps, warmup), launches=1,
                          host_synchronisations=0),
           "finalize": dict(timed(lambda: mesh_eval.scatter_iou(pg, gg, counts, iou), reps, warmup), launches=1,
                            host_synchronisations=0)}
    row["counts_over_voxelisation"] = row["counts"]["ms"] / row["voxelisation"]["ms"]
    # the condition: a sign with a margin for noise, no ratio fixed in advance
    row["batched_max_below_per_object_min"] = bool(t_batched["ms_max"] < t_per_object["ms_min"])
    with open(os.path.join(ROOT, "profiles", record)) as f:
        bench = json.load(f)
    row["reconstruction"] = {"record": "profiles/" + record, "ms_per_step": bench["ms_per_step"], "metric": bench["metric"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    need_gpu_or_exit("mesh_eval_cost")
    rows = [measure("demo-sized", 13, "r06_bench_demo.json", args.reps, args.warmup),
            measure("headline", 256, "r06_bench_headline.json", args.reps, args.warmup)]
    emit({"tool": "mesh_eval_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
          "voxel_size": 0.047, "rows": rows}, args.out)


if __name__ == "__main__":
    main()
