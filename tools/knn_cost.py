"""Cost of the k-nearest-neighbour search on one GPU -- a record, not a test.

    python tools/knn_cost.py [--out profiles/knn_cost.json] [--reps 20] [--warmup 3] [--points 100000] [--queries 100000]

`--points` uniform data points in [0,1)^3 and `--queries` queries in [-0.1, 1.1)^3, float64, default_rng(0).  Timed apart,
between HIP events, the median, minimum and maximum of `reps` calls after `warmup`, in one process: the build of PointSets
(valid points, frames, cell lists) and PointSets.query for k = 1, 8 and 32, each with the launches of the library's own
kernels (the torch sorts and prefix sums between them are not counted) and the host read-backs of one call (Tensor.cpu is
wrapped for one run).  Beside them: the same k = 1 search through chamfer_distance.nearest (float32, brute force, and it
answers both directions in its one call), and on the host scipy.spatial.cKDTree (build, and query(workers=16) for the
three k, wall-clock milliseconds, the median of `--host_reps` runs).  The k = 1 indices of the three are compared and the
number of queries on which they differ is recorded: float32 may order near-ties differently."""
import argparse
import statistics
import time

import numpy as np
import torch

from cost_common import emit, need_gpu_or_exit, timed

KS = (1, 8, 32)


def counted(fn):
    """one run of fn -> (its result, launches of the library's kernels, Tensor.cpu calls)"""
    from rfdnet_amd import _lib
    names, copies = [], []
    call, cpu = _lib.call, torch.Tensor.cpu

    def counting_call(name, *args):
        names.append(name)
        return call(name, *args)

    def counting_cpu(self, *args, **kw):
        copies.append(1)
        return cpu(self, *args, **kw)
    _lib.call, torch.Tensor.cpu = counting_call, counting_cpu
    try:
        out = fn()
    finally:
        _lib.call, torch.Tensor.cpu = call, cpu
    return out, len(names), len(copies)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return {"ms": statistics.median(out), "ms_min": min(out), "ms_max": max(out), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=100000)
    args = ap.parse_args()
    need_gpu_or_exit("knn_cost")
    from scipy.spatial import cKDTree
    from rfdnet_amd.chamfer_distance import nearest
    from rfdnet_amd.knn import PointSets
    rng = np.random.default_rng(0)
    data = rng.uniform(0., 1., (args.points, 3))
    queries = rng.uniform(-0.1, 1.1, (args.queries, 3))
    d, q = torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda()

    sets, launches, read_backs = counted(lambda: PointSets(d))
    result = {"tool": "knn_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "data_points": args.points, "queries": args.queries, "cells_per_axis": int(sets.res[0]),
              "build": dict(timed(lambda: PointSets(d), args.reps, args.warmup), launches=launches,
                            host_read_backs=read_backs)}
    for k in KS:
        _, launches, read_backs = counted(lambda: sets.query(q, k=k))
        result["query_k%d" % k] = dict(timed(lambda: sets.query(q, k=k), args.reps, args.warmup), launches=launches,
                                       host_read_backs=read_backs)
    result["query_k1_unsorted"] = timed(lambda: sets.query(q, k=1, sort_points=False), args.reps, args.warmup)
    d32, q32 = d.float()[None], q.float()[None]
    result["chamfer_nearest_k1_float32_both_directions"] = timed(lambda: nearest(q32, d32), args.reps, args.warmup)
    tree = cKDTree(data)
    result["ckdtree_build_host"] = wall_ms(lambda: cKDTree(data), args.host_reps)
    for k in KS:
        result["ckdtree_query_k%d_host_workers16" % k] = wall_ms(lambda: tree.query(queries, k=k, workers=16),
                                                                 args.host_reps)
    ours = sets.query(q, k=1)[1][:, 0].cpu().numpy()
    result["k1_indices_differing_from_ckdtree"] = int((ours != tree.query(queries, k=1, workers=16)[1]).sum())
    result["k1_indices_of_chamfer_nearest_differing"] = int((nearest(q32, d32)[1][0].cpu().numpy() != ours).sum())
    emit(result, args.out)


if __name__ == "__main__":
    main()
