"""How far is a predicted surface from a ground-truth point cloud: the surface metrics of a mesh file against the
pointcloud.npz that tools/sample_mesh.py writes, on the device.

    python tools/pointcloud_distance.py pred.off gt/pointcloud.npz [--samples 10000] [--thresholds 0.05 0.10] [--seed 0]
                                        [--original_frame]

Reads the mesh (.off / .obj / .ply) through the shared mesh reader, draws `--samples` points with their normals on it
(rfdnet_amd.mesh_distance.sample_surface_ragged) and scores them against the file's points and normals by exact nearest
neighbours in both directions (rfdnet_amd.knn.pointcloud_metrics: the mesh is the prediction, the file the truth).  The
file's points are taken as stored, in the unit cube of sample_mesh.py; --original_frame moves them back by the file's loc
and scale first.  Prints one JSON line: accuracy, completeness, chamfer_l1, chamfer_sq, rms, normal_consistency, and
precision, recall and fscore per threshold.  The thresholds are in the points' own units."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("pointcloud")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.05, 0.10])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--original_frame", action="store_true")
    return ap


def report(metrics, thresholds):
    """pointcloud_metrics' dict for one pair -> plain numbers (None for a NaN)"""
    num = lambda x: None if x != x else float(x)
    out = {k: num(float(v[0])) for k, v in metrics.items() if v.dim() == 1}
    for k in ('precision', 'recall', 'fscore'):
        out[k] = {"%g" % t: num(float(x)) for t, x in zip(thresholds, metrics[k][0])}
    return out


def main():
    args = build_parser().parse_args()
    if args.samples < 1:
        raise SystemExit("--samples must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("pointcloud_distance runs on a GPU: none is visible")
    from rfdnet_amd import io
    from rfdnet_amd.knn import PointSets, pointcloud_metrics
    from rfdnet_amd.mesh_distance import MAX_THRESHOLDS, MeshDistance, sample_surface_ragged
    if len(args.thresholds) > MAX_THRESHOLDS:
        raise SystemExit("at most %d thresholds" % MAX_THRESHOLDS)
    dev = torch.device("cuda")
    v, f = io.read_mesh(args.mesh)
    if not len(v) or not len(f):
        raise SystemExit("%s holds no triangles" % args.mesh)
    points, normals, loc, scale = io.read_pointcloud_npz(args.pointcloud, original_frame=args.original_frame)
    if not len(points):
        raise SystemExit("%s holds no points" % args.pointcloud)
    mesh = MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    samples, _, sample_normals = sample_surface_ragged(mesh, args.samples, generator=gen)
    truth = PointSets(torch.from_numpy(points).to(dev))
    m = pointcloud_metrics(PointSets(samples[0]), truth, [[0, 0]], sample_normals[0],
                           torch.from_numpy(normals).to(dev), args.thresholds)
    out = {"tool": "pointcloud_distance", "mesh": args.mesh, "pointcloud": args.pointcloud, "samples": args.samples,
           "points": int(truth.N), "valid_points": int(truth.n_valid.sum()), "loc": [float(x) for x in loc], "scale": scale}
    out.update(report(m, args.thresholds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
