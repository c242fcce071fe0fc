"""How far is one surface from another: the exact surface metrics of two mesh files on the device.

    python tools/mesh_distance.py A.off B.off [--samples 10000] [--thresholds 0.05 0.10] [--seed 0]

Reads .off / .obj / .ply through the shared mesh reader, draws `--samples` points on each mesh and asks the other mesh
for the exact closest triangle of every one (rfdnet_amd.mesh_distance.mesh_metrics: A is the prediction, B the truth).
Prints one JSON line: accuracy, completeness, chamfer_l1, chamfer_sq, rms, normal_consistency, and precision, recall
(the point coverage ratio) and fscore per threshold.  The thresholds are in the files' own units."""
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
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.05, 0.10])
    ap.add_argument("--seed", type=int, default=0)
    return ap


def report(metrics, thresholds):
    """mesh_metrics' dict for one pair -> plain numbers (None for a NaN)"""
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
        raise SystemExit("mesh_distance runs on a GPU: none is visible")
    from rfdnet_amd import io
    from rfdnet_amd.mesh_distance import MAX_THRESHOLDS, MeshDistance, mesh_metrics
    if len(args.thresholds) > MAX_THRESHOLDS:
        raise SystemExit("at most %d thresholds" % MAX_THRESHOLDS)
    dev = torch.device("cuda")
    sides = []
    for path in (args.a, args.b):
        v, f = io.read_mesh(path)
        if not len(v) or not len(f):
            raise SystemExit("%s holds no triangles" % path)
        sides.append(MeshDistance(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)))
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    m = mesh_metrics(sides[0], sides[1], [[0, 0]], args.samples, args.thresholds, generator=gen)
    out = {"tool": "mesh_distance", "a": args.a, "b": args.b, "samples": args.samples,
           "faces": [s.F for s in sides], "valid_faces": [int(s.n_valid.sum()) for s in sides]}
    out.update(report(m, args.thresholds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
