"""Cost of the scan ground truth on one GPU -- a record, not a test.

    python tools/scan_labels_cost.py [--out profiles/scan_labels_cost.json] [--reps 20] [--warmup 3]
                                     [--vertices 150000] [--models 30] [--instances 40]

A synthetic scan (vertices uniform in a 8 x 8 x 3 m room, instance ids in runs, as a scan stores them) and `models` CAD
vertex sets of 2 000 to 20 000 vertices.  Per stage of rfdnet_amd.scan_labels, device milliseconds between HIP events
(median, minimum, maximum of `reps` calls after `warmup`; uploads and read-backs of the call included), the library's
kernel launches and the host synchronisations of one call, and beside them the wall time of the numpy restatement
tests/scan_labels_f64.py of the same stage on the same machine's CPU (one run; the matching on a subset, scaled).
The stages are memory-light -- the scan is 3.6 MB, the votes 12 MB -- so the numbers say what a scan costs, not how close
a kernel is to a roof."""
import argparse
import os
import sys
import time

import numpy as np
import torch

from cost_common import ROOT, emit, need_gpu_or_exit, timed

sys.path.insert(0, os.path.join(ROOT, "tests"))

# the library's launches and the host synchronisations (read-backs) of one call, by construction of scan_labels.py
LAUNCHES = {"instance_boxes": (3, 1), "cad_extents": (3, 1), "match_instances": (1, 2), "point_votes": (1, 0),
            "make_sample_test": (1, 1), "make_sample_train": (1, 1)}


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=150000)
    ap.add_argument("--models", type=int, default=30)
    ap.add_argument("--instances", type=int, default=40)
    args = ap.parse_args()
    need_gpu_or_exit("scan_labels_cost")
    import scan_labels_f64 as ref
    from rfdnet_amd import scan_labels as sl
    from rfdnet_amd.iscnet.config import Config
    rng = np.random.RandomState(3)
    N, M, I = args.vertices, args.models, args.instances
    vertices = np.concatenate([rng.uniform((-4, -4, 0), (4, 4, 3), (N, 3)), rng.randint(0, 256, (N, 3))], 1).astype(np.float32)
    ids = np.sort(rng.randint(0, I + 1, N)).astype(np.int64)
    sets = [rng.randn(int(n), 3) * 0.3 for n in rng.randint(2000, 20001, M)]
    L = rng.randn(M, 3, 3)
    boxes = np.hstack([rng.uniform((-3.5, -3.5, 0.3), (3.5, 3.5, 1.5), (M, 3)), rng.uniform(0.4, 1.6, (M, 3)),
                       rng.uniform(-np.pi, np.pi, (M, 1))])
    d_v, d_ids = torch.from_numpy(vertices).cuda(), torch.from_numpy(ids).cuda()
    inst = sl.instance_boxes(d_v, d_ids, I)
    votes, hits = sl.point_votes(d_v, boxes)
    scan = {'mesh_vertices': d_v, 'point_votes': votes, 'instance_labels': d_ids}
    box_list = [{'box3D': b, 'cls_id': 7, 'instance_id': 0} for b in boxes]
    cfg = Config({'data': {'num_point': 80000, 'use_color_detection': True}}, mean_size_arr=np.ones((8, 3)))
    choices = rng.choice(N, 80000, replace=N < 80000)
    stages = {
        "instance_boxes": lambda: sl.instance_boxes(d_v, d_ids, I),
        "cad_extents": lambda: sl.cad_extents(sets, L, 'cuda'),
        "match_instances": lambda: sl.match_instances(boxes, inst),
        "point_votes": lambda: sl.point_votes(d_v, boxes),
        "make_sample_test": lambda: sl.make_sample(scan, box_list, cfg, 'test', choices=choices),
        "make_sample_train": lambda: sl.make_sample(scan, box_list, cfg, 'train', choices=choices, flips=(True, False),
                                                    rot_angle=0.3),
    }
    h_votes = votes.cpu().numpy()
    sub = min(M, 4)
    numpy_ms = {
        "instance_boxes": wall(lambda: ref.instance_boxes(vertices, ids, I)),
        "cad_extents": wall(lambda: [ref.extents_rule(v, l) for v, l in zip(sets, L)]),
        "match_instances": wall(lambda: ref.match(boxes[:sub], inst)) * M / sub,
        "point_votes": wall(lambda: ref.point_votes(vertices, boxes)),
        "make_sample_test": wall(lambda: ref.sample(vertices, h_votes, ids, boxes, [7] * M, [0] * M, np.ones((8, 3)),
                                                    choices, False, use_color=True)),
        "make_sample_train": wall(lambda: ref.sample(vertices, h_votes, ids, boxes, [7] * M, [0] * M, np.ones((8, 3)),
                                                     choices, True, (True, False), 0.3, use_color=True)),
    }
    rows = {}
    for name, fn in stages.items():
        rows[name] = dict(timed(fn, args.reps, args.warmup), library_launches=LAUNCHES[name][0],
                          host_synchronisations=LAUNCHES[name][1], numpy_restatement_ms=numpy_ms[name])
    result = {"tool": "scan_labels_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "warmup": args.warmup, "vertices": N, "models": M, "instances": I,
              "cad_vertices": int(sum(len(s) for s in sets)), "points_in_a_box": int((hits > 0).sum()),
              "deepest_overlap": int(hits.max()), "num_point": 80000, "stages": rows}
    emit(result, args.out)


if __name__ == "__main__":
    main()
