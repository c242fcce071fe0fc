"""tools/prepare_scan.py's output -> the scan_labels.npz that `demo.py --mode test --gt` reads: one sample of the
reference's dataloader (models/iscnet/dataloader.py), made on the GPU by rfdnet_amd.scan_labels.make_sample.

    python tools/make_scan_labels.py --scan processed/scene0000_00/full_scan.npz --bbox processed/scene0000_00/bbox.pkl \
        --mean_size_npz scannet_means.npz --out scan_labels.npz [--num_point 80000] [--seed 10] [--mode test]
        [--use_color] [--no_height] [--shapenet_path datasets/ShapeNetv2_data --points_subsample 2048]

The file holds point_clouds, center_label, heading_*_label, size_*_label, sem_cls_label, box_label_mask, vote_label,
vote_label_mask, point_instance_labels, object_instance_labels, scan_idx and, with --shapenet_path (the directory
tools/sample_mesh.py fills: point/<catid>/<id>.npz and voxel/16/<catid>/<id>.binvox), object_points, object_points_occ,
object_voxels and in test mode object_points_iou, object_points_iou_occ.  The random draws come from
numpy.random.RandomState(seed) in the dataloader's order."""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", required=True)
    ap.add_argument("--bbox", required=True)
    ap.add_argument("--mean_size_npz", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--num_point", type=int, default=80000)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--mode", choices=["test", "train"], default="test")
    ap.add_argument("--use_color", action="store_true")
    ap.add_argument("--no_height", action="store_true")
    ap.add_argument("--shapenet_path", default=None)
    ap.add_argument("--points_subsample", type=int, default=2048)
    args = ap.parse_args(argv)
    import torch
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.scan_labels import make_sample
    if not torch.cuda.is_available():
        raise SystemExit("make_scan_labels runs on a GPU: none is visible")
    cfg = Config({'data': {'num_point': args.num_point, 'use_color_detection': args.use_color,
                           'no_height': args.no_height, 'points_subsample': args.points_subsample}},
                 mean_size_arr=args.mean_size_npz)
    with open(args.bbox, "rb") as f:
        boxes = pickle.load(f)
    sample = make_sample(dict(np.load(args.scan)), boxes, cfg, args.mode, rng=np.random.RandomState(args.seed),
                         shapenet_path=args.shapenet_path, instance_labels=True)
    arrays = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in sample.items()
              if k not in ('shapenet_catids', 'shapenet_ids')}
    np.savez(args.out, **arrays)
    print("%s: %d points, %d boxes, %d points with a vote" % (args.out, len(arrays['point_clouds']), len(boxes),
                                                              int(arrays['vote_label_mask'].sum())))
    return args.out


if __name__ == "__main__":
    main()
