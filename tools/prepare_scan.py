"""One scan with aligned CAD models -> its ground truth, as the reference's ScanNet preparation stores it
(utils/scannet/gen_scannet_w_orientation.py), computed on the GPU by rfdnet_amd.scan_labels.prepare_scan.

    python tools/prepare_scan.py --scan scene0000_00_vh_clean_2.ply --instance_ids ids.npy \
        --annotation full_annotations.json --id_scan scene0000_00 --meta scene0000_00.txt \
        --shapenet ShapeNetCore.v2 --out_dir processed/scene0000_00

  --scan           a .ply (x y z and, if present, red green blue per vertex) or an .npz with `vertices` (N,3) or (N,6)
  --instance_ids   .npy (N,) integers, 0 = background, or an .npz with `instance_ids`; reading them out of ScanNet's
                   segment and aggregation JSON files is not part of this project
  --annotation     JSON in Scan2CAD's layout: one entry {id_scan, trs, aligned_models: [{catid_cad, id_cad, trs}]} or a
                   list of them (--id_scan picks one)
  --meta           the scan's .txt with the `axisAlignment = ...` line (absent: the identity)
  --shapenet       the root under which <catid_cad>/<id_cad>/models/model_normalized.obj lie
Writes out_dir/full_scan.npz (mesh_vertices, point_votes, instance_labels), out_dir/bbox.pkl and out_dir/mean_sizes.npz
(cls_id, size: one row per box, for the class means over all scans: rfdnet_amd.scan_labels.mean_size_array).  When no
model is inside the class filter nothing is written, as in the reference."""
import argparse
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_axis_alignment(path):
    if path:
        with open(path) as f:
            for line in f:
                if 'axisAlignment' in line:
                    return np.array([float(x) for x in line.split('=')[1].split()]).reshape(4, 4)
    return np.eye(4)


def read_vertices(path):
    from rfdnet_amd import io
    if path.endswith(".npz"):
        v = np.asarray(np.load(path)['vertices'], np.float32)
        return v if v.shape[1] >= 6 else np.concatenate([v[:, :3], np.zeros((len(v), 3), np.float32)], 1)
    return io.read_scan_ply(path)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", required=True)
    ap.add_argument("--instance_ids", required=True)
    ap.add_argument("--annotation", required=True)
    ap.add_argument("--id_scan", default=None)
    ap.add_argument("--meta", default=None)
    ap.add_argument("--shapenet", required=True)
    ap.add_argument("--out_dir", required=True)
    args = ap.parse_args(argv)
    import torch
    from rfdnet_amd import io, scan_labels
    if not torch.cuda.is_available():
        raise SystemExit("prepare_scan runs on a GPU: none is visible")
    with open(args.annotation) as f:
        annotation = json.load(f)
    if isinstance(annotation, list):
        annotation = [a for a in annotation if args.id_scan is None or a['id_scan'] == args.id_scan][0]
    ids = np.load(args.instance_ids)
    ids = np.asarray(ids['instance_ids'] if isinstance(ids, np.lib.npyio.NpzFile) else ids).astype(np.int64)
    vertices = read_vertices(args.scan)
    if ids.shape != (len(vertices),):
        raise SystemExit("%d vertices, instance ids %s" % (len(vertices), ids.shape))
    models = []
    for m in annotation['aligned_models']:
        m = dict(m)
        if scan_labels.class_of(m['catid_cad']) is not None:          # only what the filter keeps is read
            m['vertices'] = io.read_obj(os.path.join(args.shapenet, m['catid_cad'], m['id_cad'], 'models',
                                                     'model_normalized.obj'))[0]
        models.append(m)
    out = scan_labels.prepare_scan(torch.from_numpy(vertices).cuda(), torch.from_numpy(ids).cuda(), models,
                                   annotation['trs'], read_axis_alignment(args.meta), aligned=False)
    if out is None:
        print("%s: no model inside the class filter, nothing written" % annotation.get('id_scan', args.scan))
        return None
    boxes, scan, mean_sizes = out
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez(os.path.join(args.out_dir, "full_scan.npz"), **scan)
    with open(os.path.join(args.out_dir, "bbox.pkl"), "wb") as f:
        pickle.dump(boxes, f, protocol=pickle.HIGHEST_PROTOCOL)
    np.savez(os.path.join(args.out_dir, "mean_sizes.npz"),
             cls_id=np.array([c for c in mean_sizes for _ in mean_sizes[c]], np.int64),
             size=np.array([s for c in mean_sizes for s in mean_sizes[c]]).reshape(-1, 3))
    print("%s: %d boxes, %d of %d vertices inside one" % (args.out_dir, len(boxes), int(scan['point_votes'][:, 0].sum()),
                                                          len(vertices)))
    return args.out_dir


if __name__ == "__main__":
    main()
