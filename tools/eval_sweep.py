"""Detection mAP / AR of a sweep through ISCNet.evaluate, with the cost of the evaluation stage.

    python tools/eval_sweep.py --scenes 8 [--gpus M] [--no-fit | --fit-method device]
    python tools/eval_sweep.py --weight ckpt.pth --gt DIR --mean_size_npz scannet_means.npz

Synthetic scenes (rfdnet_amd.synthetic.synthetic_scene(return_boxes=True): the 12 furniture cuboids are the ground
truth) or ScanNet-format ground-truth .npz files, one per scan, holding `point_clouds` (N,4) and the label arrays
parse_groundtruths reads.  Prints ONE JSON line and writes it to profiles/eval_stage.json:
  mAP / AR and the per-class values at IoU 0.25 and 0.5; the evaluation stage's device milliseconds per scene (HIP
  events around its two launches, averaged over every rank's scenes); host seconds of compute_metrics; scenes/s of
  the same scenes through ISCNet.generate(selection='nms') [+ fit] without and with the evaluation, one scene at a
  time between device synchronisations ("scenes_in_flight": 1), the two legs alternating in which goes first.  A
  host-side cost that only shows with several scenes in flight is NOT visible to this tool.
With seeded weights the mAP is near zero: the tool then exists for the path and the timing ("weights": "seeded").
--completion (synthetic scenes, one process) adds a leg through ISCNet.evaluate(completion=True) on per-object occupancy
samples and 16^3 voxels of the ground-truth cuboids (synthetic.object_occupancy): the mean completion loss and voxel IoU
go into the line as "completion".  It attaches the latent encoder before the weights are seeded, which shifts the
seeded completion weights: the other figures of such a run are not comparable with a run without the flag.
--mesh (synthetic scenes) adds mesh mAP: the ground-truth mesh of a box is a unit cube (12 faces) placed in the box,
ISCNet.evaluate(mesh=True) voxelises it and the generated meshes, and "mAP_mesh@..." / "AR_mesh@..." join the line.  The
timed legs then include the mesh stage ("scenes_per_s_with_eval").
--mesh_distance (synthetic scenes, one process) adds "mesh_distance": the per-class means of the Chamfer distance, the
F-score and the normal consistency of every selected proposal's mesh against its ground truth's unit cube
(ISCNet.evaluate(mesh_distance=True)), from a pass of its own after the timed legs.
With --gpus M the scenes are dealt round robin to M processes (sharding.launch_local_ranks) and the records meet in
one all_gather (sharding.gather_records); throughput is all scenes over the slowest rank.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LABELS = ('center_label', 'heading_class_label', 'heading_residual_label', 'size_class_label', 'size_residual_label',
          'sem_cls_label', 'box_label_mask')


def labels_from_boxes(boxes, cls, dataset_config, max_obj=64):
    """(n,7) centre / size / heading + class ids -> the label arrays of one scene (1, max_obj, ...)"""
    nh, mean = dataset_config.num_heading_bin, dataset_config.mean_size_arr
    out = {'center_label': np.zeros((1, max_obj, 3), np.float32), 'heading_class_label': np.zeros((1, max_obj), np.int64),
           'heading_residual_label': np.zeros((1, max_obj), np.float32), 'size_class_label': np.zeros((1, max_obj), np.int64),
           'size_residual_label': np.zeros((1, max_obj, 3), np.float32), 'sem_cls_label': np.zeros((1, max_obj), np.int64),
           'box_label_mask': np.zeros((1, max_obj), np.float32)}
    for j, (b, c) in enumerate(zip(boxes, cls)):
        shifted = (b[6] % (2 * np.pi) + np.pi / nh) % (2 * np.pi)          # angle2class (scannet_config.py:27-41)
        hc = int(shifted / (2 * np.pi / nh))
        out['center_label'][0, j] = b[:3]
        out['heading_class_label'][0, j] = hc
        out['heading_residual_label'][0, j] = shifted - (hc * (2 * np.pi / nh) + np.pi / nh)
        out['size_class_label'][0, j] = int(c) % len(mean)
        out['size_residual_label'][0, j] = b[3:6] - mean[int(c) % len(mean)]
        out['sem_cls_label'][0, j] = int(c)
        out['box_label_mask'][0, j] = 1
    return out


CUBE_VERTICES = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                       [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def load_scene(args, i, cfg, files):
    from rfdnet_amd import synthetic
    if files:
        d = np.load(files[i])
        data = {k: np.asarray(d[k])[None] for k in LABELS}
        data['point_clouds'] = np.asarray(d['point_clouds'], np.float32)[None]
    else:
        pc, boxes, cls = synthetic.synthetic_scene(seed=args.seed + i, n_raw=int(args.points * 1.5), n_points=args.points,
                                                   return_boxes=True)
        data = labels_from_boxes(boxes, cls, cfg.dataset_config)
        data['point_clouds'] = pc[None]
        if getattr(args, 'completion', False):
            max_obj = data['box_label_mask'].shape[1]
            for k, a in zip(('object_points', 'object_points_occ', 'object_voxels'),
                            synthetic.object_occupancy(boxes, seed=args.seed + i)):
                data[k] = np.zeros((1, max_obj) + a.shape[1:], np.float32)
                data[k][0, :len(boxes)] = a
    out = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
    if getattr(args, 'mesh', False) or getattr(args, 'mesh_distance', False):
        out['gt_meshes'] = [(CUBE_VERTICES, CUBE_FACES)] * int((data['box_label_mask'][0] == 1).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--weight", type=str, default=None)
    ap.add_argument("--gt", type=str, default=None, help="directory of ground-truth .npz files (one per scan)")
    ap.add_argument("--mean_size_npz", type=str, default=None)
    ap.add_argument("--resolution_0", type=int, default=None)
    ap.add_argument("--upsampling_steps", type=int, default=None)
    ap.add_argument("--no-fit", action="store_true", help="score the decoded boxes without fit_mesh_to_scan")
    ap.add_argument("--fit-method", choices=("autograd", "device"), default="autograd",
                    help="fit_mesh_to_scan's method: the padded autograd loop (default) or the ragged loop on the device")
    ap.add_argument("--completion", action="store_true",
                    help="synthetic scenes, --gpus 1: also report the completion loss and the voxel IoU")
    ap.add_argument("--mesh", action="store_true",
                    help="synthetic scenes: also report mesh mAP / AR against unit-cube ground-truth meshes")
    ap.add_argument("--mesh_distance", action="store_true",
                    help="synthetic scenes, --gpus 1: also report the surface metrics of every selected proposal against "
                         "its unit-cube ground-truth mesh (per-class means of the Chamfer distance and the F-score)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "eval_stage.json"))
    args = ap.parse_args()
    if args.mesh_distance and (args.gt or args.gpus > 1):
        ap.error("--mesh_distance runs on synthetic scenes in one process")
    if args.mesh and args.gt:
        ap.error("--mesh runs on synthetic scenes (their ground-truth meshes are unit cubes)")
    if args.completion and (args.gt or args.gpus > 1):
        ap.error("--completion runs on synthetic scenes in one process")

    from rfdnet_amd import sharding, synthetic
    if args.gpus > 1 and not sharding.launched():
        sys.exit(sharding.launch_local_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    rank, local_rank, world = sharding.rank_env()
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world)

    from rfdnet_amd.iscnet import evaluation
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    gen = {k: v for k, v in (('resolution_0', args.resolution_0), ('upsampling_steps', args.upsampling_steps))
           if v is not None}
    cfg = Config({'generation': gen, 'data': {'latent_encoder': args.completion}}, mean_size_arr=args.mean_size_npz)
    if cfg.dataset_config.placeholder_sizes:
        if args.weight:
            raise FileNotFoundError("a real checkpoint needs the class mean sizes (--mean_size_npz)")
        cfg.eval_overrides['allow_placeholder_sizes'] = True
    net = ISCNet(cfg)
    if args.weight:
        ckpt = torch.load(args.weight, map_location="cpu")
        net.load_weight(ckpt.get('net', ckpt))
    else:
        synthetic.load_seeded(net, seed=cfg.config['seed'])
    net = net.cuda().eval()
    files = sorted(glob.glob(os.path.join(args.gt, "*.npz"))) if args.gt else None
    n_scenes = len(files) if files else args.scenes
    mine = sharding.scene_ids_for_rank(n_scenes, rank, world)
    fit = False if args.no_fit else args.fit_method                      # evaluate()'s `fit`: a method name or False
    thr = (0.25, 0.5)
    dump = cfg.config['generation']['dump_threshold']

    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)                       # the placeholder-size warning, once per scene
    def without_eval(data):
        end_points, ids, meshes = net.generate(data, selection='nms')
        if fit and len(meshes):
            net.fit_mesh_to_scan({'meshes': meshes, 'proposal_ids': ids}, end_points['parsed_predictions'],
                                 {'pred_mask': end_points['pred_mask']}, data['point_clouds'], dump, method=fit)

    def timed(fn, data):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(data)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    records, stage_ms, t_off, t_on = [], [], 0.0, 0.0
    if mine:                                                              # warm-up: caches, packed weights, allocator
        net.evaluate(load_scene(args, mine[0], cfg, files), fit=fit, ap_iou_thresh=thr, mesh=args.mesh)[3].compact()
    for n, i in enumerate(mine):
        data = load_scene(args, i, cfg, files)
        with_eval = lambda d: net.evaluate(d, fit=fit, ap_iou_thresh=thr, timing=True, mesh=args.mesh)[3]
        if n % 2:                                                         # the leg that goes first alternates
            rec, dt_on = timed(with_eval, data)
            _, dt_off = timed(without_eval, data)
        else:
            _, dt_off = timed(without_eval, data)
            rec, dt_on = timed(with_eval, data)
        t_off += dt_off
        t_on += dt_on
        records.append(rec)
        stage_ms.append(rec.device_ms())
    completion = None
    if args.completion:
        losses, ious = [], []
        for i in mine:
            ep = net.evaluate(load_scene(args, i, cfg, files), fit=False, ap_iou_thresh=thr, completion=True)[0]
            losses.append(float(ep['completion_loss']))
            ious += [] if ep['iou_stats'] is None else list(ep['iou_stats']['iou'])
        completion = {"loss": float(np.mean(losses)) if losses else None, "proposals": len(ious),
                      "voxel_iou": float(np.nanmean(ious)) if ious else None}
    distance = None
    if args.mesh_distance:
        from rfdnet_amd.iscnet.mesh_eval import class_means
        rows = {'chamfer_l1': [], 'fscore': [], 'normal_consistency': [], 'cls': []}
        for i in mine:
            md = net.evaluate(load_scene(args, i, cfg, files), fit=fit, ap_iou_thresh=thr, mesh_distance=True)[0]['mesh_distance']
            for k in ('chamfer_l1', 'fscore', 'normal_consistency'):
                rows[k].append(md[k])
            rows['cls'].append(md['pairs'][:, 2])
        if rows['cls']:
            cat = {k: torch.cat(v) for k, v in rows.items()}
            distance = {"pairs": int(cat['cls'].numel()), "thresholds": [0.05, 0.10],
                        "per_class": {k: class_means(cat, cat['cls'], k) for k in ('chamfer_l1', 'fscore', 'normal_consistency')}}
    # per rank: scenes, seconds without / with the evaluation, summed stage milliseconds
    mine_t = torch.tensor([len(mine), t_off, t_on, sum(stage_ms)], dtype=torch.float64, device="cuda")
    if dist is not None:
        times = torch.empty(world * 4, dtype=torch.float64, device="cuda")
        dist.all_gather_into_tensor(times, mine_t)
        times = times.view(world, 4).cpu().numpy()
    else:
        times = mine_t.view(1, 4).cpu().numpy()
    gathered = sharding.gather_records(records, dist, thr=thr)
    if rank == 0:
        if args.mesh:
            from rfdnet_amd.iscnet.mesh_eval import MeshAPCalculator
        calc = MeshAPCalculator(thr) if args.mesh else evaluation.APCalculator(thr)
        calc.step(gathered)
        t0 = time.perf_counter()
        m25, m50 = calc.compute_metrics()
        host_s = time.perf_counter() - t0
        num = lambda d: {k: (None if np.isnan(v) else float(v)) for k, v in d.items()}
        steps = times[:, 0].sum()
        rate = lambda col: float(steps / times[:, col].max()) if steps else None
        line = {"tool": "eval_sweep", "weights": "checkpoint" if args.weight else "seeded", "scenes": int(steps),
                "gpus": world, "fit": bool(fit), "fit_method": fit or None, "points": args.points if not files else None,
                "scenes_in_flight": 1,        # one scene at a time per GPU, timed between device synchronisations
                "mAP@0.25": num(m25)['mAP'], "AR@0.25": num(m25)['AR'], "mAP@0.5": num(m50)['mAP'],
                "AR@0.5": num(m50)['AR'], "per_class@0.25": num(m25), "per_class@0.5": num(m50),
                "records": int(len(gathered['cls'])), "ground_truths": int(gathered['npos'].sum()),
                "eval_stage_device_ms_per_scene": float(times[:, 3].sum() / steps) if steps else None,
                "compute_metrics_host_s": host_s,
                "scenes_per_s_without_eval": rate(1), "scenes_per_s_with_eval": rate(2)}
        if args.mesh:
            line.update({"mAP_mesh@0.25": num(m25)['mAP_mesh'], "AR_mesh@0.25": num(m25)['AR_mesh'],
                         "mAP_mesh@0.5": num(m50)['mAP_mesh'], "AR_mesh@0.5": num(m50)['AR_mesh']})
        if completion is not None:
            line["completion"] = completion
        if distance is not None:
            line["mesh_distance"] = distance
        text = json.dumps(line)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
