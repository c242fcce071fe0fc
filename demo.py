#!/usr/bin/env python
"""`python main.py --mode demo` of the reference (main.py:17-38, demo.py:379-420)
for the MI355X path: load a scan (.off) or a seeded synthetic scene, reconstruct,
write the reference's output files.

  python demo.py --demo_path demo/inputs/scene0549_00.off --out out/scene0549_00
  python demo.py --synthetic 10 --out out/synth --upsampling_steps 1
  python demo.py --synthetic 10 --out out/synth --with_normals     (PLYs with per-vertex nx ny nz)
  python demo.py --synthetic 10 --out out/synth --refinement_step 30   (meshes refined against the occupancy field)
  python demo.py --synthetic 10 --out out/synth --keep_components largest   (floaters dropped: the largest component stays)
  python demo.py --synthetic 10 --out out/synth --decimate_cells 16    (meshes thinned by vertex clustering, 16^3 cells)
  python demo.py --synthetic 10 --out out/synth --simplify_nfaces 500   (meshes collapsed to 500 faces each, watertight)
  python demo.py --synthetic 10 --out out/synth --render --post_processing  (scene_objects.ply and pred.png as well)

Weights: --weight <pretrained_weight.pth> (reference checkpoint, key names kept);
without it seeded random weights are used (no pretrained weights ship with the
reference checkout)."""
import argparse
import time

import numpy as np
import torch


def keep_components_arg(text):
    """--keep_components: 'largest' or a fraction in [0, 1]"""
    if text == 'largest':
        return text
    t = float(text)
    if not 0.0 <= t <= 1.0:
        raise argparse.ArgumentTypeError("largest, or a fraction in [0, 1]")
    return t


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=None,
                    help="a reference config file (configs/config_files/ISCNet_test.yaml); its data / model / test / "
                         "generation blocks and its `weight` list are used, flags below override it")
    ap.add_argument("--mode", choices=["demo", "test"], default="demo")
    ap.add_argument("--demo_path", type=str, default=None)
    ap.add_argument("--synthetic", type=int, default=None, help="seed of a synthetic ScanNet-like scene")
    ap.add_argument("--weight", type=str, default=None)
    ap.add_argument("--out", type=str, default="out/demo")
    ap.add_argument("--resolution_0", type=int, default=None)
    ap.add_argument("--upsampling_steps", type=int, default=None)       # ISCNet_test.yaml:62-63 (32, 0)
    ap.add_argument("--selection", choices=["nms", "all", "objectness"], default="nms")
    ap.add_argument("--gt", type=str, default=None,
                    help="--mode test: .npz with the scan's ground-truth labels (center_label, heading_class_label, "
                         "heading_residual_label, size_class_label, size_residual_label, sem_cls_label, "
                         "box_label_mask); the scene then goes through ISCNet.evaluate and its box AP / recall at IoU "
                         "0.25 and 0.5 are printed.  If it also holds object_points, object_points_occ and "
                         "object_voxels, the completion loss and the mean voxel IoU are printed too (needs a "
                         "checkpoint with completion.encoder_latent.* to mean anything).  If it holds vote_label and "
                         "vote_label_mask, the loss dictionary of the reference's test mode is printed (detection loss; "
                         "with point_instance_labels and object_instance_labels also PointSeg's mask loss)")
    ap.add_argument("--shapenet_path", type=str, default=None,
                    help="--mode test with --gt: the directory of the ground-truth meshes (<catid>/<id>.off for the "
                         "scan's shapenet_catids / shapenet_ids arrays); also prints the mesh AP / recall of the scene")
    ap.add_argument("--mesh_distance", action="store_true",
                    help="--mode test with --gt and --shapenet_path: also prints the surface metrics of every selected "
                         "proposal against its ground-truth mesh (Chamfer distance, F-score, normal consistency, ...: "
                         "rfdnet_amd/mesh_distance.py), as per-class means")
    ap.add_argument("--mean_size_npz", type=str, default=None,
                    help="class mean sizes (the reference's datasets/scannet/scannet_means.npz); default: "
                         "$RFD_MEAN_SIZE_NPZ or that path relative to the working directory")
    ap.add_argument("--allow-placeholder-sizes", action="store_true",
                    help="synthetic runs only: let --selection nms decode boxes with placeholder class mean sizes when "
                         "no scannet_means.npz is available (the reference fails hard on the missing file; so does this "
                         "path without the flag)")
    ap.add_argument("--with_normals", action="store_true",
                    help="vertex normals from the occupancy field's gradient (generation.with_normals, "
                         "Generator3D.estimate_normals), written to the mesh PLYs as nx ny nz")
    ap.add_argument("--refinement_step", type=int, default=None,
                    help="RMSprop steps of Generator3D.refine_mesh on every mesh (generation.refinement_step; the "
                         "reference's configs use 0 or 30)")
    ap.add_argument("--decimate_cells", type=int, default=None,
                    help="thin every mesh by vertex clustering on an N^3 grid over its cube before normals and "
                         "refinement (Generator3D.set_decimation; generation.decimate_cells, 0 = off)")
    ap.add_argument("--simplify_nfaces", type=int, default=None,
                    help="simplify every mesh to at most N faces by quadric edge collapse on the device, after "
                         "--decimate_cells and before normals and refinement (Generator3D.set_simplification; "
                         "generation.simplify_faces, 0 = off)")
    ap.add_argument("--keep_components", type=keep_components_arg, default=None, metavar="largest|T",
                    help="drop the floaters of every mesh right after marching cubes, before --decimate_cells and "
                         "--simplify_nfaces: keep the largest connected component alone, or every component with at "
                         "least the fraction T of the largest's area (Generator3D.set_components; "
                         "generation.keep_components, 0 = off)")
    ap.add_argument("--render", action="store_true",
                    help="place every mesh in its box (iscnet.scene.place_objects), render scan and meshes on the device "
                         "and write scene_objects.ply and pred.png beside the other files (demo.py:329-377; needs "
                         "--selection nms or --mode test: the boxes come from the parsed predictions)")
    ap.add_argument("--render_size", type=int, nargs=2, default=(1024, 768), metavar=("W", "H"))
    ap.add_argument("--post_processing", action="store_true",
                    help="demo mode: refine the selected boxes with ISCNet.fit_mesh_to_scan(method='device') before the "
                         "meshes are placed (the reference's post_processing=True, demo.py:273-275)")
    return ap


def main():
    args = build_parser().parse_args()

    from rfdnet_amd import io, synthetic
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet

    gen = {k: v for k, v in (('resolution_0', args.resolution_0), ('upsampling_steps', args.upsampling_steps),
                             ('refinement_step', args.refinement_step), ('decimate_cells', args.decimate_cells),
                             ('simplify_faces', args.simplify_nfaces), ('keep_components', args.keep_components))
           if v is not None}
    if args.with_normals:
        gen['with_normals'] = True
    if args.config:
        cfg = Config.from_yaml(args.config, mode=args.mode, overrides={'generation': gen},
                               mean_size_arr=args.mean_size_npz)
        if not args.weight and cfg.config.get('weight'):
            import os
            w = cfg.config['weight'][0] if isinstance(cfg.config['weight'], (list, tuple)) else cfg.config['weight']
            if os.path.exists(w):
                args.weight = w
    else:
        cfg = Config({'generation': gen}, mean_size_arr=args.mean_size_npz)
    if args.allow_placeholder_sizes:
        cfg.eval_overrides['allow_placeholder_sizes'] = True
    completion_keys = ('object_points', 'object_points_occ', 'object_voxels')
    gt = np.load(args.gt) if args.mode == "test" and args.gt else None
    completion = gt is not None and all(k in gt.files for k in completion_keys)
    loss_keys = ('vote_label', 'vote_label_mask')
    instance_keys = ('point_instance_labels', 'object_instance_labels')
    losses = gt is not None and all(k in gt.files for k in loss_keys)
    if completion:
        cfg.config['data']['latent_encoder'] = True                      # before the weights are loaded: its keys are kept
    net = ISCNet(cfg)
    if args.weight:
        ckpt = torch.load(args.weight, map_location="cpu")
        net.load_weight(ckpt.get('net', ckpt))
    else:
        synthetic.load_seeded(net, seed=cfg.config['seed'])
    net = net.cuda().eval()
    if args.demo_path:
        data = io.load_demo_data(args.demo_path, cfg.config['data']['num_point'], seed=cfg.config['seed'])
    else:
        pc = synthetic.synthetic_scene(seed=args.synthetic if args.synthetic is not None else 10,
                                       n_points=cfg.config['data']['num_point'])
        data = {'point_clouds': torch.from_numpy(pc[None])}
    data = {k: v.cuda() for k, v in data.items()}                       # (gt_meshes, a list, joins it below)
    torch.cuda.synchronize()
    t0 = time.time()
    records = None
    if gt is not None:
        for k in ('center_label', 'heading_class_label', 'heading_residual_label', 'size_class_label',
                  'size_residual_label', 'sem_cls_label', 'box_label_mask'):
            a = np.asarray(gt[k])
            per_scan = 2 if k in ('center_label', 'size_residual_label') else 1
            data[k] = torch.from_numpy(a[None] if a.ndim == per_scan else a).cuda()      # one scan: add the batch axis
        for k in completion_keys if completion else ():
            a = np.asarray(gt[k], dtype=np.float32)
            per_scan = 3 if k == 'object_points' else 2 if k == 'object_points_occ' else 4
            data[k] = torch.from_numpy(a[None] if a.ndim == per_scan else a).cuda()
        for k in (loss_keys + instance_keys if losses and all(k in gt.files for k in instance_keys) else
                  loss_keys if losses else ()):
            a = np.asarray(gt[k])
            per_scan = 2 if k == 'vote_label' else 1
            data[k] = torch.from_numpy(a[None] if a.ndim == per_scan else a).cuda()
        with_meshes = args.shapenet_path is not None
        if with_meshes:
            from rfdnet_amd.iscnet.mesh_eval import load_gt_meshes
            if not all(k in gt.files for k in ('shapenet_catids', 'shapenet_ids')):
                raise SystemExit("--shapenet_path needs shapenet_catids and shapenet_ids in the --gt file")
            rows = np.nonzero(data['box_label_mask'][0].cpu().numpy() == 1)[0]
            names = [np.asarray(gt[k]).reshape(-1)[rows] for k in ('shapenet_catids', 'shapenet_ids')]
            data['gt_meshes'] = load_gt_meshes(args.shapenet_path, *names)
        if args.mesh_distance and not with_meshes:
            raise SystemExit("--mesh_distance needs the ground-truth meshes (--shapenet_path)")
        end_points, ids, meshes, records = net.evaluate(data, completion=completion, losses=losses, mesh=with_meshes,
                                                        mesh_distance=args.mesh_distance)
    else:
        end_points, ids, meshes = net.generate(data, selection=args.selection)
    if args.post_processing and gt is None and len(meshes) and 'parsed_predictions' in end_points:
        end_points['parsed_predictions'] = net.fit_mesh_to_scan(
            {'meshes': meshes, 'proposal_ids': ids}, end_points['parsed_predictions'],
            {'pred_mask': end_points['pred_mask']}, data['point_clouds'], cfg.config['generation']['dump_threshold'],
            method='device')
    torch.cuda.synchronize()
    print('Time elapsed: %s.' % (time.time() - t0))                       # demo.py:411
    if records is not None:
        from rfdnet_amd.iscnet.evaluation import APCalculator
        from rfdnet_amd.iscnet.mesh_eval import MeshAPCalculator
        calc = (MeshAPCalculator if args.shapenet_path is not None else APCalculator)((0.25, 0.5))
        calc.step(records)
        for thr, metrics in zip((0.25, 0.5), calc.compute_metrics()):
            print('IoU %g: %s' % (thr, {k: float(v) for k, v in metrics.items()}))
    if 'mesh_distance' in end_points:
        from rfdnet_amd.iscnet.mesh_eval import METRIC_KEYS, class_means
        md = end_points['mesh_distance']
        for key in METRIC_KEYS:                                           # per ground-truth class, over the pairs with a number
            print('mesh distance, %s per class: %s' % (key, class_means(md, md['pairs'][:, 2], key)))
    if 'completion_loss' in end_points:
        stats = end_points['iou_stats']
        print('completion loss: %.4f; mean voxel IoU over %d proposals: %s'
              % (float(end_points['completion_loss']), ids.shape[1],
                 'n/a' if stats is None or not len(stats['iou']) else '%.4f' % float(np.nanmean(stats['iou']))))
    if 'loss' in end_points:
        print('loss: %s' % {k: round(float(v), 6) for k, v in end_points['loss'].items()})
    box = keep = None
    if 'parsed_predictions' in end_points:
        box = end_points['parsed_predictions']['box_params'][0].cpu().numpy()
        keep = np.zeros(box.shape[0], dtype=bool)
        keep[ids[0, :, 0].cpu().numpy()] = True
    io.save_visualization(args.out, data['point_clouds'].cpu().numpy(), ids[0].cpu().numpy(), meshes, box, keep)
    print('%d meshes written to %s' % (len(meshes), args.out))
    if args.render:
        if 'parsed_predictions' not in end_points:
            raise SystemExit("--render needs the boxes of --selection nms (or --mode test)")
        from rfdnet_amd import render
        from rfdnet_amd.iscnet.scene import place_objects
        scene = place_objects(meshes, ids, end_points['parsed_predictions'], with_normals=args.with_normals)
        camera = render.Camera.fit(data['point_clouds'][0], width=args.render_size[0], height=args.render_size[1])
        io.save_scene(args.out, scene, render.render_scene(scene, data['point_clouds'], camera))
        print('scene_objects.ply and pred.png written to %s' % args.out)


if __name__ == "__main__":
    main()
