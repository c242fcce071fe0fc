"""ISCNet: sub-networks assembled by name from the config's `model:` block and
the generation pipeline of the reference's demo / test drivers.

  ISCNet.__init__   models/iscnet/modules/network.py:17-54 (phase -> attribute
                    names backbone, voting, detection, skip_propagation,
                    completion; classes looked up in MODULES)
  ISCNet.generate   demo.py:200-276 `generate` / network.py:56-180 (minus the
                    GT-dependent steps, which need datasets absent here)
  load_weight       models/network.py:81-89 (strip `module.`, module-by-module,
                    missing keys tolerated)

Proposal selection.  'nms' is the reference's behaviour: proposals with
objectness > dump_threshold that survive empty-box removal and class-aware 3-D
NMS (parse_predictions, ap_helper.py:131-264 -- CPU numpy + scipy there, device
kernels here, see predictions.py).  'all' keeps every one of the num_target
proposals (BASELINE configs 1-4 are quoted on "256 proposals"); 'objectness'
applies the probability threshold only.
"""
import numpy as np
import torch
import torch.nn as nn

from . import (loss, occupancy_net, pointnet2backbone, proposal_module,  # noqa: F401  (register)
               skip_propagation, vote_module)
from .registers import LOSSES, METHODS, MODULES


class _StageFlag(Exception):
    """status bits raised by the stages in front of the completion (internal to ISCNet.reconstruct / complete)"""

    def __init__(self, status):
        super().__init__("status %d" % status)
        self.status = status


@METHODS.register_module
class ISCNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        phase = cfg.config[cfg.config['mode']]['phase']
        phase_names = []
        if phase in ['detection']:
            phase_names += ['backbone', 'voting', 'detection']
        if phase in ['completion']:
            phase_names += ['backbone', 'voting', 'detection', 'completion']
            if cfg.config['data']['skip_propagate']:
                phase_names += ['skip_propagation']
        if not cfg.config.get('model') or not phase_names:
            raise ModuleNotFoundError('No submodule found. Please check the phase name and model definition.')
        for phase_name, net_spec in cfg.config['model'].items():
            if phase_name not in phase_names:
                continue
            cls = MODULES.get(net_spec['method'])
            if cls is None:
                raise ModuleNotFoundError('unknown module %r' % net_spec['method'])
            self.add_module(phase_name, cls(cfg, None))
            # the phase's loss function (network.py:49-50): a plain attribute, no parameter and no state_dict key
            setattr(self, phase_name + '_loss', LOSSES.get(net_spec.get('loss'), 'Null')(net_spec.get('weight', 1)))

    def load_weight(self, pretrained_model):
        """state_dict with the reference's key names (optionally `module.`-prefixed)."""
        own = self.state_dict()
        stripped = {'.'.join(k.split('.')[1:]) if k.startswith('module.') else k: v
                    for k, v in pretrained_model.items()}
        own.update({k: v for k, v in stripped.items() if k in own})
        self.load_state_dict(own)

    def worker_view(self):
        """A second handle on THIS network for another host thread / stream: every parameter, buffer, sub-module and
        cache (packed weights, the generator's round-0 query lists) is shared (read-only at inference; an
        _lib.ArtefactCache evicts safely under scenes in flight); only the mesh generator -- the one object that keeps
        per-call state (query statistics, the mesh buffers of the last call, the round hook) -- is the view's own.
        Several scenes in flight per GPU then cost one set of weights, not one per scene."""
        import copy
        view = copy.copy(self)
        view._modules = dict(self._modules)              # a dict of its own: re-pointing `completion` stays local
        comp = copy.copy(self.completion)
        comp.__dict__ = dict(self.completion.__dict__)
        gen = copy.copy(self.completion.generator)
        gen.__dict__ = dict(self.completion.generator.__dict__)
        gen.model, gen.stats, gen.round_hook = comp, {}, None
        gen.__dict__.pop('last_buffers', None)
        comp.generator = gen
        view._modules['completion'] = comp
        return view

    # ---------------------------------------------------------------- stages ---
    def detect(self, point_clouds):
        """backbone -> voting (+L2 norm) -> proposal  (demo.py:206-221)."""
        end_points = self.backbone(point_clouds, {})
        xyz, features = end_points['fp2_xyz'], end_points['fp2_features']
        end_points['seed_inds'] = end_points['fp2_inds']
        end_points['seed_xyz'] = xyz
        end_points['seed_features'] = features
        xyz, features = self.voting(xyz, features)
        features = features.div(torch.norm(features, p=2, dim=1).unsqueeze(1))
        end_points['vote_xyz'] = xyz
        end_points['vote_features'] = features
        end_points, proposal_features = self.detection(xyz, features, end_points, True)
        return end_points, proposal_features

    def select_proposals(self, end_points, selection='all', point_clouds=None):
        """-> (B, K, 1) int64 proposal ids (the layout of BATCH_PROPOSAL_IDs, demo.py:50-75)."""
        B, P = end_points['center'].shape[0], end_points['center'].shape[1]
        dev = end_points['center'].device
        if selection == 'all':
            return torch.arange(P, device=dev).view(1, P, 1).expand(B, P, 1).contiguous()
        if selection == 'nms':      # the reference's behaviour (demo.py:223-234)
            from . import predictions
            eval_dict, parsed = predictions.parse_predictions(
                end_points, point_clouds, self.cfg.dataset_config, getattr(self.cfg, 'eval_overrides', None))
            end_points['parsed_predictions'] = parsed
            end_points['pred_mask'] = eval_dict['pred_mask']
            return predictions.get_proposal_id(end_points, eval_dict['pred_mask'],
                                               self.cfg.config['generation']['dump_threshold'])
        if selection == 'objectness':
            assert B == 1
            thr = self.cfg.config['generation']['dump_threshold']
            prob = torch.softmax(end_points['objectness_scores'], dim=2)[..., 1]
            ids = torch.nonzero(prob[0] > thr).view(1, -1, 1)
            return ids
        raise ValueError(selection)

    def object_codes(self, end_points, proposal_features, ids, point_clouds, labels=None):
        """gather per-proposal features / centres / headings and run skip
        propagation (demo.py:236-258) -> (B*K, c_dim).
        labels: (point_instance_labels (B,N), proposal_instance_labels (B,K), sink) -- the test mode's call of
        SkipPropagation.forward (network.py:123-124); its mask loss goes to sink['mask_loss']."""
        dev = end_points['center'].device
        idx = ids[..., 0]
        feats = torch.gather(proposal_features, 2, idx.unsqueeze(1).expand(-1, 128, -1))
        if not self.cfg.config['data']['skip_propagate']:
            obj = feats
        else:
            centers = torch.gather(end_points['center'], 1, idx.unsqueeze(-1).expand(-1, -1, 3))
            dc = self.cfg.dataset_config
            heading_class = torch.argmax(end_points['heading_scores'], -1)
            residuals = end_points['heading_residuals_normalized'] * (np.pi / dc.num_heading_bin)
            heading_residual = torch.gather(residuals, 2, heading_class.unsqueeze(-1)).squeeze(2)
            angles = dc.class2angle_cuda(heading_class, heading_residual)
            angles = torch.gather(angles, 1, idx)
            if labels is not None:
                obj, labels[2]['mask_loss'] = self.skip_propagation(centers.contiguous(), angles, feats, point_clouds,
                                                                    labels[0], labels[1])
            else:
                obj = self.skip_propagation.generate(centers.contiguous(), angles, feats, point_clouds)
        B, C, K = obj.size()
        return obj.transpose(1, 2).contiguous().view(B * K, C)

    def cls_codes(self, end_points, ids):
        sem = end_points['sem_cls_scores']
        g = torch.gather(sem, 1, ids[..., 0].unsqueeze(-1).expand(-1, -1, sem.size(2)))
        one_hot = (g >= torch.max(g, dim=2, keepdim=True)[0]).float()
        return one_hot.view(-1, sem.size(2))

    @torch.no_grad()
    def fit_mesh_to_scan(self, pred_mesh_dict, parsed_predictions, eval_dict, input_scan, dump_threshold,
                         method='autograd'):
        """Box refinement of the evaluation path (network.py:182-303); see iscnet/fit.py.
        pred_mesh_dict = {'meshes': [...], 'proposal_ids': (B,K',1)} as in the reference.
        method: 'autograd' (the reference's padded loop) or 'device' (the ragged loop of csrc/fit_pose.hip)."""
        from . import fit
        return fit.fit_mesh_to_scan(pred_mesh_dict['meshes'], pred_mesh_dict['proposal_ids'], parsed_predictions,
                                    eval_dict, input_scan, dump_threshold, method=method)

    def generate(self, data, selection='all', return_grids=False, hook=None, labels_sink=None):
        """data['point_clouds'] (B,N,3+f) -> (end_points, proposal ids, meshes).  hook: see reconstruct().
        labels_sink: a dictionary, for the test mode with losses: `data` then carries the ground truth, and the proposal ->
        ground-truth pairing is made BEFORE skip propagation, so that the proposals' instance labels exist when the codes
        are built (network.py:97, 123-124); the sink receives 'pairs' (evaluation.proposal_to_gt) and 'mask_loss'."""
        pc = data['point_clouds']
        end_points, proposal_features = self.detect(pc)
        ids = self.select_proposals(end_points, selection, pc)
        if ids.shape[1] == 0:                  # nothing survived the selection
            # detect() may have raised a flag (FPS abort): it is this scene's, read it before returning (reconstruct()
            # does the same on the other path)
            from .. import _lib
            _lib.raise_status(_lib.stream_status_bits())
            return end_points, ids, []
        labels = None
        if labels_sink is not None:
            from . import evaluation
            labels_sink['pairs'] = pairs = evaluation.proposal_to_gt(end_points, data, ids)
            if self.cfg.config['data']['skip_propagate'] and 'point_instance_labels' in data and \
                    'object_instance_labels' in data:
                wanted = torch.gather(data['object_instance_labels'].to(pc.device), 1, pairs[:, :, 1])
                labels = (data['point_instance_labels'], wanted, labels_sink)
        out = self.reconstruct(end_points, proposal_features, ids, pc, return_grids=return_grids, hook=hook, labels=labels)
        return end_points, ids, out

    def loss(self, est_data, gt_data):
        """network.py:473-487: est_data = (end_points, completion_loss (1,2): [completion loss, mask loss], ...) -> the
        detection dictionary, plus completion_loss / mask_loss and the `total` update when the phase is `completion`."""
        end_points, completion_loss = est_data[:2]
        total_loss = self.detection_loss(end_points, gt_data, self.cfg.dataset_config)
        if self.cfg.config[self.cfg.config['mode']]['phase'] == 'completion':
            completion_loss = self.completion_loss(completion_loss)
            total_loss = {**total_loss, 'completion_loss': completion_loss['completion_loss'],
                          'mask_loss': completion_loss['mask_loss']}
            total_loss['total'] = total_loss['total'] + completion_loss['total_loss']
        return total_loss

    def evaluate(self, data, fit=True, ap_iou_thresh=(0.25, 0.5), timing=False, completion=False, completion_eps=None,
                 losses=False, mesh=False, voxel_size=None, mesh_distance=False, distance_samples=10000,
                 distance_thresholds=(0.05, 0.10)):
        """The tail of the reference's `generate` in test mode (network.py:85-177): detection and completion with
        selection='nms', then (fit: True or 'autograd', or 'device' for the ragged loop of csrc/fit_pose.hip; False for
        none) the box refinement of fit_mesh_to_scan, then the evaluation records of the --
        refined -- boxes against the ground-truth labels in `data` (center_label, heading_class_label,
        heading_residual_label, size_class_label, size_residual_label, sem_cls_label, box_label_mask).
        -> (end_points, proposal ids, meshes, records): what generate returns plus evaluation.SceneRecords, queued on
        the current stream (feed them to evaluation.APCalculator.step).  end_points['parsed_predictions'] holds the
        corners that were scored.
        completion=True adds the ground-truth-dependent completion block (network.py:126-150): `data` also carries
        object_points (B,G,T,3), object_points_occ (B,G,T) and optionally object_voxels (B,G,16,16,16); every selected
        proposal is paired with its nearest ground-truth box (evaluation.proposal_to_gt), that box's occupancy samples
        are gathered (prepare_data) and ONet.compute_loss is run on them (completion_eps: its `eps`).  Results:
        end_points['completion_loss'] (0-d device tensor), ['proposal_to_gt'] (B,K',3) and ['iou_stats'] =
        {'cls','iou'} numpy arrays over the B*K' proposals (None without object_voxels).  The return tuple is the same.
        losses=True adds the loss dictionary the reference prints beside the metrics (testing.py:63-68): `data` also
        carries vote_label (B,N,9) and vote_label_mask (B,N), and for the mask loss point_instance_labels (B,N) and
        object_instance_labels (B,G) (absent: mask loss 0).  end_points['loss'] = ISCNet.loss(...): DetectionLoss's thirteen
        keys, completion_loss, mask_loss, and `total` with ONet_Loss's weight * (completion + 100 mask) added.
        mesh=True adds the mesh half of the reference's evaluation (ap_helper.py:267-323, :371-401; one scene, as its
        `assert bsize == 1`): the generated meshes are placed in the boxes that are scored (after fit_mesh_to_scan if it
        ran), the ground-truth meshes data['gt_meshes'] -- one (vertices, faces) per ground-truth row with box_label_mask
        == 1, None for a missing mesh -- in the ground-truth boxes, both sides are voxelised (voxel_size: 0.047) and the
        mesh IoU of every pair (mesh_eval.scene_mesh_iou, kept in end_points['mesh_iou'] (1,K,G)) is matched like the box
        IoU: the records carry 'tp_mesh' for mesh_eval.MeshAPCalculator.  A detection that takes part but has no mesh
        has mesh IoU 0 with everything (the reference raises ValueError there).
        mesh_distance=True (off by default: without it evaluate makes exactly the calls it made) adds the surface metrics
        of every selected proposal against its ground truth (one scene; data['gt_meshes'] as for mesh=True): the pairs are
        the rows of evaluation.proposal_to_gt, the meshes are placed as for the mesh IoU, and
        end_points['mesh_distance'] = mesh_eval.scene_mesh_distance's dict (accuracy, completeness, chamfer_l1, chamfer_sq,
        precision, recall, fscore, normal_consistency, rms; distance_samples points per mesh, distance_thresholds in
        scan units) plus 'pairs' (P,3): proposal id, ground-truth row, ground-truth class."""
        from . import evaluation, fit as fit_module
        method = fit_module.fit_method(fit)
        captured = {}
        hook = (lambda codes, cls: captured.update(codes=codes, cls=cls)) if completion else None
        end_points, ids, meshes = self.generate(data, selection='nms', hook=hook, labels_sink=captured if losses else None)
        if completion:
            self._completion_block(end_points, data, ids, captured, completion_eps)
        if losses:
            dev = end_points['center'].device
            zero = torch.zeros((), device=dev)
            value = torch.stack([end_points.get('completion_loss', zero).float(),
                                 captured.get('mask_loss', zero).float()]).unsqueeze(0)
            end_points['loss'] = self.loss((end_points, value), data)
        parsed = end_points['parsed_predictions']
        eval_dict = {'pred_mask': end_points['pred_mask']}
        if method and len(meshes):
            parsed = self.fit_mesh_to_scan({'meshes': meshes, 'proposal_ids': ids}, parsed, eval_dict,
                                           data['point_clouds'], self.cfg.config['generation']['dump_threshold'],
                                           method=method)
            end_points['parsed_predictions'] = parsed
        parsed_gts = evaluation.parse_groundtruths(data, self.cfg.dataset_config)
        mesh_iou = None
        if mesh:
            from . import mesh_eval
            mesh_iou = end_points['mesh_iou'] = mesh_eval.scene_mesh_iou(
                meshes, ids, parsed, parsed_gts, data['gt_meshes'], voxel_size or mesh_eval.VOXEL_SIZE)
        if mesh_distance:
            from . import mesh_eval
            pairs = captured['pairs'] if 'pairs' in captured else evaluation.proposal_to_gt(end_points, data, ids)
            if pairs.shape[0] != 1:
                raise ValueError("mesh distance runs on one scene at a time, got a batch of %d" % pairs.shape[0])
            end_points['mesh_distance'] = dict(
                mesh_eval.scene_mesh_distance(meshes, ids, parsed, parsed_gts, data['gt_meshes'], pairs[0],
                                              distance_samples, distance_thresholds), pairs=pairs[0])
        records = evaluation.scene_records(eval_dict, parsed, parsed_gts, getattr(self.cfg, 'eval_overrides', None),
                                           ap_iou_thresh, timing=timing, mesh_iou=mesh_iou)
        return end_points, ids, meshes, records

    @torch.no_grad()
    def _completion_block(self, end_points, data, ids, captured, eps):
        from . import evaluation
        dev = end_points['center'].device
        end_points['iou_stats'] = None
        if ids.shape[1] == 0:
            end_points['completion_loss'] = torch.zeros((), device=dev)
            end_points['proposal_to_gt'] = ids.new_zeros(ids.shape[0], 0, 3)
            return
        pairs = captured['pairs'] if 'pairs' in captured else evaluation.proposal_to_gt(end_points, data, ids)
        on_dev = {k: data[k].to(dev) for k in ('object_points', 'object_points_occ')}
        points, occ = evaluation.prepare_data(on_dev, pairs)
        voxels = data.get('object_voxels')
        loss, _, terms = self.completion.compute_loss(captured['codes'], points, occ, captured['cls'],
                                                      export_shape=voxels is not None, eps=eps, return_terms=True)
        end_points['completion_loss'] = loss
        end_points['proposal_to_gt'] = pairs
        if voxels is not None:
            voxels = voxels.to(dev)
            B, Kp = pairs.shape[:2]
            box = pairs[:, :, 1].view(B, Kp, 1, 1, 1).expand(B, Kp, *voxels.shape[2:])
            gt = torch.gather(voxels, 1, box).reshape(B * Kp, -1)
            iou = evaluation.voxel_iou(terms['voxel_logits'], self.completion.logit_threshold(), gt)
            end_points['iou_stats'] = {'cls': pairs[:, :, 2].reshape(-1).cpu().numpy(), 'iou': iou.cpu().numpy()}

    def reconstruct(self, end_points, proposal_features, ids, pc, return_grids=False, hook=None, labels=None):
        """skip propagation -> object codes -> occupancy completion for the selected proposals, with the status
        reads that must follow (see complete()).  A split-precision GEMM activation beyond the f16 range at the
        default scale (_lib.STATUS_GEMM_RANGE, skip-propagation encoder) does not fail the scene either: the stage is run
        again at the fallback scale (gemm.lower_scale), and only a second flag raises.
        hook(codes, cls): called before the completion (the benchmark installs its copy scheduling there).
        labels: see object_codes()."""
        from .. import _lib, gemm
        for attempt in (0, 1):
            # the GEMM scale THIS attempt runs at: the model (and gemm.SA) is shared by every scene in flight, so
            # another scene may lower it while this one runs
            sa_used = gemm.SA
            codes = self.object_codes(end_points, proposal_features, ids, pc, labels)
            cls = self.cls_codes(end_points, ids)
            # A snapshot of the stream's status word is taken HERE, before the completion, without waiting: a GEMM that
            # overflowed has clipped the codes, and a decoder run on clipped codes could raise ITS range flag -- the
            # completion must then neither lower the decoder's scale for good nor hide the GEMM's flag.
            # The snapshot is read after the completion's own status read has synchronised the stream.
            with torch.cuda.device(pc.device):
                snap = _lib.StatusSnapshot()
            if hook is not None:
                hook(codes, cls)
            try:
                return self.complete(codes, cls, pc.device, return_grids=return_grids, before=snap)
            except _StageFlag as e:
                if e.status & _lib.STATUS_GEMM_RANGE and not e.status & ~_lib.STATUS_GEMM_RANGE and attempt == 0:
                    with _lib.BUILD_LOCK:
                        lowered = gemm.lower_scale()
                    # again when the scale came down -- by this scene, or by another scene in flight since this one
                    # started (its run was at the OLD scale: lower_scale() says "already at the fallback" but THIS
                    # scene has never run there); only a flag raised AT the fallback scale is a real overflow
                    if lowered or gemm.SA < sa_used:
                        continue
                _lib.raise_status(e.status)                # FPS abort, or an overflow at the fallback scale
                raise

    def complete(self, codes, cls, device, return_grids=False, before=None):
        """Occupancy completion of the selected proposals + the status read that must follow it.
        FPS exchange time-outs and f16-range flags are reported through the stream's status word, not through
        return codes (the kernels are asynchronous): never hand back results without reading it (waits for THIS
        stream only; several scenes may be in flight, each stream has its own word).  A decoder activation beyond
        the f16 range at the default scale does not fail the scene: the completion is run again at the fallback
        scale (the reference's fp32 decoder cannot overflow, occ_decoder.py:110-123) and only a second flag raises.
        before: a StatusSnapshot taken in front of the completion -- flags in it belong to the stages before (raised as
        _StageFlag for reconstruct() to answer) and are looked at FIRST: the decoder's scale is not touched on their
        account."""
        from .occ_decoder import run_with_range_fallback
        gen = self.completion.generator
        run = gen.generate_grids if return_grids else gen.generate_mesh

        def stage_flags():
            if before.read():
                raise _StageFlag(before.read())
        # refinement draws its weights from numpy's global stream: a second run (the range fallback) starts from the
        # state the first one started from, so the stream is consumed once, as by the reference
        rng = np.random.get_state() if getattr(gen, 'refinement_step', 0) > 0 and gen.refine_eps_source == 'numpy' else None

        def stage():
            if rng is not None:
                np.random.set_state(rng)
            return run(codes, cls)
        return run_with_range_fallback(self.completion.decoder, stage, device,
                                       None if before is None else stage_flags)

    @staticmethod
    def check_device_status(device):
        from .. import _lib
        with torch.cuda.device(device):
            _lib.stream_status()
