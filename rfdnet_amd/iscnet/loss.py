"""The losses the reference's test mode reports beside its metrics (models/loss.py), values only -- no gradient of any
loss is built.

  compute_vote_loss / compute_objectness_loss / compute_box_and_sem_cls_loss   models/loss.py:41-202
  DetectionLoss                                                               models/loss.py:205-271
  Null, ONet_Loss                                                             models/loss.py:33-38, 298-306
  huber_loss                                                                  net_utils/nn_distance.py:15-32

The detection loss is three launches of csrc/det_loss.hip (include/rfd_loss.h: seeds, proposals, finish) where the
reference runs about 150 torch kernels, and its twelve Python floats come from ONE copy of the result vector.  ChamferDist,
PCN_Loss and the BoxNet variants are not part of ISCNet_test.yaml and are left out."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .registers import LOSSES

FAR_THRESHOLD = 0.6
NEAR_THRESHOLD = 0.3
GT_VOTE_FACTOR = 3                         # number of GT votes per point
OBJECTNESS_CLS_WEIGHTS = [0.2, 0.8]        # put larger weights on positive objectness

PARTIALS = 16                              # RFD_LOSS_PARTIALS
KEYS = ('total', 'vote_loss', 'objectness_loss', 'box_loss', 'sem_cls_loss', 'pos_ratio', 'neg_ratio', 'center_loss',
        'heading_cls_loss', 'heading_reg_loss', 'size_cls_loss', 'size_reg_loss', 'obj_acc')      # the result vector


def huber_loss(error, delta=1.0):
    abs_error = torch.abs(error)
    quadratic = torch.clamp(abs_error, max=delta)
    linear = (abs_error - quadratic)
    return 0.5 * quadratic ** 2 + delta * linear


def _as(t, dtype, dev):
    """`t` on `dev`, contiguous, of `dtype`: no kernel when it already is (the dataloader's dtypes)"""
    return _lib.as_tensor(t, dev, dtype).contiguous()


def _strided(t):
    """(tensor, [batch, proposal, channel strides]) of a (B,K,C) or (B,K,NS,3) fp32 prediction, read in place when its
    channels are uniformly spaced (the head's slices are)"""
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() == 4:
        if t.stride(2) != 3 * t.stride(3):
            t = t.contiguous()
        return t, [t.stride(0), t.stride(1), t.stride(3)]
    return t, [t.stride(0), t.stride(1), t.stride(2)]


def _vote_partial(est_data, gt_data, partial):
    seed_xyz = est_data['seed_xyz']
    _lib.need_gpu(seed_xyz)
    dev = seed_xyz.device
    B, S = seed_xyz.shape[:2]
    vote_xyz = _as(est_data['vote_xyz'], torch.float32, dev)
    vote_factor = vote_xyz.shape[1] // max(S, 1)
    assert vote_xyz.shape[1] == S * vote_factor
    vote_label = _as(gt_data['vote_label'], torch.float32, dev)
    mask = _as(gt_data['vote_label_mask'], torch.int64, dev)
    N = mask.shape[1]
    assert vote_label.shape == (B, N, 3 * GT_VOTE_FACTOR)
    inds = _as(est_data['seed_inds'], torch.int32, dev)
    seed_xyz = _as(seed_xyz, torch.float32, dev)
    _lib.call("rfd_vote_loss_partial", dev, B, N, S, vote_factor, seed_xyz.data_ptr(), inds.data_ptr(),
              vote_xyz.data_ptr(), vote_label.data_ptr(), mask.data_ptr(), partial.data_ptr())


def _mean_size(config, dev):
    """config.mean_size_arr as fp32 on `dev`, uploaded once per config and device"""
    arr = np.ascontiguousarray(np.asarray(config.mean_size_arr).astype(np.float32))
    key = (str(dev), arr.tobytes())
    return _lib.build_once(config.__dict__, '_mean_size_f32_%s' % dev, key, lambda: torch.from_numpy(arr).to(dev), dev)


def _proposal_partial(est_data, gt_data, config, partial, meta_data=None):
    agg = est_data['aggregated_vote_xyz']
    _lib.need_gpu(agg)
    dev = agg.device
    B, K = agg.shape[:2]
    agg = _as(agg, torch.float32, dev)
    center = _as(est_data['center'], torch.float32, dev)
    names = ('objectness_scores', 'heading_scores', 'heading_residuals_normalized', 'size_scores',
             'size_residuals_normalized', 'sem_cls_scores')
    preds, strides = [], []
    for n in names:
        t, st = _strided(est_data[n])
        preds.append(t)
        strides += st
    NH, NS, NC = preds[1].shape[2], preds[3].shape[2], preds[5].shape[2]
    assert preds[0].shape == (B, K, 2) and preds[2].shape == (B, K, NH) and preds[4].shape == (B, K, NS, 3)
    assert (NH, NS, NC) == (config.num_heading_bin, config.num_size_cluster, config.num_class)
    center_label = gt_data['center_label'].to(dev)
    if center_label.dtype != torch.float32 or center_label.stride(2) != 1 or center_label.stride(0) != \
            center_label.shape[1] * center_label.stride(1):
        center_label = center_label.float().contiguous()
    G = center_label.shape[1]
    lab = {k: _as(gt_data[k], torch.int64, dev) for k in ('heading_class_label', 'size_class_label', 'sem_cls_label')}
    flt = {k: _as(gt_data[k], torch.float32, dev) for k in ('heading_residual_label', 'size_residual_label',
                                                            'box_label_mask')}
    given = meta_data is not None
    if given:
        objectness_label = _as(meta_data['objectness_label'], torch.int64, dev)
        assignment = _as(meta_data['object_assignment'], torch.int64, dev)
        objectness_mask = None
    else:
        objectness_label = torch.empty(B, K, dtype=torch.int64, device=dev)
        assignment = torch.empty(B, K, dtype=torch.int64, device=dev)
        objectness_mask = torch.empty(B, K, dtype=torch.float32, device=dev)
    st = (C.c_int * 18)(*[int(s) for s in strides])
    _lib.call("rfd_proposal_loss_partial", dev, B, K, G, NH, NS, NC, agg.data_ptr(), center.data_ptr(),
              *[p.data_ptr() for p in preds], st, center_label.data_ptr(), int(center_label.stride(1)),
              lab['heading_class_label'].data_ptr(), flt['heading_residual_label'].data_ptr(),
              lab['size_class_label'].data_ptr(), flt['size_residual_label'].data_ptr(),
              lab['sem_cls_label'].data_ptr(), flt['box_label_mask'].data_ptr(), _mean_size(config, dev).data_ptr(),
              objectness_label.data_ptr(), _lib.ptr(objectness_mask), assignment.data_ptr(), int(given),
              partial.data_ptr())
    return objectness_label, objectness_mask, assignment


def _finish(B, K, have, partial):
    out = torch.empty(len(KEYS), dtype=torch.float32, device=partial.device)
    _lib.call("rfd_detection_loss_finish", partial.device, B, K, have, partial.data_ptr(), out.data_ptr())
    return out


def _partials(B, dev):
    return torch.empty(B, PARTIALS, dtype=torch.float64, device=dev)


@torch.no_grad()
def compute_vote_loss(est_data, gt_data):
    """-> vote_loss, a 0-d device tensor (models/loss.py:41-88)"""
    _lib.need_gpu(est_data['seed_xyz'])
    dev = est_data['seed_xyz'].device
    B = est_data['seed_xyz'].shape[0]
    partial = _partials(B, dev)
    _vote_partial(est_data, gt_data, partial)
    return _finish(B, 1, 1, partial)[KEYS.index('vote_loss')]


@torch.no_grad()
def compute_objectness_loss(est_data, gt_data, config=None):
    """-> objectness_loss (0-d), objectness_label (B,K) int64, objectness_mask (B,K) f32, object_assignment (B,K) int64
    (models/loss.py:90-129).  config: the dataset config (default: ScanNet's) -- the proposal kernel computes the box
    terms in the same pass."""
    _lib.need_gpu(est_data['aggregated_vote_xyz'])
    dev = est_data['aggregated_vote_xyz'].device
    B, K = est_data['aggregated_vote_xyz'].shape[:2]
    if config is None:
        config = _default_config()
    partial = _partials(B, dev)
    label, mask, assignment = _proposal_partial(est_data, gt_data, config, partial)
    return _finish(B, K, 2, partial)[KEYS.index('objectness_loss')], label, mask, assignment


_DEFAULT_CONFIG = []


def _default_config():
    if not _DEFAULT_CONFIG:
        from .config import ScannetConfig
        _DEFAULT_CONFIG.append(ScannetConfig())
    return _DEFAULT_CONFIG[0]


@torch.no_grad()
def compute_box_and_sem_cls_loss(est_data, gt_data, meta_data, config):
    """-> center_loss, heading_cls_loss, heading_reg_loss, size_cls_loss, size_reg_loss, sem_cls_loss (0-d device
    tensors) at meta_data's object_assignment / objectness_label (models/loss.py:131-202)"""
    _lib.need_gpu(est_data['center'])
    dev = est_data['center'].device
    B, K = est_data['center'].shape[:2]
    partial = _partials(B, dev)
    _proposal_partial(est_data, gt_data, config, partial, meta_data)
    out = _finish(B, K, 2, partial)
    return tuple(out[KEYS.index(k)] for k in ('center_loss', 'heading_cls_loss', 'heading_reg_loss', 'size_cls_loss',
                                              'size_reg_loss', 'sem_cls_loss'))


@LOSSES.register_module
class BaseLoss(object):
    '''base loss class'''

    def __init__(self, weight=1):
        '''initialize loss module'''
        self.weight = weight


@LOSSES.register_module
class Null(BaseLoss):
    '''This loss function is for modules where a loss preliminary calculated.'''

    def __call__(self, loss):
        return self.weight * torch.mean(loss)


@LOSSES.register_module
class DetectionLoss(BaseLoss):
    @torch.no_grad()
    def __call__(self, est_data, gt_data, dataset_config):
        """-> the reference's dictionary: 'total' a 0-d device tensor, the twelve other keys Python floats"""
        _lib.need_gpu(est_data['seed_xyz'])
        dev = est_data['seed_xyz'].device
        B, K = est_data['aggregated_vote_xyz'].shape[:2]
        partial = _partials(B, dev)
        _vote_partial(est_data, gt_data, partial)
        _proposal_partial(est_data, gt_data, dataset_config, partial)
        out = _finish(B, K, 3, partial)
        values = out.tolist()                                   # the one device-to-host copy
        loss = {k: v for k, v in zip(KEYS, values)}
        loss['total'] = out[0]
        return loss


@LOSSES.register_module
class ONet_Loss(BaseLoss):
    def __call__(self, value):
        completion_loss = torch.mean(value[:, 0])
        mask_loss = torch.mean(value[:, 1])
        total_loss = self.weight * (completion_loss + 100 * mask_loss)
        return {'total_loss': total_loss,
                'completion_loss': completion_loss.item(),
                'mask_loss': mask_loss.item()}
