"""CPU: iscnet/box_util.py is the one definition of the box geometry -- the prediction decoder and the ground-truth parser
go through the same functions and give the same bits for the same boxes."""
import types

import numpy as np
import torch

from rfdnet_amd.iscnet import box_util, evaluation, fit, predictions


def boxes(seed=0):
    g = torch.Generator().manual_seed(seed)
    center = torch.randn(2, 5, 3, generator=g, dtype=torch.float64)
    size = torch.rand(2, 5, 3, generator=g, dtype=torch.float64) + 0.3
    angle = (torch.rand(2, 5, generator=g, dtype=torch.float64) - 0.5) * 6.0
    return center, size, angle


def test_box_corners_upright_camera_is_get_3d_box_of_the_flipped_centre():
    center, size, angle = boxes()
    want = box_util.get_3d_box(size, -angle, box_util.flip_axis_to_camera(center))
    assert torch.equal(box_util.box_corners_upright_camera(center, size, angle), want)
    # the names the other modules are used under are these functions
    assert predictions.box_corners_upright_camera is box_util.box_corners_upright_camera
    assert fit.get_3d_box is box_util.get_3d_box and fit.flip_axis_to_camera is box_util.flip_axis_to_camera
    assert fit.flip_axis_to_depth is box_util.flip_axis_to_depth
    assert fit.box_params_from_corners is box_util.box_params_from_corners


def test_decoder_and_groundtruth_parser_decode_the_same_boxes_bitwise():
    """2 x 5 boxes given once as head outputs (scores whose argmax is the class, normalised residuals) and once as
    labels (the class, the fp32 residual the decoder derives): angle, size and corners are the same bits.  Classes
    7 .. 11 of 12 bins lie above pi and take the wrap."""
    B, K, NH, NS = 2, 5, 12, 4
    rng = np.random.default_rng(4)
    cfg = types.SimpleNamespace(num_heading_bin=NH, mean_size_arr=rng.uniform(0.3, 2.0, (NS, 3)))
    heading_class = torch.tensor([[0, 3, 6, 7, 11], [5, 6, 9, 1, 10]])
    size_class = torch.from_numpy(rng.integers(0, NS, (B, K)))
    one_hot = lambda cls, n: torch.nn.functional.one_hot(cls, n).float() * 3 - 1
    end_points = {'center': torch.from_numpy(rng.normal(0, 1, (B, K, 3)).astype(np.float32)),
                  'heading_scores': one_hot(heading_class, NH), 'size_scores': one_hot(size_class, NS),
                  'heading_residuals_normalized': torch.from_numpy(rng.uniform(-1, 1, (B, K, NH)).astype(np.float32)),
                  'size_residuals_normalized': torch.from_numpy(rng.uniform(-0.3, 0.3, (B, K, NS, 3)).astype(np.float32))}
    center, size, angle = predictions.decode_boxes(end_points, cfg)
    assert center.dtype == size.dtype == angle.dtype == torch.float64

    heading_residual = torch.gather(end_points['heading_residuals_normalized'] * (np.pi / NH), 2,
                                    heading_class.unsqueeze(-1)).squeeze(2)
    mean_f32 = torch.from_numpy(cfg.mean_size_arr).float()
    size_residual = torch.gather(end_points['size_residuals_normalized'] * mean_f32, 2,
                                 size_class.view(B, K, 1, 1).expand(-1, -1, 1, 3)).squeeze(2)
    raw = heading_class.double() * (2 * np.pi / NH) + heading_residual.double()
    assert int((raw > np.pi).sum()) >= 3 and int((raw <= np.pi).sum()) >= 3
    assert torch.equal(angle, box_util.class2angle(heading_class, heading_residual, NH))
    assert torch.equal(angle, torch.where(raw > np.pi, raw - 2 * np.pi, raw)) and float(angle.max()) <= np.pi
    assert torch.equal(size, box_util.class2size(size_class, size_residual, cfg.mean_size_arr))
    assert torch.equal(size, torch.from_numpy(cfg.mean_size_arr)[size_class] + size_residual.double())

    gts = evaluation.parse_groundtruths(
        {'center_label': end_points['center'], 'heading_class_label': heading_class, 'heading_residual_label': heading_residual,
         'size_class_label': size_class, 'size_residual_label': size_residual,
         'sem_cls_label': torch.zeros(B, K, dtype=torch.int64), 'box_label_mask': torch.ones(B, K)}, cfg)
    # the parser returns corners only: they are the decoder's corners, so its angle and size were the decoder's
    assert torch.equal(gts['gt_corners_3d_upright_camera'], predictions.box_corners_upright_camera(center, size, angle))
