"""Oriented-box geometry of the test-mode path, defined once (net_utils/box_util.py, net_utils/libs.py,
configs/scannet_config.py): the frame flips, the corner order, the class / residual decoding in float64.  Batched tensor
code, any device; predictions.py, evaluation.py and fit.py import these names.
(ScannetConfig.class2angle_cuda, the float32 formula object_codes uses, is another function and lives with the config.)"""
import numpy as np
import torch

from .. import _lib


def flip_axis_to_depth(p):
    """cam (x, y, z) -> depth (x, z, -y)  (net_utils/libs.py:116-120)."""
    return torch.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)


def flip_axis_to_camera(p):
    """depth (x, y, z) -> cam (x, -z, y)  (net_utils/libs.py:98-105)."""
    return torch.stack([p[..., 0], -p[..., 2], p[..., 1]], -1)


def get_3d_box(size, heading, center):
    """size (...,3) [l,w,h], heading (...), center (...,3) -> corners (...,8,3)
    (net_utils/box_util.py:183-198; roty(t) = [[c,0,s],[0,1,0],[-s,0,c]])."""
    dt, dev = size.dtype, size.device
    sx = torch.tensor([1, 1, -1, -1, 1, 1, -1, -1], dtype=dt, device=dev)
    sy = torch.tensor([1, 1, 1, 1, -1, -1, -1, -1], dtype=dt, device=dev)
    sz = torch.tensor([1, -1, -1, 1, 1, -1, -1, 1], dtype=dt, device=dev)
    xc = size[..., 0:1] / 2 * sx
    yc = size[..., 2:3] / 2 * sy
    zc = size[..., 1:2] / 2 * sz
    c, s = torch.cos(heading).unsqueeze(-1), torch.sin(heading).unsqueeze(-1)
    x = c * xc + s * zc
    z = -s * xc + c * zc
    return torch.stack([x + center[..., 0:1], yc + center[..., 1:2], z + center[..., 2:3]], -1)


def box_corners_upright_camera(center, size, angle):
    """depth-frame centre (...,3), size (...,3) [l,w,h], heading angle (...) -> the box's corners in the upright camera
    frame (...,8,3), as parse_predictions and parse_groundtruths build them (ap_helper.py:176-181, :352-356)."""
    return get_3d_box(size, -angle, flip_axis_to_camera(center))


def box_params_from_corners(corners_cam):
    """(P,8,3) upright-camera corners -> centroid (P,3), sizes (P,3), orientation (P), depth
    frame (network.py:220-229)."""
    d = flip_axis_to_depth(corners_cam)
    centroid = (d.max(dim=1)[0] + d.min(dim=1)[0]) / 2.
    fwd, left, up = d[:, 1] - d[:, 2], d[:, 0] - d[:, 1], d[:, 6] - d[:, 2]
    orientation = torch.atan2(fwd[:, 1], fwd[:, 0])
    sizes = torch.stack([fwd.norm(dim=1), left.norm(dim=1), up.norm(dim=1)], 1)
    return centroid, sizes, orientation


def class2angle(cls, residual, num_heading_bin):
    """heading class and residual -> angle in (-pi, pi], float64 as the reference's numpy scalars
    (scannet_config.py:43-53)."""
    angle = cls.double() * (2 * np.pi / float(num_heading_bin)) + residual.double()
    return torch.where(angle > np.pi, angle - 2 * np.pi, angle)


def class2size(cls, residual, mean_size_arr):
    """size class (...) and residual (...,3) -> size (...,3) float64 (scannet_config.py:71-73); mean_size_arr: numpy
    or a tensor."""
    return _lib.as_tensor(mean_size_arr, residual.device, torch.float64)[cls.long()] + residual.double()
