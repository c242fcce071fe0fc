"""float64 composition of one set-abstraction layer after its ball query (PointnetSAModuleVotes.forward,
pointnet2_modules.py:219-255): the ground truth csrc/sa_fused.hip is held to.  The grouped (3 + C, npoint, nsample)
tensor comes from the module's own fp32 grouper -- pinned bit-exact against the reference's group / subtract / divide /
cat by test_group_concat_equals_reference_composition -- so the float64 result starts from the very input rounding the
kernel sees; everything after it (three 1x1 convolutions with eval-mode BatchNorm and ReLU, the max over the
neighbours) runs in float64 through a deep copy of the module's shared MLP."""
import copy

import torch


@torch.no_grad()
def sa_layer_f64(mod, xyz, new_xyz, features):
    """mod: PointnetSAModuleVotes (eval); xyz (B,N,3), new_xyz (B,npoint,3), features (B,C,N) ->
    (float64 result (B,C3,npoint), the fp32 torch composition of the same layer on the same grouped tensor)"""
    grouped, _ = mod.grouper(xyz, new_xyz, features)
    ref32 = mod.mlp_module(grouped).max(dim=3)[0]
    mlp64 = copy.deepcopy(mod.mlp_module).double()
    want = mlp64(grouped.double()).max(dim=3)[0]
    return want, ref32
