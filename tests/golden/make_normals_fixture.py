"""Generate tests/golden/F_NRM.npz (DEV CONTAINER ONLY): the reference's Generator3D.estimate_normals
(generator.py:200-224, torch CPU fp32 autograd through its ONet.decode) on the meshes of F_GEN's `mise16x1` grids.

Same recipe as make_fixtures.py (whose mount_reference it imports): the F_GEN ONet with seed-202 weights and F_GEN's
codes; vertices from the CPU oracle's marching cubes of the padded grids with the generator's affine (generator.py:157-168).
Stored: the vertices (f64), the per-mesh vertex bounds and the reference normals.  Weights are regenerated from the seed
by the tests.

Usage:  python tests/golden/make_normals_fixture.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402
from make_fixtures import mount_reference, ns  # noqa: E402


def main():
    import torch
    from oracle import oracle
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.config import Config
    mount_reference()
    ns('external.libmise').MISE = None
    ns('models.registers')
    reg = importlib.import_module('net_utils.registry')
    sys.modules['models.registers'].MODULES = reg.Registry('module')
    sys.modules['models.registers'].METHODS = reg.Registry('method')
    sys.modules['models.registers'].LOSSES = reg.Registry('loss')
    onet_mod = importlib.import_module('models.iscnet.modules.occupancy_net')
    gen = np.load(os.path.join(HERE, "F_GEN.npz"))
    codes, grids = gen["codes"], gen["mise16x1_grid"]
    cfg = Config({'generation': {'resolution_0': 16, 'upsampling_steps': 1}})
    onet = onet_mod.ONet(cfg)
    synthetic.load_seeded(onet, 202)
    onet.eval()
    g3d = onet.generator
    thr = float(np.log(g3d.threshold) - np.log(1. - g3d.threshold))
    box = 1 + g3d.padding
    verts, vend, normals = [], [0], []
    z = onet.get_z_from_prior((1,), sample=False, device='cpu')[0]
    for k in range(grids.shape[0]):
        occ = grids[k].astype(np.float64)
        n = occ.shape[0]
        v, _ = oracle.marching_cubes(np.pad(occ, 1, 'constant', constant_values=-1e6), thr)
        v = v - 0.5                                          # generator.py:163-168
        v = v - 1
        v = v / np.array([n - 1, n - 1, n - 1])
        v = box * (v - 0.5)
        nrm = g3d.estimate_normals(v, z, torch.from_numpy(codes[k]), device='cpu')
        verts.append(v)
        normals.append(nrm.astype(np.float32))
        vend.append(vend[-1] + v.shape[0])
        print("F_NRM mesh %d: %d vertices" % (k, v.shape[0]))
    np.savez_compressed(os.path.join(HERE, "F_NRM.npz"), verts=np.concatenate(verts), vend=np.array(vend, np.int64),
                        normals=np.concatenate(normals), codes=codes, seed=202)


if __name__ == "__main__":
    assert mf.REF
    main()
