"""Generate tests/golden/F_REF.npz (DEV CONTAINER ONLY): the reference's Generator3D.refine_mesh (generator.py:226-289,
torch CPU fp32, double backward through its ONet.decode) on mesh 0 of F_GEN's `mise16x1` grids, for 5 and for 30 steps.

Same recipe as make_normals_fixture.py: the F_GEN ONet with seed-202 weights and F_GEN's codes; vertices and faces from the
CPU oracle's marching cubes with the generator's affine (generator.py:157-168).  np.random.seed(SEED) in front of every run:
the reference draws its barycentric weights from numpy's global stream, one Dirichlet call per step.

Beside the reference's fp32 results the file holds a float64 run of the same loop on the same draws (autograd with
create_graph, i.e. nothing closed-form: the ground truth tests/refine_f64.py is checked against), the first step's vertex
gradient in both precisions and the loss at barycentre weights before and after the 30 steps.  The draws are not stored: the
legacy numpy stream regenerates them (draws()).

Usage:  python tests/golden/make_refine_fixture.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
from make_fixtures import mount_reference, ns  # noqa: E402

SEED = 7


def draws(n_faces, steps, seed=SEED):
    """the weights the reference draws in `steps` steps after np.random.seed(seed), as it uploads them (FloatTensor)"""
    np.random.seed(seed)
    return np.stack([np.random.dirichlet((0.5, 0.5, 0.5), size=n_faces) for _ in range(steps)]).astype(np.float32)


def autograd_loop(decode, v0, faces, eps, tau, dtype):
    """the loop of generator.py:251-285 in `dtype` with given weights: decode(q (F,3)) -> logits (F,).
    -> vertices after the last step, the first step's gradient, the first step's loss"""
    import torch
    v = torch.nn.Parameter(torch.as_tensor(np.array(v0)).to(dtype))      # np.array: a copy, the optimiser works in place
    faces = torch.as_tensor(np.asarray(faces, np.int64))
    opt = torch.optim.RMSprop([v], lr=1e-4)
    first = loss0 = None
    for e in eps:
        opt.zero_grad()
        fv = v[faces]
        q = (fv * torch.as_tensor(e).to(dtype)[:, :, None]).sum(dim=1)
        nf = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1], dim=1)
        nf = nf / (nf.norm(dim=1, keepdim=True) + 1e-10)
        s = torch.sigmoid(decode(q))
        nt = -torch.autograd.grad([s.sum()], [q], create_graph=True)[0]
        nt = nt / (nt.norm(dim=1, keepdim=True) + 1e-10)
        loss = (s - tau).pow(2).mean() + 0.01 * (nf - nt).pow(2).sum(dim=1).mean()
        loss.backward()
        if first is None:
            first, loss0 = v.grad.detach().numpy().copy(), float(loss.detach())
        opt.step()
    return v.detach().numpy(), first, loss0


def main():
    import torch
    from oracle import oracle
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.config import Config
    from normals_f64 import decoder_torch
    from refine_f64 import refine_f64
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
    onet = onet_mod.ONet(Config({'generation': {'resolution_0': 16, 'upsampling_steps': 1}}))
    synthetic.load_seeded(onet, 202)
    onet.eval()
    g3d = onet.generator
    thr = float(np.log(g3d.threshold) - np.log(1. - g3d.threshold))
    box = 1 + g3d.padding
    occ = grids[0].astype(np.float64)
    n = occ.shape[0]
    v, f = oracle.marching_cubes(np.pad(occ, 1, 'constant', constant_values=-1e6), thr)
    v = box * ((v - 0.5 - 1) / np.array([n - 1, n - 1, n - 1]) - 0.5)            # generator.py:163-168
    v32 = v.astype(np.float32)
    f = np.asarray(f, np.int32)
    print("F_REF: %d vertices, %d faces" % (v.shape[0], f.shape[0]))
    z = onet.get_z_from_prior((1,), sample=False, device='cpu')[0]
    c = torch.from_numpy(codes[0])
    tau = float(g3d.threshold)
    sd = {k: t.detach().numpy() for k, t in onet.decoder.state_dict().items()}
    z64, c64 = z.double(), c.double()
    dec32 = lambda q: onet.decode(q.unsqueeze(0), z.unsqueeze(0), c.unsqueeze(0)).logits[0]
    dec64 = lambda q: decoder_torch(sd, q[None], z64[None], c64[None])[0]
    bary = np.full((1, f.shape[0], 3), 1.0 / 3, np.float32)
    out = {"verts": v32, "faces": f, "seed": SEED, "code_index": 0, "threshold": tau}
    for steps in (5, 30):
        class M(object):
            vertices, faces = v.copy(), f.astype(np.int64)
        g3d.refinement_step = steps
        np.random.seed(SEED)
        ref = g3d.refine_mesh(M, occ, z.unsqueeze(0), c.unsqueeze(0), device='cpu').vertices
        eps = draws(f.shape[0], steps)
        mine32, g32, _ = autograd_loop(dec32, v32, f, eps, tau, torch.float32)
        f64, g64, _ = autograd_loop(dec64, v32, f, eps, tau, torch.float64)
        closed, gc = refine_f64(sd, v32, f, z.numpy(), codes[0], eps, tau, return_grad=True)
        print("%2d steps: restated loop vs refine_mesh (fp32) %.1e; closed form vs double backward (f64) %.1e, step-1 "
              "gradient %.1e relative; refine_mesh vs f64 max %.1e mean %.1e, > 1e-5: %.3f %%, > 1e-4: %.3f %%; mean "
              "movement %.1e" % (steps, np.abs(mine32 - ref).max(), np.abs(closed - f64).max(),
                                 np.abs(gc - g64).max() / np.abs(g64).max(), np.abs(ref - f64).max(),
                                 np.abs(ref - f64).mean(), 100 * (np.abs(ref - f64) > 1e-5).mean(),
                                 100 * (np.abs(ref - f64) > 1e-4).mean(), np.abs(f64 - v32).mean()))
        out["ref32_%d" % steps] = ref.astype(np.float32)
        out["f64_%d" % steps] = f64
        if steps == 5:
            out["grad32"], out["grad64"] = g32, g64
    out["loss32_before"] = autograd_loop(dec32, v32, f, bary, tau, torch.float32)[2]
    out["loss64_before"] = autograd_loop(dec64, v32, f, bary, tau, torch.float64)[2]
    out["loss32_after"] = autograd_loop(dec32, out["ref32_30"], f, bary, tau, torch.float32)[2]
    out["loss64_after"] = autograd_loop(dec64, out["f64_30"], f, bary, tau, torch.float64)[2]
    print("loss at barycentre weights: fp32 %.6e -> %.6e, f64 %.6e -> %.6e"
          % (out["loss32_before"], out["loss32_after"], out["loss64_before"], out["loss64_after"]))
    path = os.path.join(HERE, "F_REF.npz")
    np.savez_compressed(path, **out)
    print("F_REF.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    assert mf.REF
    main()
