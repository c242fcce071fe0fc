"""GPU (-m gpu): batched mesh refinement (Generator3D.refine_meshes, csrc/mesh_refine.hip + the decoder's value and gradient
kernels) against the float64 run of the reference's refine_mesh stored in F_REF (tests/golden/make_refine_fixture.py) and
the closed-form float64 restatement (tests/refine_f64.py).

Bounds, set against the reference's own fp32-vs-float64 scatter on the fixture mesh (ReLU-kink flips and RMSprop's sign-like
first steps):  5 steps: every coordinate within 2e-4 (reference fp32: 4.6e-5), at most 0.5 % beyond 1e-5 (0.06 %), mean
movement >= 1e-3 (2.6e-3);  30 steps: at most 1 % beyond 1e-4 (0.16 %), mean deviation <= 1e-5 (1.2e-6), loss at barycentre
weights within 10 % of the reference's;  first-step gradient: max deviation / max |grad| <= 4 x the reference fp32's."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from rfdnet_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_f64 import loss_f64, refine_f64  # noqa: E402
from seeded import reference_draws, seeded_onet  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    ref, gen = np.load(os.path.join(golden_dir, "F_REF.npz")), np.load(os.path.join(golden_dir, "F_GEN.npz"))
    onet = seeded_onet(gen, 202)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in onet.decoder.state_dict().items())
    return ref, gen, onet, sd


def run(onet, meshes, codes, steps, eps, return_grad=False):
    """meshes: [(verts (n,3), faces (m,3) local)], codes (K,C) -> refine_meshes' result(s) as numpy, split per mesh"""
    g = onet.generator
    vend = np.concatenate([[0], np.cumsum([m[0].shape[0] for m in meshes])]).tolist()
    tend = np.concatenate([[0], np.cumsum([m[1].shape[0] for m in meshes])]).tolist()
    v = torch.from_numpy(np.concatenate([np.asarray(m[0], np.float64).reshape(-1, 3) for m in meshes])).cuda()
    f = torch.from_numpy(np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in meshes])).cuda()
    with torch.no_grad():
        z = torch.zeros(len(meshes), onet.z_dim, device="cuda")
        fold = onet.decoder.fold(z, torch.as_tensor(np.asarray(codes, np.float32)).cuda())
        out = g.refine_meshes(v, f, vend, tend, fold, steps, eps=eps, return_grad=return_grad)
    outs = [o.cpu().numpy() for o in (out if return_grad else (out,))]
    split = [[o[vend[k]:vend[k + 1]] for k in range(len(meshes))] for o in outs]
    return split if return_grad else split[0]


def five_step_bounds(name, got, want, v0, referenced=None):
    d = np.abs(got.astype(np.float64) - want)
    moved = np.abs(want - v0)
    if referenced is not None:
        moved = moved[referenced]
    print("%s: max |dv| %.2e, %.3f %% beyond 1e-5, mean movement %.2e" % (name, d.max(), 100 * (d > 1e-5).mean(), moved.mean()))
    assert d.max() <= 2e-4
    assert (d > 1e-5).mean() <= 0.005
    assert np.abs(got - v0)[referenced if referenced is not None else slice(None)].mean() >= 1e-3


def test_first_step_gradient_against_float64(hip, fx):
    ref, gen, onet, sd = fx
    code = gen["codes"][int(ref["code_index"])]
    eps = reference_draws(ref["faces"].shape[0], 1, int(ref["seed"]))
    _, grad = run(onet, [(ref["verts"], ref["faces"])], code[None], 1, eps, return_grad=True)
    hip.device_status()
    scale = np.abs(ref["grad64"]).max()
    ours, theirs = np.abs(grad[0] - ref["grad64"]).max() / scale, np.abs(ref["grad32"] - ref["grad64"]).max() / scale
    print("first-step vertex gradient, max deviation / max |grad|: kernels %.2e, reference fp32 %.2e" % (ours, theirs))
    assert ours <= 4 * theirs


def test_five_and_thirty_steps_against_the_reference_fixture(hip, fx):
    ref, gen, onet, sd = fx
    code = gen["codes"][int(ref["code_index"])]
    eps = reference_draws(ref["faces"].shape[0], 30, int(ref["seed"]))
    mesh = [(ref["verts"], ref["faces"])]
    v0 = ref["verts"]
    five_step_bounds("5 steps", run(onet, mesh, code[None], 5, eps[:5])[0], ref["f64_5"], v0)
    got = run(onet, mesh, code[None], 30, eps)[0]
    hip.device_status()
    d = np.abs(got.astype(np.float64) - ref["f64_30"])
    loss = loss_f64(sd, got, ref["faces"], np.zeros(onet.z_dim, np.float32), code, float(ref["threshold"]))
    print("30 steps: %.3f %% beyond 1e-4, mean |dv| %.2e, max %.2e; loss at barycentre weights %.6e (reference fp32 %.6e, "
          "before %.6e)" % (100 * (d > 1e-4).mean(), d.mean(), d.max(), loss, float(ref["loss32_after"]),
                            float(ref["loss32_before"])))
    assert (d > 1e-4).mean() <= 0.01
    assert d.mean() <= 1e-5
    assert abs(loss - float(ref["loss32_after"])) <= 0.1 * float(ref["loss32_after"])


def compact(verts, faces):
    """the sub-mesh of `faces` with its own vertex numbering"""
    used, inv = np.unique(faces.reshape(-1), return_inverse=True)
    return verts[used], inv.reshape(-1, 3).astype(np.int32)


def ragged_meshes(ref):
    v, f = ref["verts"], ref["faces"]
    tri = compact(v, f[100:101])
    sliver_v, sliver_f = compact(v, f[2000:2040])
    sliver_f = np.concatenate([sliver_f, [[sliver_f[0, 0], sliver_f[0, 0], sliver_f[0, 1]]]]).astype(np.int32)   # (i, i, j)
    return [(v, f[:37]),                                                   # most vertices unreferenced
            (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),    # empty
            tri,                                                           # a single triangle
            compact(v, f[1000:1129]),                                      # 129 faces: two decoder tiles, nine 16-groups
            (sliver_v, sliver_f)]                                          # a zero-area face


def test_ragged_batch_equals_single_meshes_and_float64(hip, fx):
    ref, gen, onet, sd = fx
    meshes = ragged_meshes(ref)
    c = gen["codes"]
    codes = np.stack([c[0], c[1], c[2], c[0][::-1], 0.5 * (c[1] + c[2])]).astype(np.float32)      # five distinct codes
    steps = 3
    counts = [m[1].shape[0] for m in meshes]
    eps = np.random.default_rng(5).dirichlet((0.5, 0.5, 0.5), size=(steps, sum(counts))).astype(np.float32)
    at = np.concatenate([[0], np.cumsum(counts)])
    batch = run(onet, meshes, codes, steps, eps)
    again = run(onet, meshes, codes, steps, eps)
    hip.device_status()
    z = np.zeros(onet.z_dim, np.float32)
    for k, (mv, mf) in enumerate(meshes):
        assert batch[k].shape == mv.shape and np.isfinite(batch[k]).all()
        assert np.array_equal(batch[k], again[k])
        if mf.shape[0] == 0:
            continue
        e = eps[:, at[k]:at[k + 1]]
        single = run(onet, [(mv, mf)], codes[k:k + 1], steps, e)[0]
        assert np.array_equal(batch[k], single), k
        used = np.zeros(mv.shape[0], bool)
        used[mf.reshape(-1)] = True
        assert np.array_equal(batch[k][~used], mv[~used])                  # bit-unchanged
        want = refine_f64(sd, mv, mf, z, codes[k], e, float(ref["threshold"]))
        five_step_bounds("ragged mesh %d (%d faces)" % (k, mf.shape[0]), batch[k], want, mv, used)
    assert (~np.isin(np.arange(meshes[0][0].shape[0]), meshes[0][1])).sum() > 6000
    hip.device_status()


def test_device_weights_are_dirichlet_half(hip, fx):
    g = fx[2].generator
    a = g.device_weights(30000, 123, 0, "cuda").cpu().numpy().astype(np.float64)
    assert (a >= 0).all() and np.abs(a.sum(1) - 1).max() <= 1e-6
    print("device Dirichlet: means %s, variances %s" % (a.mean(0), a.var(0)))
    assert np.abs(a.mean(0) - 1 / 3).max() <= 0.01
    assert np.abs(a.var(0) - 0.0889).max() <= 0.005
    assert np.array_equal(a, g.device_weights(30000, 123, 0, "cuda").cpu().numpy())
    assert not np.array_equal(a, g.device_weights(30000, 124, 0, "cuda").cpu().numpy())
    assert not np.array_equal(a, g.device_weights(30000, 123, 1, "cuda").cpu().numpy())
    # and the source drives the loop: same seed, same vertices
    ref, gen, onet, _ = fx
    g.set_refinement(2, eps_source='device', seed=9)
    try:
        one = run(onet, [(ref["verts"], ref["faces"][:300])], gen["codes"][:1], 2, None)[0]
        two = run(onet, [(ref["verts"], ref["faces"][:300])], gen["codes"][:1], 2, None)[0]
    finally:
        g.set_refinement(0)
    hip.device_status()
    assert np.array_equal(one, two) and np.abs(one - ref["verts"]).max() > 1e-4


def test_refine_mesh_single_entry_point_and_unsupported_modes(hip, fx):
    """the reference-shaped call: numpy mesh in, numpy vertices out, the numpy stream consumed as the reference consumes it"""
    from rfdnet_amd.iscnet.generator import Mesh
    ref, gen, onet, sd = fx
    g = onet.generator
    code = gen["codes"][int(ref["code_index"])]
    mv, mf = compact(ref["verts"], ref["faces"][500:900])
    g.set_refinement(5)
    try:
        np.random.seed(3)
        mesh = g.refine_mesh(Mesh(mv.astype(np.float64), mf), None, torch.zeros(onet.z_dim), torch.from_numpy(code).cuda())
        hip.device_status()
        assert isinstance(mesh.vertices, np.ndarray) and mesh.vertices.dtype == np.float32
        want = refine_f64(sd, mv, mf, np.zeros(onet.z_dim, np.float32), code, reference_draws(mf.shape[0], 5, 3),
                          float(ref["threshold"]))
        five_step_bounds("refine_mesh", mesh.vertices, want, mv)
        dec = onet.decoder
        dec.mode = 1
        with pytest.raises(NotImplementedError):
            g.refine_mesh(Mesh(mv, mf), None, torch.zeros(onet.z_dim), torch.from_numpy(code).cuda())
        dec.mode = 3
        # the four-wave kernel's weight stream is not the one the gradient kernel reads
        v, f = torch.from_numpy(mv).cuda(), torch.from_numpy(mf).cuda()
        with torch.no_grad():
            fold = dec.fold(torch.zeros(1, onet.z_dim, device="cuda"), torch.from_numpy(code).cuda()[None])
        dec.kernel = "w4"
        with pytest.raises(NotImplementedError):
            g.refine_meshes(v, f, [0, v.shape[0]], [0, f.shape[0]], fold, 2)
        dec.kernel = "w8"
        with pytest.raises(ValueError, match="code c"):
            g.refine_mesh(Mesh(mv, mf), None, torch.zeros(onet.z_dim))
        with pytest.raises(ValueError, match="code c"):
            g.extract_mesh(np.zeros((9, 9, 9), np.float32))
    finally:
        onet.decoder.mode, onet.decoder.kernel = 3, "w8"
        g.set_refinement(0)


def test_iscnet_generate_with_refinement(hip):
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    cfg = Config({'data': {'num_point': 4096}, 'generation': {'resolution_0': 16, 'upsampling_steps': 1,
                                                              'refinement_step': 3, 'with_normals': True}})
    net = ISCNet(cfg)
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    gen = net.completion.generator
    assert gen.refinement_step == 3
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=21, n_raw=6000, n_points=4096)[None]).cuda()
    with torch.no_grad():
        np.random.seed(1)
        _, ids, refined = net.generate({'point_clouds': pc}, selection='all')
        hip.device_status()                                          # the status word is clean
        gen.set_refinement(0)
        _, ids0, plain = net.generate({'point_clouds': pc}, selection='all')
        hip.device_status()
        # refinement without normals: the same vertices from the same draws, no normals
        gen.with_normals = False
        gen.set_refinement(3)
        np.random.seed(1)
        _, ids1, bare = net.generate({'point_clouds': pc}, selection='all')
        hip.device_status()
    assert torch.equal(ids, ids1) and len(bare) == len(refined)
    for r, b in zip(refined, bare):
        assert b.vertex_normals is None and torch.equal(r.vertices, b.vertices) and torch.equal(r.faces, b.faces)
    assert torch.equal(ids, ids0) and len(refined) == len(plain) > 0
    moved = 0
    for r, p in zip(refined, plain):
        assert torch.equal(r.faces, p.faces) and r.vertices.shape == p.vertices.shape
        assert r.vertices.dtype == torch.float32 and torch.isfinite(r.vertices).all()
        if p.vertices.shape[0] == 0:
            continue
        assert torch.equal(r.vertex_normals, p.vertex_normals)      # taken before the refinement (generator.py:173-195)
        d = (r.vertices.double() - p.vertices.double()).abs()
        assert d.max().item() <= 3e-3 + 1e-6                            # three RMSprop steps: at most 1e-3 + 0.71e-3 + 0.58e-3
        moved += int((d > 1e-4).sum())
    assert moved > 0
