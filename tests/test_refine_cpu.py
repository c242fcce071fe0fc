"""CPU: mesh refinement (Generator3D.set_refinement / refine_meshes, csrc/mesh_refine.hip) -- the float64 closed-form
restatement (tests/refine_f64.py) against the fixture of the reference's refine_mesh (F_REF: its double-backward float64 run),
the host draw order, configuration and binding.  No kernel runs here."""
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_f64 import loss_f64, refine_f64  # noqa: E402
from seeded import reference_draws, seeded_onet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["rfd_refine_sample", "rfd_refine_face_backward", "rfd_refine_vertex_step", "rfd_refine_dirichlet"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    ref, gen = np.load(os.path.join(golden_dir, "F_REF.npz")), np.load(os.path.join(golden_dir, "F_GEN.npz"))
    onet = seeded_onet(gen, 202)
    sd = OrderedDict((k, v.detach().cpu().numpy()) for k, v in onet.decoder.state_dict().items())
    return ref, gen["codes"][int(ref["code_index"])], np.zeros(onet.z_dim, np.float32), sd


def test_closed_form_float64_reproduces_the_double_backward_fixture(fx):
    ref, code, z, sd = fx
    eps = reference_draws(ref["faces"].shape[0], 30, int(ref["seed"]))
    snaps = {5: None}
    v30, g1 = refine_f64(sd, ref["verts"], ref["faces"], z, code, eps, float(ref["threshold"]), return_grad=True,
                         snapshots=snaps)
    d5, d30 = np.abs(snaps[5] - ref["f64_5"]).max(), np.abs(v30 - ref["f64_30"]).max()
    dg = np.abs(g1 - ref["grad64"]).max() / np.abs(ref["grad64"]).max()
    print("closed form vs double backward: 5 steps %.1e, 30 steps %.1e, step-1 gradient %.1e relative" % (d5, d30, dg))
    assert d5 <= 1e-10 and d30 <= 1e-10
    assert dg <= 1e-12
    # the fixture's own bookkeeping: the loss it stores is the one this restatement evaluates, and 30 steps lower it
    after = loss_f64(sd, ref["f64_30"], ref["faces"], z, code, float(ref["threshold"]))
    assert abs(after - float(ref["loss64_after"])) <= 1e-9 * after
    assert float(ref["loss64_after"]) < float(ref["loss64_before"]) and float(ref["loss32_after"]) < float(ref["loss32_before"])


def test_host_draw_consumes_numpys_stream_in_the_references_order(fx):
    """two meshes refined in one call draw what the reference's per-object loop draws: mesh 0's steps, then mesh 1's"""
    from rfdnet_amd.iscnet.generator import draw_dirichlet
    ref, code, z, sd = fx
    faces = [ref["faces"][:37], ref["faces"][200:329]]
    steps = 3
    np.random.seed(11)
    batched = draw_dirichlet([37, 0, 129], steps)                    # an empty mesh between them draws nothing
    assert batched.shape == (steps, 166, 3) and batched.dtype == np.float32
    np.random.seed(11)
    sequential = [np.stack([np.random.dirichlet((0.5, 0.5, 0.5), size=n) for _ in range(steps)]).astype(np.float32)
                  for n in (37, 129)]
    tau = float(ref["threshold"])
    for k, (lo, hi) in enumerate(((0, 37), (37, 166))):
        assert np.array_equal(batched[:, lo:hi], sequential[k])
        a = refine_f64(sd, ref["verts"], faces[k], z, code, batched[:, lo:hi], tau)
        b = refine_f64(sd, ref["verts"], faces[k], z, code, sequential[k], tau)
        assert np.array_equal(a, b) and np.abs(a - ref["verts"]).max() > 1e-4


def test_config_enables_refinement_and_the_constructor_still_raises():
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.generator import Generator3D
    from rfdnet_amd.iscnet.occupancy_net import ONet
    g = ONet(Config({'generation': {'refinement_step': 5}})).generator
    assert g.refinement_step == 5 and g.refine_eps_source == 'numpy'
    assert ONet(Config({})).generator.refinement_step == 0
    with pytest.raises(NotImplementedError, match="set_refinement"):
        Generator3D(None, refinement_step=3)
    with pytest.raises(NotImplementedError):
        Generator3D(None, simplify_nfaces=1000)
    g = Generator3D(None)
    assert g.set_refinement(30, eps_source='device', seed=4) is g
    assert (g.refinement_step, g.refine_eps_source, g.refine_seed) == (30, 'device', 4)
    assert g.set_refinement(0).refinement_step == 0
    with pytest.raises(ValueError):
        g.set_refinement(-1)
    with pytest.raises(ValueError):
        g.set_refinement(3, eps_source='host')


def test_demo_refinement_flag_parses():
    sys.path.insert(0, ROOT)
    import demo
    assert demo.build_parser().parse_args(["--synthetic", "10", "--refinement_step", "30"]).refinement_step == 30
    assert demo.build_parser().parse_args([]).refinement_step is None


def test_entry_points_are_declared_bound_and_exported():
    import ctypes
    from rfdnet_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfd_occ.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.ABI and hasattr(lib, name), name
        n_params = len(re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S).group(1).split(","))
        assert len(_lib.ABI[name][1]) == n_params, name
    assert os.path.exists(os.path.join(ROOT, "rfdnet_amd", "csrc", "mesh_refine.hip"))


def test_a_stage_run_again_by_the_range_fallback_consumes_numpys_stream_once(monkeypatch):
    """ISCNet.complete: the second run of the completion (f16-range flag at the default scale) starts from the stream's
    state at the first run, so a seeded scene draws what the reference draws whether or not the fallback ran"""
    import contextlib
    import types
    from rfdnet_amd import _lib
    from rfdnet_amd.iscnet.network import ISCNet

    class Dec(object):
        ka = 6

        def lower_activation_scale(self):
            self.ka = 3
            return True

    def complete(statuses, source):
        draws = []

        def run(codes, cls):
            draws.append(np.random.dirichlet((0.5, 0.5, 0.5), size=4))
            return draws[-1]
        gen = types.SimpleNamespace(generate_mesh=run, generate_grids=run, refinement_step=3, refine_eps_source=source)
        net = types.SimpleNamespace(completion=types.SimpleNamespace(generator=gen, decoder=Dec()))
        seq = list(statuses)
        monkeypatch.setattr(_lib, "stream_status_bits", lambda: seq.pop(0))
        monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
        np.random.seed(5)
        out = ISCNet.complete(net, None, None, None)
        return out, draws, np.random.random()

    once, d1, next1 = complete([0], 'numpy')
    twice, d2, next2 = complete([2, 0], 'numpy')
    assert len(d1) == 1 and len(d2) == 2
    assert np.array_equal(once, twice) and np.array_equal(d2[0], d2[1]) and next1 == next2
    _, d3, _ = complete([2, 0], 'device')                    # nothing to protect: the stream is left alone
    assert not np.array_equal(d3[0], d3[1])
