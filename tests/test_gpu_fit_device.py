"""GPU: fit_mesh_to_scan's device method (csrc/fit_pose.hip, include/rfd_fit.h; fit.prepare_fit / run_fit / finish_fit)
against the reference's own run (tests/golden/F_FIT.npz) and against the float64 histories of the ragged restatement
tests/fit_f64.py (tests/golden/F_FITD.npz), its repeatability, its freedom from host round trips, and ISCNet.evaluate.

Bounds (the convention of tests/test_gpu_loss.py).  At every iteration the loss and every parameter lie within
max(8 x dev32, 64 * 2^-24 * |value|) of the float64 history, dev32 being the deviation of the restatement's own fp32
variant from float64 at that iteration: the kernel's per-point terms are that variant's, its sums are f64.  The final
corners keep the project's 5e-3 against the reference's run."""
import os

import numpy as np
import pytest
import torch

from rfdnet_amd import synthetic
from rfdnet_amd.iscnet import fit

from test_fit_device_cpu import f_fit_inputs

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
RAGGED = ("one", "three", "pad9999", "pad10000", "centre")


@pytest.fixture(scope="module")
def fxd(golden_dir):
    return np.load(os.path.join(golden_dir, "F_FITD.npz"))


@pytest.fixture(scope="module")
def f_fit_problem(golden_dir, hip):
    """F_FIT's problem, prepared once on the GPU (nothing modifies it: run_fit works on a copy of params0)"""
    fx, args = f_fit_inputs(golden_dir, "cuda")
    return fx, args, fit.prepare_fit(*args)


def check_history(tag, res, fxd, key):
    """device loss / parameters at every iteration against the float64 history -> the largest |difference| / bound"""
    worst = 0.0
    for name, got in (("loss", res['hist_loss']), ("params", res['hist_params'])):
        got = got.cpu().numpy().astype(np.float64)
        f64, f32 = fxd["%s_f64_%s" % (key, name)], fxd["%s_f32_%s" % (key, name)].astype(np.float64)
        assert got.shape == f64.shape
        bound = np.maximum(8 * np.abs(f32 - f64), 64 * ULP * np.abs(f64))
        err = np.abs(got - f64)
        at = np.unravel_index(np.argmax(err / bound), err.shape)
        print("%s %-6s over %d iterations: largest |device - f64| %.2e; nearest the bound at %s: %.2e of %.2e "
              "(fp32 variant there %.2e)" % (tag, name, len(f64), err.max(), at, err[at], bound[at], abs(f32[at] - f64[at])))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (tag, name, at, err[at], bound[at])
    return worst


# ------------------------------------------------------------------------------------------------------- 6. F_FIT
def test_f_fit_through_the_device_method(hip, golden_dir, fxd):
    """Measured on the MI355X: final corners 3.6e-4 / 5.0e-4 from the reference's run (the float64 restatement: 4.1e-4 /
    5.0e-4); |device - f64| is the fp32 variant's own deviation at every iteration (nearest the bound: loss 3.2e-8 of
    2.6e-7 at iteration 31, a parameter 4.7e-6 of 3.7e-5 at iteration 76; largest 6.8e-7 and 2.1e-4, late in the flat
    valley); best iteration 97 on both sides, loss 0.0655324."""
    fx, args = f_fit_inputs(golden_dir, "cuda")
    out = fit.fit_mesh_to_scan(*args, method='device', history=True)
    K = int(fx["n_meshes"])
    got, want = out['pred_corners_3d_upright_camera'].cpu().numpy(), fx["corners_out"]
    err = np.abs(got - want).reshape(K, -1).max(1)
    print("final corners vs the reference's run: %s (float64 restatement: %s)"
          % (err, np.abs(fxd["fit_f64_corners"] - want[0, :2]).reshape(2, -1).max(1)))
    assert err.max() < 5e-3, err
    assert np.array_equal(got[0, 2], fx["corners_in"][0, 2])                 # the masked proposal is untouched
    assert out['fit_indices'] == [(0, 0), (0, 1)]
    hist = out['fit_history']
    check_history("F_FIT", {'hist_loss': hist['loss'], 'hist_params': hist['params']}, fxd, "fit")
    loss = hist['loss'].cpu().numpy()
    assert loss.shape == (100,) and loss.dtype == np.float32
    best = hist['best_iter']
    assert best == int(np.argmin(loss))                                      # argmin: the FIRST minimum
    assert out['fit_loss'] == float(loss[best])
    ref_best, ref_loss = int(fxd["fit_f64_best_iter"]), fxd["fit_f64_loss"]
    print("best iteration %d, loss %.7f (restatement: %d, %.7f)" % (best, loss[best], ref_best, ref_loss[ref_best]))
    if best != ref_best:                                                     # a flat valley: the two are a tie there
        assert abs(ref_loss[best] - ref_loss[ref_best]) <= 64 * ULP * ref_loss[ref_best]


# ------------------------------------------------------------------------------------------------- 7. ragged edges
def fixture_problem(fxd, name, points_per_thread):
    t = lambda k: torch.from_numpy(fxd["%s_%s" % (name, k)]).cuda()
    return fit.ragged_problem(t("obj"), fxd[name + "_obj_off"], t("scan"), fxd[name + "_scan_off"], t("params0"),
                              float(fxd[name + "_loss_scale"]), points_per_thread)


@pytest.mark.parametrize("name", RAGGED)
def test_ragged_edges(hip, fxd, name):
    """P = 1 and 3; 5, 255, 257, 1025 and 4097 scan points; 1, 1023, 1024, 1025 vertices, 9 999 (the extra zero row is row
    9 999) and 10 000 (no extra row); `centre`: every scan point is nearest the extra row.  Ten steps, each against the
    float64 history, with one and with four points per thread.

    The two instantiations are compared within 2^-24 relative, not bit for bit: their per-point terms are the same, but a
    tile is 256 points in one (one per thread, then the tree) and 1024 in the other (a thread adds its four, then the
    tree), so the f64 sums associate differently and a gradient can round to the neighbouring fp32 value."""
    runs = {}
    for ppt in (1, 4):
        pb = fixture_problem(fxd, name, ppt)
        n_vertices = np.diff(fxd[name + "_obj_off"])
        assert pb.points_per_thread == ppt and pb.tile_obj.shape[0] == sum(-(-n // (256 * ppt)) for n in pb.n_scan_points)
        res = fit.run_fit(pb, iterations=10, history=True)
        check_history("%s, %d per thread" % (name, ppt), res, fxd, name)
        runs[ppt] = {k: res[k].cpu().numpy() for k in ('hist_loss', 'hist_params', 'best_params', 'best_loss', 'best_iter',
                                                       'params')}
        loss = runs[ppt]['hist_loss']
        assert int(runs[ppt]['best_iter'][0]) == int(np.argmin(loss)) and runs[ppt]['best_loss'][0] == loss.min()
        np.testing.assert_array_equal(runs[ppt]['best_params'], runs[ppt]['hist_params'][int(np.argmin(loss))])
        if name == "centre":                                                 # q = 0 for every point: the heading never moves
            start = fxd["centre_params0"][0, 3]
            assert (runs[ppt]['hist_params'][:, 0, 3] == start).all() and runs[ppt]['params'][0, 3] == start
            assert (runs[ppt]['hist_params'][-1, 0, :3] != fxd["centre_params0"][0, :3]).all()
        if name == "pad9999":
            assert n_vertices[0] == 10000 and (fxd["pad9999_obj"][9999] == 0).all()
        if name == "pad10000":
            assert n_vertices[0] == 10000 and (fxd["pad10000_obj"][9999] != 0).all()
    same = all(np.array_equal(runs[1][k], runs[4][k]) for k in runs[1])
    print("%s: one and four points per thread are %s" % (name, "bitwise equal" if same else "equal within 2^-24 relative"))
    for k in ('hist_loss', 'hist_params', 'best_params', 'best_loss', 'params'):
        a, b = runs[1][k].astype(np.float64), runs[4][k].astype(np.float64)
        assert (np.abs(a - b) <= ULP * np.abs(a)).all(), k
    assert runs[1]['best_iter'][0] == runs[4]['best_iter'][0] or not same


# --------------------------------------------------------------------------------------------------- 8. determinism
def test_two_runs_are_bitwise_equal(hip, f_fit_problem):
    _, _, pb = f_fit_problem
    a = fit.run_fit(pb, history=True)
    b = fit.run_fit(pb, history=True)
    assert a is not b and pb.result is b
    for k in ('params', 'best_params', 'best_loss', 'best_iter', 'hist_loss', 'hist_params'):
        assert a[k].data_ptr() != b[k].data_ptr() and torch.equal(a[k], b[k]), k
    assert float(a['hist_loss'][-1]) < 0.3 * float(a['hist_loss'][0])


# ---------------------------------------------------------------------------------------------- 9. no host round trip
def test_run_fit_never_waits_for_the_device(hip, f_fit_problem):
    _, _, pb = f_fit_problem
    fit.run_fit(pb)                                                          # the library is loaded, the allocator warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = fit.run_fit(pb, history=True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert int(res['best_iter']) >= 0 and hip.stream_status_bits() == 0


def test_launcher_checks_its_arguments(hip, f_fit_problem):
    _, _, pb = f_fit_problem
    for change in (dict(points_per_thread=2), dict(loss_scale=float("nan"))):
        bad = fit.FitProblem(**dict(pb.__dict__, **change))
        with pytest.raises(hip.RfdHipError, match="rfd_fit_pose_run"):
            fit.run_fit(bad, iterations=2)
    for iterations in (0, 100001):
        with pytest.raises(hip.RfdHipError, match="iterations"):
            fit.run_fit(pb, iterations=iterations)
    assert hip.lib().rfd_fit_pose_workspace_bytes(0, 5) == 0 and hip.lib().rfd_fit_pose_workspace_bytes(2, 27) == \
        8 * (27 * 5 + 2) + 4 * 8 * 2
    assert hip.stream_status_bits() == 0


# --------------------------------------------------------------------------------------------------- 10. evaluate
def test_evaluate_with_the_device_fit(hip, golden_dir):
    """the scene of tests/test_gpu_evaluation.py::test_evaluate_end_to_end"""
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    from test_gpu_evaluation import labels_from_proposals
    fn = np.load(os.path.join(golden_dir, "F_NET.npz"))
    fnms = np.load(os.path.join(golden_dir, "F_NMS.npz"))
    seed, n_raw, n_pts = (int(v) for v in fn["pc_seed"])
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=seed, n_raw=n_raw, n_points=n_pts)[None]).cuda()
    cfg = Config({'generation': {'resolution_0': 8, 'upsampling_steps': 1}}, mean_size_arr=fnms['mean_size_arr'])
    net = ISCNet(cfg)
    for name, s in (('backbone', 101), ('voting', 102), ('detection', 103), ('skip_propagation', 104),
                    ('completion', 105)):
        synthetic.load_seeded(getattr(net, name), s)
    net = net.cuda().eval()
    detect = net.detect

    def detect_like_the_fixture(point_clouds):
        ep, pf = detect(point_clouds)
        ep['objectness_scores'] = torch.from_numpy(fnms['objectness_scores']).cuda()
        ep['size_residuals_normalized'] = ep['size_residuals_normalized'] * 0.2
        return ep, pf
    net.detect = detect_like_the_fixture
    end_points, ids, meshes = net.generate({'point_clouds': pc}, selection='nms')
    labels, n_gt = labels_from_proposals(end_points['parsed_predictions'], end_points['pred_mask'], fnms['mean_size_arr'])
    data = dict(labels, point_clouds=pc)
    unrefined = end_points['parsed_predictions']['pred_corners_3d_upright_camera'].clone()
    parsed0 = end_points['parsed_predictions']
    ep, ids2, meshes2, rec = net.evaluate(data, fit='device')
    assert torch.equal(ids2, ids) and len(meshes2) == len(meshes)
    assert len(rec.compact()['cls']) > 0 and rec.compact()['npos'].sum() == n_gt
    # the other method on the same proposals and meshes: what evaluate(fit='autograd') runs after the same generate()
    auto = net.fit_mesh_to_scan({'meshes': meshes2, 'proposal_ids': ids2}, parsed0, {'pred_mask': ep['pred_mask']}, pc,
                                cfg.config['generation']['dump_threshold'], method='autograd')
    scored = ep['parsed_predictions']['pred_corners_3d_upright_camera']
    fitted = [j for _, j in ep['parsed_predictions']['fit_indices']]
    moved = (scored - unrefined).abs().amax(dim=(2, 3))[0]
    assert fitted and float(moved[fitted].max()) > 1e-4, "the device fit moved no box"
    assert float(moved[[j for j in range(moved.shape[0]) if j not in fitted]].max()) == 0.0
    assert ep['parsed_predictions']['fit_indices'] == auto['fit_indices']
    diff = float((scored - auto['pred_corners_3d_upright_camera']).abs().max())
    print("%d boxes fitted, the furthest by %.3f; device vs autograd corners: %.2e" % (len(fitted), float(moved.max()), diff))
    assert diff < 5e-3
    with pytest.raises(ValueError, match="one of autograd, device"):
        net.evaluate(data, fit='host')
    assert hip.stream_status_bits() == 0
