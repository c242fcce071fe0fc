"""CPU: the pieces of fit_mesh_to_scan's device method that need no GPU -- the ragged float64 restatement tests/fit_f64.py
(its analytic gradient against autograd on the reference's padded formulation, its fp32 Adam against torch.optim.Adam),
the fixture tests/golden/F_FITD.npz (against the reference's run in F_FIT.npz, and against the restatement it was made
with), and fit.prepare_fit's batched set-up and fit.padded_problem's tensors against the per-object loop below (the
set-up written out one object at a time; it must stay independent of prepare_fit: fit.py's docstring)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fit_f64
from rfdnet_amd.iscnet import fit


@pytest.fixture(scope="module")
def fxd(golden_dir):
    return np.load(os.path.join(golden_dir, "F_FITD.npz"))


class Mesh(object):
    def __init__(self, vertices):
        self.vertices = vertices


def f_fit_inputs(golden_dir, device="cpu"):
    """-> fixture, the arguments of fit_mesh_to_scan for it"""
    fx = np.load(os.path.join(golden_dir, "F_FIT.npz"))
    K = int(fx["n_meshes"])
    meshes = [Mesh(fx["verts_%d" % j]) for j in range(K)]
    parsed = {'pred_corners_3d_upright_camera': torch.from_numpy(fx["corners_in"]).to(device),
              'obj_prob': torch.from_numpy(fx["obj_prob"]).to(device)}
    return fx, (meshes, np.arange(K).reshape(1, K, 1), parsed, {'pred_mask': torch.from_numpy(fx["pred_mask"]).to(device)},
                torch.from_numpy(fx["scan"]).to(device), 0.5)


# ------------------------------------------------------------------------------------------------ 1. analytic gradient
def test_analytic_gradient_equals_autograd_on_the_padded_formulation():
    """three objects padded to 64 mesh rows and 96 scan rows (the constants only set the mean's denominator): one with
    fewer vertices than the pad and scan points next to its centre (the extra zero row is the nearest neighbour of some),
    one with exactly 64 vertices (no extra row), one with a single vertex and every scan point next to its centre"""
    rng = np.random.default_rng(5)
    PAD_V, PAD_S = 64, 96
    n_vertices, n_scan = (40, 64, 1), (50, 96, 7)
    P = 3
    params = np.array([[0.9, -0.42, 0.45, 0.42], [-1.0, 0.98, 0.35, -0.5], [0.3, 0.2, -0.6, 2.1]])
    objs, scans = [], []
    for p in range(P):
        o = rng.uniform(-0.5, 0.5, (n_vertices[p], 3)) * np.array([1.2, 0.6, 0.9])
        o[:, 0] = np.where(o[:, 0] > 0, 0.6, -0.6)               # on two faces: nothing near the centre
        s = params[p, :3] + rng.uniform(-0.7, 0.7, (n_scan[p], 3))
        s[:10] = params[p, :3] + rng.uniform(-0.05, 0.05, (10, 3))[:len(s[:10])]
        objs.append(o)
        scans.append(s)
    obj_pad, scan_pad, mask = torch.zeros(P, PAD_V, 3, dtype=torch.float64), torch.zeros(P, PAD_S, 3, dtype=torch.float64), \
        torch.zeros(P, PAD_S, dtype=torch.float64)
    for p in range(P):
        obj_pad[p, :n_vertices[p]] = torch.from_numpy(objs[p])
        scan_pad[p, :n_scan[p]] = torch.from_numpy(scans[p])
        mask[p, :n_scan[p]] = 1
    centre = torch.tensor(params[:, :3], requires_grad=True)
    theta = torch.tensor(params[:, 3], requires_grad=True)
    rot = torch.zeros(P, 3, 3, dtype=torch.float64)                # network.py:293-303
    rot[:, 2, 2] = 1
    rot[:, 0, 0] = torch.cos(theta)
    rot[:, 0, 1] = torch.sin(theta)
    rot[:, 1, 0] = -torch.sin(theta)
    rot[:, 1, 1] = torch.cos(theta)
    after = torch.bmm(obj_pad, rot) + centre.unsqueeze(-2)
    nearest = torch.cdist(scan_pad, after, compute_mode='donot_use_mm_for_euclid_dist').argmin(2)    # the first minimum
    diff = torch.gather(after, 1, nearest.unsqueeze(-1).expand(-1, -1, 3)) - scan_pad
    dist2 = (diff * diff).sum(-1)
    per_object = (dist2 * mask).sum(1)
    loss = torch.mean(dist2 * mask) * 1e3
    loss.backward()
    want_grad = torch.cat([centre.grad, theta.grad[:, None]], 1).numpy()
    assert int((nearest[0, :n_scan[0]] >= n_vertices[0]).sum()) >= 5      # padded rows are nearest neighbours
    assert int((nearest[0, :n_scan[0]] > n_vertices[0]).sum()) == 0       # ... and only the first of them

    ragged = [np.concatenate([o, np.zeros((1, 3))]) if len(o) < PAD_V else o for o in objs]
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    assert [len(r) for r in ragged] == [41, 64, 2]
    loss_scale = 1e3 / (P * PAD_S)
    got = fit_f64.terms(np.concatenate(ragged), off(ragged), np.concatenate(scans), off(scans), params)
    got_loss, got_grad = got[:, 0].sum() * loss_scale, got[:, 1:] * loss_scale
    want_loss = float(loss.detach())
    # the third object's seven scan points all sit next to its centre: every one is assigned to the extra row, q = 0,
    # and its heading gradient is exactly 0 on both sides
    assert want_grad[2, 3] == 0 and got_grad[2, 3] == 0 and np.abs(want_grad).reshape(-1)[:11].min() > 0
    err = np.abs(got_grad - want_grad)
    print("loss %.15g vs %.15g; gradient, largest relative difference %.2e"
          % (got_loss, want_loss, (err.reshape(-1)[:11] / np.abs(want_grad).reshape(-1)[:11]).max()))
    assert abs(got_loss - want_loss) <= 1e-12 * abs(want_loss)
    np.testing.assert_allclose(got[:, 0], per_object.detach().numpy(), rtol=1e-12, atol=0)
    assert (err <= 1e-12 * np.abs(want_grad)).all(), err


# -------------------------------------------------------------------------------------------------------------- 2. Adam
def test_fp32_adam_equals_torch_bit_for_bit():
    """100 steps of a recorded gradient sequence on the reference's two parameter tensors, (P,3) centres and (P) headings,
    CPU fp32; gradients over five decades, some exactly 0"""
    rng = np.random.default_rng(9)
    P, T = 3, 100
    grads = (rng.normal(0, 1, (T, P, 4)) * 10.0 ** rng.uniform(-4, 1, (T, P, 4))).astype(np.float32)
    grads[:, 2, 3] = 0                                              # a heading whose gradient is exactly 0 stays put
    grads[::7, 0, 1] = 0
    start = rng.normal(0, 1, (P, 4)).astype(np.float32)
    centre = torch.tensor(start[:, :3].copy(), requires_grad=True)
    theta = torch.tensor(start[:, 3].copy(), requires_grad=True)
    opt = torch.optim.Adam([centre, theta], lr=0.01)
    par, m, v = start.copy(), np.zeros_like(start), np.zeros_like(start)
    for t in range(T):
        centre.grad, theta.grad = torch.from_numpy(grads[t, :, :3].copy()), torch.from_numpy(grads[t, :, 3].copy())
        opt.step()
        par, m, v = fit_f64.adam_step(par, m, v, grads[t], t + 1, 0.01, True)
        assert par.dtype == np.float32
        want = np.concatenate([centre.detach().numpy(), theta.detach().numpy()[:, None]], 1)
        assert np.array_equal(par.view(np.int32), want.view(np.int32)), (t, par, want)
    assert par[2, 3] == start[2, 3] and not np.array_equal(par, start)


def test_fma32_rounds_once():
    """(1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies half-way between two fp32 values; +-2^-80 decides the direction, but a sum
    rounded to f64 first has lost it and goes to the even neighbour both times"""
    a = np.array([1 + 2.0 ** -12], np.float32)
    lo, hi = np.float32(1 + 2.0 ** -11), np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert fit_f64.fma32(a, a, np.array([2.0 ** -80], np.float32))[0] == hi
    assert fit_f64.fma32(a, a, np.array([-2.0 ** -80], np.float32))[0] == lo
    assert fit_f64.fma32(a, a, np.array([0.0], np.float32))[0] == lo                 # the tie itself: to even
    assert np.float32(np.float64(a[0]) * np.float64(a[0]) + np.float64(np.float32(2.0 ** -80))) == lo   # the naive way
    out = fit_f64.fma32(np.array([3.0, 0.0], np.float32), np.array([0.5, 7.0], np.float32), np.array([0.25, -0.0], np.float32))
    assert out.dtype == np.float32 and out[0] == 1.75 and out[1] == 0


# ------------------------------------------------------------------------------------ 3. fixture against the reference
def test_fixture_float64_corners_match_the_reference_run(golden_dir, fxd):
    fx = np.load(os.path.join(golden_dir, "F_FIT.npz"))
    got, want = fxd["fit_f64_corners"], fx["corners_out"][0, :2]
    moved = np.abs(want - fx["corners_in"][0, :2]).reshape(2, -1).max(1)
    err = np.abs(got - want).reshape(2, -1).max(1)
    print("float64 restatement vs the reference's fit_mesh_to_scan: %s on boxes that moved %s; fp32 variant vs float64 %.1e"
          % (err, moved, np.abs(fxd["fit_f32_corners"] - got).max()))
    assert err.max() < 5e-3 and moved.min() > 0.02
    assert fxd["fit_f64_loss"].shape == (100,) and fxd["fit_f64_params"].shape == (100, 2, 4)
    best = int(fxd["fit_f64_best_iter"])
    assert best == int(np.argmin(fxd["fit_f64_loss"])) and fxd["fit_f64_loss"][best] < 0.3 * fxd["fit_f64_loss"][0]
    np.testing.assert_array_equal(fxd["fit_f64_best_params"], fxd["fit_f64_params"][best])
    np.testing.assert_allclose(fit_f64.box_corners(fxd["fit_sizes"], fxd["fit_f64_best_params"]), got, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------- 4. fixture drift
def test_fixture_is_what_the_restatement_computes(golden_dir, fxd):
    _, args = f_fit_inputs(golden_dir)
    pb = fit.prepare_fit(*args)
    assert pb.n_vertices == list(fxd["fit_n_vertices"]) and pb.n_scan_points == list(fxd["fit_n_scan_points"])
    np.testing.assert_array_equal(pb.obj_off.numpy(), fxd["fit_obj_off"])
    np.testing.assert_array_equal(pb.scan_off.numpy(), fxd["fit_scan_off"])
    assert pb.loss_scale == float(fxd["fit_loss_scale"]) == 1e3 / (2 * 50000)
    problem = (pb.obj.numpy(), pb.obj_off.numpy(), pb.scan.numpy(), pb.scan_off.numpy(), pb.params0.numpy(), pb.loss_scale)
    for fp32, tag in ((False, "f64"), (True, "f32")):
        got = fit_f64.fit(*problem, iterations=3, fp32=fp32)
        np.testing.assert_allclose(got['hist_loss'], fxd["fit_%s_loss" % tag][:3], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got['hist_params'], fxd["fit_%s_params" % tag][:3], rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------------- 5. set-up
def per_object_setup(meshes, proposal_ids, parsed_predictions, eval_dict, input_scan, dump_threshold):
    """the reference's set-up loop (network.py:196-269), one object at a time, with the scan rows it selects kept as indices
    -> index_list, scaled mesh points (V,3) f32, scan rows (index array), scan points (S,3) f32, start parameters"""
    corners_all = torch.as_tensor(np.asarray(parsed_predictions['pred_corners_3d_upright_camera'])).double()
    obj_prob = torch.as_tensor(np.asarray(parsed_predictions['obj_prob'])).double()
    pred_mask = torch.as_tensor(np.asarray(eval_dict['pred_mask'])).long()
    ids = torch.as_tensor(np.asarray(proposal_ids)).long()
    scan = input_scan.double()
    out = []
    for i in range(obj_prob.shape[0]):
        id_row = ids[i, :, 0].tolist()
        height = torch.quantile(scan[i, :, 2], 0.05)
        above = torch.nonzero(scan[i, :, 2] >= height)[:, 0]
        scene_scan = scan[i, above, :3]
        for j in range(obj_prob.shape[1]):
            if not (pred_mask[i, j] == 1 and obj_prob[i, j] > dump_threshold):
                continue
            verts = torch.as_tensor(np.asarray(meshes[id_row.index(j)].vertices))
            if verts.shape[0] > fit.MAX_OBJ_POINTS:
                verts = verts[::-(-verts.shape[0] // fit.MAX_OBJ_POINTS)]
            obj_points = fit.normalise_mesh_points(verts)
            centroid, sizes, orientation = fit.box_params_from_corners(corners_all[i, j][None])
            larger = fit.flip_axis_to_depth(fit.get_3d_box(1.2 * sizes, -orientation, fit.flip_axis_to_camera(centroid)))[0]
            rows = above[fit.points_in_box(scene_scan, larger)]
            if rows.shape[0] < 5:
                continue
            rows = rows[:fit.MAX_PC_IN_BOX]
            out.append(((i, j), (obj_points * sizes).float(), rows, scan[i, rows, :3].float(),
                        torch.cat([centroid[0].float(), orientation.float()]), sizes[0]))
    return out


def random_scene():
    """two scenes of 3000 points around six boxes each in one call; masked proposals, one with a low score, one far from
    every point, one mesh of 12 000 vertices (subsampled with stride 2), vertices as arrays and as tensors, and another
    proposal -> mesh permutation in each scene"""
    rng = np.random.default_rng(17)
    B, K, N = 2, 6, 3000
    centre = rng.uniform(-2, 2, (B, K, 3)) * np.array([1, 1, 0.2]) + np.array([0, 0, 0.6])
    size = rng.uniform(0.4, 1.4, (B, K, 3))
    heading = rng.uniform(-3, 3, (B, K))
    centre[1, 4] = (9.0, 9.0, 0.5)                                    # no scan point anywhere near
    scan = np.zeros((B, N, 4), np.float32)
    for b in range(B):
        pts = [np.c_[rng.uniform(-3, 3, (600, 2)), rng.normal(0, 0.01, 600)]]
        for k in range(K):
            if (b, k) == (1, 4):
                pts.append(np.c_[rng.uniform(-3, 3, (400, 2)), rng.normal(0, 0.01, 400)])
                continue
            u = rng.uniform(-0.6, 0.6, (400, 3)) * size[b, k]
            c, s = np.cos(heading[b, k]), np.sin(heading[b, k])
            pts.append(u @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]) + centre[b, k])
        scan[b, :, :3] = np.concatenate(pts)[rng.permutation(N)]
    corners = fit.get_3d_box(torch.from_numpy(size), -torch.from_numpy(heading),
                             fit.flip_axis_to_camera(torch.from_numpy(centre))).numpy()
    obj_prob = rng.uniform(0.6, 1.0, (B, K))
    obj_prob[0, 3] = 0.2
    pred_mask = np.ones((B, K), np.int64)
    pred_mask[0, 1] = pred_mask[1, 0] = 0
    ids = np.stack([rng.permutation(K) for _ in range(B)]).reshape(B, K, 1)
    meshes = []
    for k in range(K):
        n = 12000 if k == 2 else int(rng.integers(30, 400))
        v = rng.normal(0, 1, (n, 3)) * rng.uniform(0.5, 2, 3) + rng.uniform(-1, 1, 3)
        meshes.append(Mesh(torch.from_numpy(v.astype(np.float32)) if k % 2 else v))
    return (meshes, ids, {'pred_corners_3d_upright_camera': corners, 'obj_prob': obj_prob}, {'pred_mask': pred_mask},
            torch.from_numpy(scan), 0.5)


def check_setup(args):
    want = per_object_setup(*args)
    pb = fit.prepare_fit(*args)
    assert pb.P == len(want) and pb.index_list == [w[0] for w in want]
    obj_off, scan_off = pb.obj_off.numpy(), pb.scan_off.numpy()
    assert obj_off.dtype == scan_off.dtype == np.int32 and pb.obj.dtype == pb.scan.dtype == pb.params0.dtype == torch.float32
    assert obj_off[0] == scan_off[0] == 0 and obj_off[-1] == pb.obj.shape[0] and scan_off[-1] == pb.scan.shape[0]
    for p, (_, scaled, rows, pts, par, sizes) in enumerate(want):
        V, extra = scaled.shape[0], scaled.shape[0] < fit.MAX_OBJ_POINTS
        assert obj_off[p + 1] - obj_off[p] == V + extra and pb.n_vertices[p] == V
        assert torch.equal(pb.obj[obj_off[p]:obj_off[p] + V], scaled)
        if extra:
            assert (pb.obj[obj_off[p + 1] - 1] == 0).all()
        assert scan_off[p + 1] - scan_off[p] == rows.shape[0] == pb.n_scan_points[p] >= 5
        assert torch.equal(pb.scan_index[scan_off[p]:scan_off[p + 1]], rows)
        assert torch.equal(pb.scan[scan_off[p]:scan_off[p + 1]], pts)
        assert torch.equal(pb.params0[p], par) and torch.equal(pb.sizes[p], sizes)
    # the tiles partition every object's rows, in order
    step = 256 * pb.points_per_thread
    tile_obj, tile_start = pb.tile_obj.numpy(), pb.tile_start.numpy()
    assert pb.points_per_thread == (1 if scan_off[-1] <= fit.PPT_SWITCH else 4) and len(tile_obj) == sum(-(-n // step) for n in pb.n_scan_points)
    for p in range(pb.P):
        np.testing.assert_array_equal(tile_start[tile_obj == p], np.arange(scan_off[p], scan_off[p + 1], step))
    return pb


def test_prepare_fit_equals_the_per_object_setup(golden_dir):
    _, args = f_fit_inputs(golden_dir)
    pb = check_setup(args)
    assert pb.index_list == [(0, 0), (0, 1)] and pb.n_vertices == [1500, 1700]
    seen = check_setup(random_scene())
    assert seen.index_list == [(0, 0), (0, 2), (0, 4), (0, 5), (1, 1), (1, 2), (1, 3), (1, 5)]      # all but the four
    assert seen.n_vertices.count(6000) == 2                              # 12 000 vertices, stride 2, once per scene
    # nothing selected: an empty problem, and finish_fit hands the boxes back untouched
    meshes, ids, parsed, ev, scan, _ = random_scene()
    empty = fit.prepare_fit(meshes, ids, parsed, ev, scan, 2.0)
    assert empty.P == 0 and fit.run_fit(empty) is None
    out = fit.finish_fit(empty, parsed)
    assert np.array_equal(out['pred_corners_3d_upright_camera'].numpy(), parsed['pred_corners_3d_upright_camera'])
    assert 'fit_indices' not in out
    # four points per thread above the switch, or on request
    assert fit.prepare_fit(*args, points_per_thread=4).tile_start.tolist() == [0, 1024, 2048, 3072, 3536, 4560, 5584, 6608]
    assert fit.PPT_SWITCH == 65536


def check_padded(args):
    """the padded tensors of the reference's loop, built from the per-object set-up"""
    want = per_object_setup(*args)
    P = len(want)
    obj = torch.zeros(P, fit.MAX_OBJ_POINTS, 3)
    pc = torch.zeros(P, fit.MAX_PC_IN_BOX, 3)
    mask = torch.zeros(P, fit.MAX_PC_IN_BOX)
    for p, (_, scaled, rows, pts, par, sizes) in enumerate(want):
        obj[p, :scaled.shape[0]] = scaled
        pc[p, :pts.shape[0]] = pts
        mask[p, :pts.shape[0]] = 1
    par = torch.stack([w[4] for w in want])
    got = fit.padded_problem(fit.prepare_fit(*args))
    assert len(got) == 5 and all(g.dtype == torch.float32 for g in got)
    for g, w in zip(got, (obj, pc, mask, par[:, :3], par[:, 3])):
        assert g.shape == w.shape and torch.equal(g, w)
    return P


def test_padded_problem_equals_the_padded_per_object_setup(golden_dir):
    _, args = f_fit_inputs(golden_dir)
    assert check_padded(args) == 2
    assert check_padded(random_scene()) == 8


def test_autograd_method_with_nothing_to_fit_returns_the_boxes_untouched(monkeypatch):
    meshes, ids, parsed, ev, scan, _ = random_scene()

    def no_loop(*a, **k):
        raise AssertionError("the optimisation loop was entered")
    monkeypatch.setattr(fit, "chamfer_loss", no_loop)
    monkeypatch.setattr(fit, "padded_problem", no_loop)
    out = fit.fit_mesh_to_scan(meshes, ids, parsed, ev, scan, 2.0, method='autograd')
    got = out['pred_corners_3d_upright_camera']
    assert np.array_equal(got.numpy(), parsed['pred_corners_3d_upright_camera'])
    assert not np.shares_memory(got.numpy(), parsed['pred_corners_3d_upright_camera'])
    assert 'fit_indices' not in out and 'fit_loss' not in out


def test_the_50000_point_cap_keeps_the_first_rows():
    rng = np.random.default_rng(3)
    N = 60000
    scan = np.c_[rng.uniform(-0.4, 0.4, (N, 2)), rng.uniform(0.1, 0.9, N), np.zeros(N)].astype(np.float32)[None]
    corners = fit.get_3d_box(torch.tensor([[[1.0, 1.0, 1.0], [0.5, 0.5, 0.5]]], dtype=torch.float64), torch.zeros(1, 2, dtype=torch.float64),
                             fit.flip_axis_to_camera(torch.tensor([[[0.0, 0.0, 0.5], [0.1, 0.1, 0.5]]], dtype=torch.float64))).numpy()
    meshes = [Mesh(rng.normal(0, 1, (20, 3))), Mesh(rng.normal(0, 1, (30, 3)))]
    args = (meshes, np.arange(2).reshape(1, 2, 1), {'pred_corners_3d_upright_camera': corners, 'obj_prob': np.ones((1, 2))},
            {'pred_mask': np.ones((1, 2), np.int64)}, torch.from_numpy(scan), 0.5)
    pb = check_setup(args)
    assert pb.n_scan_points[0] == 50000 and 5 <= pb.n_scan_points[1] < 50000 and pb.points_per_thread == 4


def test_unknown_method_is_refused():
    assert fit.fit_method(True) == 'autograd' and fit.fit_method('device') == 'device' and fit.fit_method(False) is None
    with pytest.raises(ValueError, match="one of autograd, device"):
        fit.fit_method('host')
    with pytest.raises(ValueError, match="one of autograd, device"):
        fit.fit_mesh_to_scan([], None, {}, {}, torch.zeros(1, 4, 3), 0.5, method='host')


# ------------------------------------------------------------------------------------------- the kernels' registers
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_fit_kernels_do_not_spill_and_use_no_atomics(tmp_path):
    """-Rpass-analysis=kernel-resource-usage with the library's flags: the three kernels of csrc/fit_pose.hip (the search
    with one and with four points per thread, the update) use no scratch; and no floating-point atomic is generated"""
    from rfdnet_amd.build import CODEGEN_FLAGS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(root, "rfdnet_amd", "csrc", "fit_pose.hip")
    common = [hipcc] + CODEGEN_FLAGS + ["-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "rfdnet_amd", "csrc"),
                                        "--cuda-device-only"]
    r = subprocess.run(common + ["-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "f.o"), src],
                       check=True, capture_output=True, text=True, cwd=str(tmp_path))
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 3 and sum("fit_nn_kernel" in n for n in names) == 2 and sum("fit_update_kernel" in n for n in names) == 1
    for key in ("VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]"):
        values = [int(v) for v in re.findall(r"remark:\s+%s:\s+(\d+)" % key, r.stderr)]
        assert values == [0, 0, 0], (key, values)
    print({n: v for n, v in zip(names, re.findall(r"remark:\s+VGPRs:\s+(\d+)", r.stderr))})
    subprocess.run(common + ["-S", "-o", str(tmp_path / "f.s"), src], check=True, capture_output=True, cwd=str(tmp_path))
    assert "atomic" not in open(str(tmp_path / "f.s")).read()
