"""Cost of fit_mesh_to_scan on one GPU, both methods: 'autograd' (every object padded to 10 000 mesh rows and 50 000 scan
rows, both Chamfer directions per step, the gradient through atomics, one host read per step) and 'device' (the ragged
loop of csrc/fit_pose.hip) -- a comparison, not a test.  Both legs start with the same batched set-up (fit.prepare_fit);
the 'autograd' leg then pads it (fit.padded_problem).

    python tools/fit_cost.py [--out profiles/fit_stage.json] [--reps 3]

Two cases: the scene of tests/golden/F_FIT.npz (two fitted objects), and a demo-sized synthetic scene: 13 boxes (the
synthetic scene's twelve cuboids and one of them again, all a little off in centre and heading) with 13 meshes from the
generator (ISCNet.reconstruct on the scene's first 13 proposals, seeded weights).  Per case and method: device milliseconds per call
(HIP events around a call that ends in a synchronise; the two methods alternate, `reps` rounds after a warm-up, the median),
the pairs evaluated per step (from the shapes), the calls through the C ABI and the host synchronisations per call (counted
under torch's sync debug mode).  For the device method also the loop alone (run_fit), the kernel launches (two per step),
and both points-per-thread instantiations of fit_nn_kernel: the one fit.PPT_SWITCH chooses and the other."""
import argparse
import os
import statistics
import warnings

import numpy as np
import torch

from cost_common import ROOT, emit, event_ms


class Mesh(object):
    def __init__(self, vertices):
        self.vertices = vertices


def host_syncs(fn):
    """synchronising calls torch itself makes inside fn (sync debug mode 'warn': one warning each)"""
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def f_fit_case():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "F_FIT.npz"))
    K = int(fx["n_meshes"])
    parsed = {'pred_corners_3d_upright_camera': torch.from_numpy(fx["corners_in"]).cuda(),
              'obj_prob': torch.from_numpy(fx["obj_prob"]).cuda()}
    return ([Mesh(fx["verts_%d" % j]) for j in range(K)], np.arange(K).reshape(1, K, 1), parsed,
            {'pred_mask': torch.from_numpy(fx["pred_mask"]).cuda()}, torch.from_numpy(fx["scan"]).cuda(), 0.5)


def demo_case(points, n_obj=13):
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet import fit
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    pc, boxes, _ = synthetic.synthetic_scene(seed=100, n_raw=int(points * 1.5), n_points=points, return_boxes=True)
    cfg = Config({}, mean_size_arr=None)
    cfg.eval_overrides['allow_placeholder_sizes'] = True
    net = ISCNet(cfg)
    synthetic.load_seeded(net, seed=cfg.config['seed'])
    net = net.cuda().eval()
    scan = torch.from_numpy(pc[None]).cuda()
    with torch.no_grad():                                                  # the first n_obj proposals, whatever their scores
        end_points, proposal_features = net.detect(scan)
        ids = torch.arange(n_obj, device="cuda").view(1, n_obj, 1)
        meshes = net.reconstruct(end_points, proposal_features, ids, scan)
    assert len(meshes) == n_obj, "the generator returned %d meshes" % len(meshes)
    meshes = [Mesh(m.vertices) for m in meshes]
    rng = np.random.default_rng(4)
    boxes = np.concatenate([boxes, boxes[:1]])[:n_obj].astype(np.float64)
    centre = boxes[:, :3] + rng.normal(0, 0.04, (n_obj, 3))
    heading = boxes[:, 6] + rng.normal(0, 0.1, n_obj)
    corners = fit.get_3d_box(torch.from_numpy(boxes[:, 3:6]), -torch.from_numpy(heading),
                             fit.flip_axis_to_camera(torch.from_numpy(centre)))[None].cuda()
    parsed = {'pred_corners_3d_upright_camera': corners, 'obj_prob': torch.ones(1, n_obj, dtype=torch.float64, device="cuda")}
    return (meshes, np.arange(n_obj).reshape(1, n_obj, 1), parsed,
            {'pred_mask': torch.ones(1, n_obj, dtype=torch.int64, device="cuda")}, scan, 0.5)


def measure(name, args, reps):
    from rfdnet_amd import _lib
    from rfdnet_amd.iscnet import fit
    calls = []
    call = _lib.call

    def counting(entry, *a):
        calls.append(entry)
        return call(entry, *a)
    chosen = fit.prepare_fit(*args)
    other = fit.prepare_fit(*args, points_per_thread=5 - chosen.points_per_thread)
    legs = {'autograd': lambda: fit.fit_mesh_to_scan(*args, method='autograd'),
            'device': lambda: fit.fit_mesh_to_scan(*args, method='device'),
            'device_loop': lambda: fit.run_fit(chosen),
            'device_loop_other': lambda: fit.run_fit(other)}
    ms = {k: [] for k in legs}
    for k in legs:                                                        # warm-up
        legs[k]()
    torch.cuda.synchronize()
    for _ in range(reps):                                                 # the legs alternate
        for k in legs:
            ms[k].append(event_ms(legs[k]))
    counts = {}
    _lib.call = counting
    try:
        for k in ('autograd', 'device'):
            del calls[:]
            syncs = host_syncs(legs[k])
            counts[k] = {"abi_calls": len(calls), "host_synchronisations": syncs}
    finally:
        _lib.call = call
    a, d = fit.fit_mesh_to_scan(*args, method='autograd'), fit.fit_mesh_to_scan(*args, method='device')
    diff = float((a['pred_corners_3d_upright_camera'] - d['pred_corners_3d_upright_camera']).abs().max())
    P = chosen.P
    stat = lambda v: {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
    n_rows = [v + (v < fit.MAX_OBJ_POINTS) for v in chosen.n_vertices]
    return {"case": name, "objects": P, "vertices": chosen.n_vertices, "scan_points": chosen.n_scan_points, "iterations": 100,
            "max_corner_diff_between_methods": diff,
            "autograd": dict(stat(ms['autograd']), pairs_per_step=2 * P * fit.MAX_OBJ_POINTS * fit.MAX_PC_IN_BOX, **counts['autograd']),
            "device": dict(stat(ms['device']), pairs_per_step=int(sum(s * v for s, v in zip(chosen.n_scan_points, n_rows))),
                           kernel_launches=200, **counts['device'],
                           loop=dict(stat(ms['device_loop']), points_per_thread=chosen.points_per_thread,
                                     workgroups=int(chosen.tile_obj.shape[0])),
                           loop_other_choice=dict(stat(ms['device_loop_other']), points_per_thread=other.points_per_thread,
                                                  workgroups=int(other.tile_obj.shape[0])))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fit_stage.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=80000, help="points of the synthetic scene")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from rfdnet_amd.iscnet import fit
    rows = [measure("F_FIT", f_fit_case(), args.reps), measure("demo-sized, 13 objects", demo_case(args.points), args.reps)]
    line = {"tool": "fit_cost", "device": torch.cuda.get_device_name(0), "rounds": args.reps, "ppt_switch": fit.PPT_SWITCH,
            "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    emit(line, args.out)


if __name__ == "__main__":
    main()
