"""CPU: the mesh-IoU restatement (tests/mesh_iou_f64.py, rules M1 - M5 of include/rfd_mesh_eval.h) against the
reference's own results in tests/golden/F_MIOU.npz, rule M1 on hand-made extents, and the host half of mesh mAP
(rfdnet_amd.iscnet.mesh_eval.MeshAPCalculator, merge_records / gather_records with 'tp_mesh').

IoU: bit-equal, no tolerance -- the reference and the restatement perform the same correctly rounded float64 operations
in the same order on the same integer counts.  Metrics: 1e-12, the tolerance tests/test_gpu_evaluation.py holds the box
metrics to (the cumulative sums are of 0 / 1 flags; only the order of a mean's additions can differ)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_det_f64 as E
import mesh_iou_f64 as M
from rfdnet_amd import sharding

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = (("pcp1", True), ("pcp0", False))
THR = (0.25, 0.5)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "F_MIOU.npz"))


@pytest.fixture(scope="module")
def objs(fx):
    return M.fixture_objects(fx)


def restated_records(fx, pcp):
    """box records from the reference's box IoU, with 'tp_mesh' from the same matching on its mesh IoU"""
    args = (fx['corners'], fx['obj_prob'], fx['sem_cls_probs'], fx['pred_sem_cls'], fx['pred_mask'], fx['gt_corners'],
            fx['gt_sem_cls_label'], fx['gt_box_label_mask'] == 1)
    kw = dict(thr=THR, conf_thresh=float(fx['conf_thresh']), per_class_proposal=pcp)
    rec, _ = E.scene_records(*args, iou3d=fx['iou3d'], **kw)
    rec_mesh, _ = E.scene_records(*args, iou3d=fx['mesh_iou'], **kw)
    return dict(rec, tp_mesh=rec_mesh['tp'])


def test_fixture_covers_the_cases(fx, objs):
    D = set(int(d) for d in fx['D'])
    assert {2, 63, 64, 65, 130} <= D and len(objs) == 21
    assert any(o.S.sum() == 0 and o.I.sum() > 0 for o in objs) and any(o.I.sum() == 0 and o.S.sum() > 0 for o in objs)
    v = fx['mesh_iou']
    assert (v == 1.0).sum() == 2 and ((v > 0) & (v < 0.25)).any() and ((v > 0.25) & (v < 0.5)).any() and (v > 0.5).any()
    live = v[(v > 0) & (v < 1)]
    assert min(np.abs(live - t).min() for t in THR) > 1e-6
    assert fx['gt_sem_cls_label'].max() == 2 and fx['pred_mask'].shape[0] == 2
    assert os.path.getsize(os.path.join(GOLDEN, "F_MIOU.npz")) < 256 * 1024
    # the tie is real: the D = 65 block's centres lie exactly on the D = 64 block's cell boundaries and outer faces
    src, dst = objs[int(fx['pred_obj'][0, 3])], objs[int(fx['gt_obj'][0, 1])]
    q = (M.centres(src.U, src.lo, src.cell) - dst.lo) / dst.cell
    assert (q == np.round(q)).all() and q.min() == 0 and q.max() == 64


def test_restatement_equals_the_reference(fx, objs):
    for s in range(fx['pred_obj'].shape[0]):
        pi, gi = fx['pred_obj'][s], fx['gt_obj'][s]
        P, G = int((pi >= 0).sum()), int((gi >= 0).sum())
        iou, cnt = M.iou_matrix([objs[i] for i in pi[:P]], [objs[i] for i in gi[:G]])
        np.testing.assert_array_equal(cnt, fx['counts'][s, :P, :G])
        assert iou.tobytes() == np.ascontiguousarray(fx['mesh_iou'][s, :P, :G]).tobytes()          # bit-equal
    # an object against itself is exactly 1; one without a grid is 0 with everything
    assert M.iou_matrix([objs[0]], [objs[0]])[0][0, 0] == 1.0
    assert M.iou_matrix([M.Obj()], [objs[0]])[0][0, 0] == 0.0


def test_pack_words_layout():
    rng = np.random.default_rng(0)
    for D in (2, 63, 64, 65, 130):
        U = rng.random((D, D, D)) < 0.3
        w = M.pack_words(U)
        W = (D + 63) // 64
        assert w.shape == (D * D * W,) and w.dtype == np.uint64
        for i, j, k in ((0, 0, 0), (D - 1, D - 1, D - 1), (1, 0, D // 2)):
            assert bool((int(w[(i * D + j) * W + (k >> 6)]) >> (k & 63)) & 1) == bool(U[i, j, k])
        assert sum(bin(int(x)).count("1") for x in w[:W * D]) == int(U[0].sum())


@pytest.mark.parametrize("frame_of", ["restatement", "module"])
def test_rule_m1(frame_of):
    from rfdnet_amd.iscnet import mesh_eval
    f = M.frame_of_extent if frame_of == "restatement" else mesh_eval.object_frame
    lo = np.array([1.0, -2.0, 0.5])

    def run(L, vs, other=(0.3, 0.1)):
        return f(lo, lo + np.array([L * other[0], L, L * other[1]]), vs)
    # voxel size 0.25 is exact in binary: L / voxel_size at an integer, and one ulp below it
    lo_, L, cell, D = run(1.0, 0.25)
    assert D == 4 and cell == 0.25 and L == 1.0 and (lo_ == lo).all()
    below = np.nextafter(1.0, 0.0)
    # the extent is hi - lo of the stored corners: take it from there
    got = f(np.zeros(3), np.array([0.2, below, 0.1]), 0.25)
    assert got[3] == 3 and got[1] == below and got[2] == below / 3
    assert f(np.zeros(3), np.array([0.0, 1.75, 1.0]), 0.25)[3] == 7
    # clamped to 2
    assert f(np.zeros(3), np.array([0.01, 0.02, 0.03]), 0.047)[3] == 2
    assert f(np.zeros(3), np.array([0.01, 0.02, 0.03]), 0.047)[2] == 0.03 / 2
    # the default voxel size: 12 m is the first refusal
    assert f(np.zeros(3), np.array([1.0, 12.0, 1.0]), 0.047)[3] == 255
    with pytest.raises(ValueError):
        f(np.zeros(3), np.array([1.0, 12.1, 1.0]), 0.047)
    # no grid
    assert f(np.zeros(3), np.zeros(3), 0.047) is None
    assert f(np.zeros(3), np.array([np.nan, 1.0, 1.0]), 0.047) is None
    assert f(np.zeros(3), np.array([np.inf, 1.0, 1.0]), 0.047) is None
    assert f(np.full(3, np.inf), np.full(3, -np.inf), 0.047) is None


@pytest.mark.parametrize("tag,pcp", SETTINGS)
def test_mesh_calculator_gives_the_reference_metrics(fx, tag, pcp):
    from rfdnet_amd.iscnet.mesh_eval import MeshAPCalculator
    rec = restated_records(fx, pcp)
    calc = MeshAPCalculator(THR)
    calc.step(rec)
    got = calc.compute_metrics()
    for ti, t in enumerate(THR):
        key = "%s_%g" % (tag, t)
        keys = list(fx[key + '_metric_keys'])
        assert list(got[ti].keys()) == keys
        np.testing.assert_allclose(np.array([got[ti][k] for k in keys], np.float64), fx[key + '_metric_values'],
                                   rtol=0, atol=1e-12)
        for flags, sfx in (('tp', ''), ('tp_mesh', '_mesh')):                 # the reference's flags, in its score order
            cur = calc.class_curves(ti, flags=flags)
            box_like = E.class_curves([dict(rec, tp=rec[flags])], ti)
            for c in cur:
                np.testing.assert_array_equal(box_like[c][3], fx['%s_tp%s_%d' % (key, sfx, c)])
                np.testing.assert_allclose(cur[c][0], fx['%s_rec%s_%d' % (key, sfx, c)], rtol=0, atol=1e-12)
                np.testing.assert_allclose(cur[c][1], fx['%s_prec%s_%d' % (key, sfx, c)], rtol=0, atol=1e-12)
    single = MeshAPCalculator(0.5)
    single.step({k: (v[1:] if k in ('tp', 'tp_mesh') else v) for k, v in dict(rec, thr=(0.5,)).items()})
    assert single.compute_metrics() == got[1]
    assert got[0]['mAP_mesh'] != got[0]['mAP']                                # the two halves are not the same number


def test_mesh_calculator_needs_mesh_flags(fx):
    from rfdnet_amd.iscnet.evaluation import APCalculator
    from rfdnet_amd.iscnet.mesh_eval import MeshAPCalculator
    rec = restated_records(fx, True)
    box_only = {k: v for k, v in rec.items() if k != 'tp_mesh'}
    calc = MeshAPCalculator(THR)
    calc.step(box_only)
    with pytest.raises(ValueError):
        calc.compute_metrics()
    plain = APCalculator(THR)
    plain.step(rec)                                                           # the box calculator ignores the extra key
    ref = APCalculator(THR)
    ref.step(box_only)
    assert plain.compute_metrics() == ref.compute_metrics()
    with pytest.raises(NotImplementedError):
        APCalculator(0.25, None, evaluate_mesh=True)


def test_merge_records_with_and_without_mesh_flags(fx):
    from rfdnet_amd.iscnet.evaluation import merge_records
    rec = restated_records(fx, True)
    box_only = {k: v for k, v in rec.items() if k != 'tp_mesh'}
    both = merge_records([rec, rec])
    n = len(rec['cls'])
    assert both['tp_mesh'].shape == (2, 2 * n) and both['tp_mesh'].dtype == np.uint8
    np.testing.assert_array_equal(both['tp_mesh'][:, n:], rec['tp_mesh'])
    np.testing.assert_array_equal(both['tp'][:, :n], rec['tp'])
    plain = merge_records([box_only, box_only])
    assert set(plain) == {'cls', 'score', 'tp', 'npos', 'thr'}                # nothing new without mesh flags
    for k in ('cls', 'score', 'tp', 'npos'):
        np.testing.assert_array_equal(plain[k], both[k])
    with pytest.raises(ValueError, match="mesh"):
        merge_records([rec, box_only])
    assert 'tp_mesh' not in merge_records([], THR)


def test_native_symbols_and_header_present():
    from rfdnet_amd import _lib
    assert {"rfd_objgrid_pack", "rfd_mesh_iou_counts", "rfd_mesh_iou_finalize"} <= set(_lib.exported_symbols())
    header = os.path.join(os.path.dirname(GOLDEN), "..", "include", "rfd_mesh_eval.h")
    # the call table has one argument type per parameter of the prototype, the trailing stream included: ctypes passes
    # an argument beyond the table as a C int, which cuts a stream handle to 32 bits
    import re
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    protos = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(rfd_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}
    assert len(protos) == 3
    for name, n_params in protos.items():
        assert len(_lib.ABI[name][1]) == n_params, name


# ------------------------------------------------------------------------------------------------ gather_records
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, rec, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = sharding.gather_records([] if rank == 1 else [rec], dist, thr=THR)     # rank 1 was dealt no scene
    q.put((rank, {k: (v if k == 'thr' else np.asarray(v)) for k, v in g.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_records_passes_mesh_flags_through(fx):
    rec = restated_records(fx, True)
    assert (rec['tp_mesh'] != rec['tp']).any()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, rec, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, g in res:
        for k in ('cls', 'score', 'tp', 'tp_mesh', 'npos'):
            np.testing.assert_array_equal(g[k], rec[k])
    g = sharding.gather_records(rec, None)
    np.testing.assert_array_equal(g['tp_mesh'], rec['tp_mesh'])
