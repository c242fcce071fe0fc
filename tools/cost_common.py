"""What the *_cost.py tools share: the repository on sys.path, timing between HIP events, the "no GPU" exit, the JSON
line, the dented marching-cubes spheres that render_cost, decimate_cost, fuse_cost and sample_cost measure on, and the
scene of such spheres that render_cost and mesh_dist_cost share.
Importing it is the tools' prologue; no *_cost.py imports another."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRID = 48


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = [event_ms(fn) for _ in range(reps)]
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def device_ms(fn, reps, windows=5):
    """completion_cost's and loss_cost's figure: ms per call over `windows` windows of `reps` calls -> median, min, max"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def need_gpu_or_exit(tool_name):
    if not torch.cuda.is_available():
        raise SystemExit("%s measures on a GPU: none is visible" % tool_name)


def emit(result, out_path):
    """print `result` as one JSON line; write the same line to out_path if one is given"""
    text = json.dumps(result)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


def placement_draws(rng, n_obj):
    """the two draws that place a box used again (centre offsets, heading noise); the objects' dents are drawn after them"""
    return rng.uniform(-1.5, 1.5, (n_obj, 3)), rng.normal(0, 0.3, n_obj)


def object_grids(rng, n_obj):
    """(n_obj, GRID, GRID, GRID) f32 value grids on the GPU: a sphere with a few dents of its own per object"""
    g = np.stack(np.meshgrid(*[np.arange(GRID, dtype=np.float32)] * 3, indexing='ij'), -1) - (GRID - 1) / 2.
    r = np.linalg.norm(g, axis=-1)
    grids = torch.empty(n_obj, GRID, GRID, GRID, device="cuda")
    for k in range(n_obj):
        w = rng.normal(0, 1, 3)
        grids[k] = torch.from_numpy((0.45 * GRID - r + 1.5 * np.sin(g @ w / 4.)).astype(np.float32))
    return grids


def real_mesh():
    """one of those spheres as a mesh on the GPU -> vertices, faces"""
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    return marching_cubes_batch(object_grids(np.random.default_rng(5), 1), 0.)[0]


def scene_inputs(n_obj, points=80000):
    """the scene render_cost and mesh_dist_cost measure on: n_obj of those spheres as meshes in the synthetic scene's boxes (a
    box used again: somewhere else) -> meshes, proposal ids, parsed predictions, scan"""
    import types
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet import box_util
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    pc, boxes, _ = synthetic.synthetic_scene(seed=100, n_raw=int(points * 1.5), n_points=points, return_boxes=True)
    rng = np.random.default_rng(5)
    again = np.arange(n_obj) >= len(boxes)                                       # a box used again: somewhere else
    boxes = boxes[np.arange(n_obj) % len(boxes)].astype(np.float64)
    offset, noise = placement_draws(rng, n_obj)
    centre = boxes[:, :3] + again[:, None] * offset * (1., 1., 0.)
    heading = boxes[:, 6] + noise
    corners = box_util.box_corners_upright_camera(torch.from_numpy(centre), torch.from_numpy(boxes[:, 3:6]),
                                                  torch.from_numpy(heading))[None].cuda()
    grids = object_grids(rng, n_obj)
    meshes = [types.SimpleNamespace(vertices=v, faces=f) for v, f in marching_cubes_batch(grids, 0.)]
    parsed = {'pred_corners_3d_upright_camera': corners,
              'pred_sem_cls': torch.from_numpy(rng.integers(0, 18, (1, n_obj))).cuda()}
    return meshes, torch.arange(n_obj).view(1, n_obj, 1), parsed, torch.from_numpy(pc[None]).cuda()
