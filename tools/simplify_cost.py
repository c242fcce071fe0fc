"""Cost of the mesh simplification on one GPU -- a record, not a test.

    python tools/simplify_cost.py [--out profiles/simplify_cost.json] [--reps 5] [--warmup 1]

The meshes of one synthetic scene (the 13 marching-cubes meshes of dented spheres at 48^3 of tools/decimate_cost.py, about
18 600 faces each, in the generator's cube) simplified to 2 000 and to 500 faces each, and one model of the size a 256^3
TSDF fusion leaves (the marching-cubes mesh of such a sphere at 256^3) simplified to 10 000 faces, the target of the
reference's 3_simplify_fusion.py.  Per row: device milliseconds of simplify_meshes (HIP events around the call, the
median, minimum and maximum of `reps` calls after `warmup`; the call's host synchronisations are inside), its rounds, the
launches of its own kernels (the torch sorts and prefix sums between them are not counted), its host synchronisations
(one D2H copy per round, one before the first, one for the new offsets; the boolean gather of the kept vertices waits
once more), faces and vertices before and after, whether every mesh reached its target and stayed watertight.  Alongside:
the same meshes through the clustering decimation (decimate_meshes) at cells 16 and 32, timed the same way."""
import argparse

import numpy as np
import torch

from cost_common import GRID, emit, need_gpu_or_exit, object_grids, placement_draws, timed

PADDING = 0.1


def sphere_mesh(n):
    """the marching-cubes mesh of a dented sphere on an n^3 grid, in the generator's cube -> flat buffers"""
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    ax = torch.arange(n, dtype=torch.float32, device="cuda") - (n - 1) / 2.
    x, y, z = torch.meshgrid(ax, ax, ax, indexing='ij')
    r = torch.sqrt(x * x + y * y + z * z)
    grid = (0.45 * n - r + (n / 32.) * torch.sin((x * 0.7 - y * 0.4 + z) / (n / 12.)))[None].contiguous()
    box = 1 + PADDING
    a = box / (n - 1)
    return marching_cubes_batch(grid, 0., return_flat=True, affine=(a, -1.5 * a - 0.5 * box))


def measure(label, buffers, targets, reps, warmup):
    from rfdnet_amd.iscnet.decimate import decimate_meshes
    from rfdnet_amd.iscnet.simplify import simplify_meshes
    from rfdnet_amd.mesh_sample import is_watertight
    v, f, vend, tend = buffers
    K = len(vend) - 1
    box = 1 + PADDING
    tight = [is_watertight(f[tend[k]:tend[k + 1]]) for k in range(K)]
    row = {"case": label, "meshes": K, "vertices": int(vend[-1]), "faces": int(tend[-1]), "watertight": all(tight),
           "simplify": {}, "decimate": {}}
    for n_faces in targets:
        stats = {}
        out = simplify_meshes(v, f, vend, tend, n_faces, stats=stats)
        cell = {"vertices": int(out[2][-1]), "faces": int(out[3][-1]), "reached": bool(out[4].all()),
                "watertight": all(is_watertight(out[1][out[3][k]:out[3][k + 1]]) for k in range(K)),
                "rounds": stats["rounds"], "launches": stats["launches"], "host_syncs": stats["host_syncs"] + 1}
        cell.update(timed(lambda: simplify_meshes(v, f, vend, tend, n_faces), reps, warmup))
        row["simplify"][str(n_faces)] = cell
    for cells in (16, 32):
        lo, h = np.full((K, 3), -box / 2), np.full(K, box / cells)
        run = lambda: decimate_meshes(v, f, vend, tend, cells, lo=lo, h=h)
        thin = run()
        cell = {"vertices": int(thin[2][-1]), "faces": int(thin[3][-1]),
                "watertight": all(is_watertight(thin[1][thin[3][k]:thin[3][k + 1]]) for k in range(K))}
        cell.update(timed(run, reps, warmup))
        row["decimate"][str(cells)] = cell
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    need_gpu_or_exit("simplify_cost")
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    rng = np.random.default_rng(5)
    placement_draws(rng, 13)                         # the same stream, so the same objects, as decimate_cost
    box = 1 + PADDING
    a = box / (GRID - 1)
    scene = marching_cubes_batch(object_grids(rng, 13), 0., return_flat=True, affine=(a, -1.5 * a - 0.5 * box))
    rows = [measure("scene of 13 meshes at 48^3", scene, (2000, 500), args.reps, args.warmup),
            measure("one model at 256^3", sphere_mesh(256), (10000,), args.reps, args.warmup)]
    emit({"tool": "simplify_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
          "rows": rows}, args.out)


if __name__ == "__main__":
    main()
