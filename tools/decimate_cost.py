"""Cost of the mesh decimation on one GPU -- a record, not a test.

    python tools/decimate_cost.py [--out profiles/decimate_cost.json] [--reps 20] [--warmup 3]

The two scenes of tools/render_cost.py (13 and 256 marching-cubes meshes of dented spheres at 48^3, about 18 600 faces
each, here in the generator's cube), decimated with cells = 16 and 32.  Per scene and grid: device milliseconds of
decimate_meshes (HIP events around the call, the median, minimum and maximum of `reps` calls after `warmup`; the call
holds three small host synchronisations, which the events include), vertices and faces before and after, and one
refinement step (Generator3D.refine_meshes with weights drawn on the device, seeded network and codes: the time of a
two-step call minus that of a one-step call, so the once-per-call set-up cancels) on the full and on the decimated
meshes.  Beside them the marching-cubes extraction of the same scene, timed the same way."""
import argparse

import numpy as np
import torch

from cost_common import GRID, emit, need_gpu_or_exit, object_grids, placement_draws, timed

PADDING = 0.1


def refine_step_ms(gen, buffers, fold, reps, warmup):
    v, f, vend, tend = buffers
    if tend[-1] == 0:
        return None
    one = timed(lambda: gen.refine_meshes(v, f, vend, tend, fold, 1), reps, warmup)
    two = timed(lambda: gen.refine_meshes(v, f, vend, tend, fold, 2), reps, warmup)
    return {"ms": two["ms"] - one["ms"], "ms_call_1_step": one["ms"], "ms_call_2_steps": two["ms"]}


def measure(label, n_obj, onet, reps, warmup):
    from rfdnet_amd import _lib
    from rfdnet_amd.iscnet.decimate import decimate_meshes
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    rng = np.random.default_rng(5)
    placement_draws(rng, n_obj)                      # the same stream, so the same objects, as render_cost
    grids = object_grids(rng, n_obj)
    box = 1 + PADDING
    a = box / (GRID - 1)
    extract = lambda: marching_cubes_batch(grids, 0., return_flat=True, affine=(a, -1.5 * a - 0.5 * box))
    full = extract()
    gen, dec = onet.generator, onet.decoder
    code_rng = np.random.default_rng(7)
    with torch.no_grad():
        fold = dec.fold(torch.zeros(n_obj, onet.z_dim, device="cuda"),
                        torch.from_numpy(code_rng.normal(0, 1, (n_obj, 512)).astype(np.float32)).cuda())
    row = {"scene": label, "objects": n_obj, "grid": GRID, "vertices": int(full[2][-1]),
           "faces": int(full[3][-1]), "marching_cubes": timed(extract, reps, warmup),
           "refine_step_full": refine_step_ms(gen, full, fold, reps, warmup), "cells": {}}
    for cells in (16, 32):
        lo, h = np.full((n_obj, 3), -box / 2), np.full(n_obj, box / cells)
        run = lambda: decimate_meshes(full[0], full[1], full[2], full[3], cells, lo=lo, h=h)
        thin = run()
        row["cells"][str(cells)] = {"vertices": int(thin[2][-1]), "faces": int(thin[3][-1]),
                                    "decimate_meshes": timed(run, reps, warmup),
                                    "refine_step_decimated": refine_step_ms(gen, thin, fold, reps, warmup)}
    row["status_bits"] = _lib.stream_status_bits()               # the decoder's f16-range flag, if random codes raised it
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    need_gpu_or_exit("decimate_cost")
    from rfdnet_amd import synthetic
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.occupancy_net import ONet
    onet = ONet(Config({}))
    synthetic.load_seeded(onet, 10)
    onet = onet.cuda().eval()
    onet.generator.set_refinement(0, eps_source='device', seed=1)
    rows = [measure("demo-sized", 13, onet, args.reps, args.warmup),
            measure("headline", 256, onet, args.reps, args.warmup)]
    result = {"tool": "decimate_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "rows": rows}
    emit(result, args.out)


if __name__ == "__main__":
    main()
