#!/usr/bin/env python
"""Mesh refinement (Generator3D.refine_meshes: csrc/mesh_refine.hip around the decoder's value and gradient kernels): device
time per step, and beside it the time of the step's two decoder launches alone.

Meshes: those of one synthetic headline scene (80 000 points, 256 proposals, MISE 32 -> 64 with seeded weights: a real
generate_mesh), all K = 256 of them and the first K = 13 (the reference demo's proposal count).  Weights are drawn on the device
(eps_source='device': a host draw for 13 M faces would dominate the wall time and is not what is measured).

Per-step time = (time of 2 N steps - time of N steps) / N, HIP events around the whole call: the once-per-call work (the
vertex -> corner CSR, buffers) cancels.  The decoder launches alone: rfd_occ_decode_w8 on the loop's tiled sample points +
rfd_occ_normals_w8 on its compact ones.  What the three small kernels (and the weight draw) add is the difference; what a fused
value + gradient kernel could save is at most the forward pass the normals kernel repeats: one decoder pass of three.

  python tools/refine_bench.py [--steps N] [--iters M] [--out profiles/refine_bench.json]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from rfdnet_amd import _lib, synthetic
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.network import ISCNet
    from rfdnet_amd.iscnet.occ_decoder import TILE

    cfg = Config({'data': {'num_point': 80000}, 'generation': {'resolution_0': 32, 'upsampling_steps': 1}})
    net = ISCNet(cfg)
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=10, n_points=80000, n_raw=120000)[None]).cuda()
    gen, dec = net.completion.generator, net.completion.decoder
    gen.set_refinement(0, eps_source='device', seed=1)
    res = {"metric": "mesh refinement, device ms per step (all meshes of the set in one loop)", "steps": args.steps,
           "iters": args.iters, "sets": {}}
    with torch.no_grad():
        end_points, feats = net.detect(pc)
        ids = net.select_proposals(end_points, 'all', pc)
        codes = net.object_codes(end_points, feats, ids, pc)
        cls = net.cls_codes(end_points, ids)
        fold = []
        grids = gen.generate_grids(codes, cls, fold_out=fold)
        gen.extract_meshes(grids)
        table, fcp = fold[0]
        v, f, vend, tend = gen.last_buffers
        _lib.device_status()
        for K in (13, len(vend) - 1):
            ve, te = vend[:K + 1], tend[:K + 1]
            V, F = int(ve[-1]), int(te[-1])
            tab = table[:K].contiguous()
            n = args.steps
            t1 = timed(lambda: gen.refine_meshes(v, f, ve, te, (tab, fcp), n), args.iters)
            t2 = timed(lambda: gen.refine_meshes(v, f, ve, te, (tab, fcp), 2 * n), args.iters)
            _lib.device_status()
            # the two decoder launches of a step, alone, on face barycentres laid out as the loop lays its samples out
            counts = np.diff(np.asarray(te))
            tiles = (counts + TILE - 1) // TILE
            first = torch.repeat_interleave(torch.as_tensor(np.asarray(ve[:-1])).cuda(), torch.as_tensor(counts).cuda())
            q = v[:V].float()[(f[:F].long() + first[:, None])].mean(1)
            starts = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * TILE
            slot = torch.from_numpy(np.concatenate([s + np.arange(c) for s, c in zip(starts, counts)])).cuda()
            qt = torch.zeros(int(tiles.sum()) * TILE, 3, dtype=torch.float32, device="cuda")
            qt[slot] = q
            qd = q.double().contiguous()
            tile_prop = torch.from_numpy(np.repeat(np.arange(K, dtype=np.int32), tiles)).cuda()
            t_dec = timed(lambda: dec.decode_tiles(qt, tile_prop, tab, fcp), args.iters)
            t_nrm = timed(lambda: dec.normals(qd, te, tab, fcp, return_grad=True), args.iters)
            _lib.device_status()
            step = (t2 - t1) / n
            res["sets"]["K%d" % K] = {
                "meshes": K, "vertices": V, "faces": F, "ms_per_step": round(step, 4),
                "ms_call_%d_steps" % n: round(t1, 3), "ms_call_%d_steps" % (2 * n): round(t2, 3),
                "ms_decode_alone": round(t_dec, 4), "ms_gradient_alone": round(t_nrm, 4),
                "decoder_share_of_step": round((t_dec + t_nrm) / step, 4),
                "ms_added_by_small_kernels": round(step - t_dec - t_nrm, 4),
                "fused_value_gradient_could_save_at_most_ms": round(t_dec, 4),
                "faces_per_s": F / step * 1e3}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
