#!/usr/bin/env python
"""Vertex normals (csrc/occ_normals.hip) timed against the tail decoder's forward rate, in one process.

Vertex sets: the headline one -- the meshes of one synthetic scene (80 000 points, 256 proposals, MISE 32 -> 64 with
seeded weights: a real generate_mesh) -- and the reference demo's size, 13 meshes x 3 400 vertices (taken from the first
13 headline meshes).  The comparison: the tail decoder (csrc/occ_decoder_tail.hip, chosen with rfd_occ_set_tail_tiles)
evaluating the logits of the same headline vertices, tiled per proposal.

Algorithmic FLOP per vertex: the decoder forward (fc_p 2*3*256, ten 256x256 GEMMs 2*256*256 each, fc_out 2*256 =
1 312 768) twice -- the backward pass has the same ten GEMMs (transposed) plus the 256 -> 3 reduction.

  python tools/normals_bench.py [--iters N] [--out profiles/normals_bench.json]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FWD_FLOP = 2 * 3 * 256 + 10 * 2 * 256 * 256 + 2 * 256          # 1 312 768
NORMALS_FLOP = 2 * FWD_FLOP


def timed(fn, iters, warmup=2):
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
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
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
    with torch.no_grad():
        end_points, feats = net.detect(pc)
        ids = net.select_proposals(end_points, 'all', pc)
        codes = net.object_codes(end_points, feats, ids, pc)
        cls = net.cls_codes(end_points, ids)
        fold = []
        grids = gen.generate_grids(codes, cls, fold_out=fold)
        gen.extract_meshes(grids)
        table, fcp = fold[0]
        v, _, vend, _ = gen.last_buffers
        _lib.device_status()
        V, K = int(vend[-1]), len(vend) - 1

        head_ms, head_min = timed(lambda: dec.normals(v, vend, table, fcp), args.iters)
        _lib.device_status()
        # demo size: 13 meshes x 3400 vertices
        dv = torch.cat([v[vend[k]:vend[k] + 3400] for k in range(13)]).contiguous()
        dend = [0]
        for k in range(13):
            dend.append(dend[-1] + min(3400, vend[k + 1] - vend[k]))
        demo_ms, demo_min = timed(lambda: dec.normals(dv, dend, table[:13].contiguous(), fcp), args.iters)
        _lib.device_status()

        # tail decoder forward over the same vertices, per-proposal tiles
        counts = np.diff(np.asarray(vend))
        tiles = (counts + TILE - 1) // TILE
        pts = torch.zeros(int(tiles.sum()) * TILE, 3, dtype=torch.float32, device="cuda")
        starts = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * TILE
        idx = torch.from_numpy(np.concatenate([s + np.arange(n) for s, n in zip(starts, counts)])).cuda()
        pts[idx] = v.float()
        tile_prop = torch.from_numpy(np.repeat(np.arange(K, dtype=np.int32), tiles)).cuda()
        old = _lib.lib().rfd_occ_set_tail_tiles(1 << 30)
        try:
            tail_ms, tail_min = timed(lambda: dec.decode_tiles(pts, tile_prop, table, fcp), args.iters)
        finally:
            _lib.lib().rfd_occ_set_tail_tiles(old)
        _lib.device_status()

    n_tail = int(tiles.sum()) * TILE
    res = {
        "metric": "vertex normals (decoder input gradient), one launch per vertex set",
        "headline": {"meshes": K, "vertices": V, "ms": round(head_ms, 3), "ms_min": round(head_min, 3),
                     "vertices_per_s": V / head_ms * 1e3, "tflops_algorithmic": V * NORMALS_FLOP / head_ms * 1e-9},
        "demo": {"meshes": 13, "vertices": dend[-1], "ms": round(demo_ms, 4), "ms_min": round(demo_min, 4),
                 "vertices_per_s": dend[-1] / demo_ms * 1e3},
        "tail_decoder_forward": {"points": V, "slots": n_tail, "ms": round(tail_ms, 3),
                                 "points_per_s": V / tail_ms * 1e3,
                                 "tflops_algorithmic": V * FWD_FLOP / tail_ms * 1e-9},
        "flop_per_vertex": NORMALS_FLOP, "flop_per_point_forward": FWD_FLOP, "iters": args.iters,
    }
    res["normals_vs_tail_per_flop"] = res["headline"]["tflops_algorithmic"] / res["tail_decoder_forward"]["tflops_algorithmic"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
