"""Cost of the completion loss of the test mode on one GPU: Encoder_Latent.forward, the whole ONet.compute_loss, and the
reference module's own torch ops (encoder_latent.py:49-73 as nn.Linear / relu / max / cat on the same device), at
K = 64 and K = 256 proposals of T = 2048 points.

    python tools/completion_cost.py [--out profiles/completion_eval.json] [--reps 20]

Each figure is device milliseconds per call (HIP events around `reps` calls in a row after a warm-up of every shape, the
median of five such windows) with the number of kernel launches through the library's C ABI beside it (the torch
composition's launches are torch's own and are counted from the profiler-free op list: 8 linear layers, 3 relu, 3 max,
2 expand + cat, 3 adds).  Also the largest difference between the two encoders' outputs, so that "faster" is about the same
numbers.  Seeded weights (synthetic.load_seeded): the cost does not depend on them."""
import argparse
import json
import os

import numpy as np
import torch

from cost_common import ROOT, device_ms

TORCH_OPS_OF_THE_MODULE = 8 + 3 + 3 + 2 * 2 + 3


def torch_encoder(enc, p, x, c):
    """the module's forward as the reference writes it, on the parameters of `enc`"""
    lin = torch.nn.functional.linear
    net = lin(x.unsqueeze(-1), enc.fc_0.weight, enc.fc_0.bias) + lin(p, enc.fc_pos.weight, enc.fc_pos.bias)
    net = net + lin(c, enc.fc_c.weight, enc.fc_c.bias).unsqueeze(1)
    net = lin(torch.relu(net), enc.fc_1.weight, enc.fc_1.bias)
    for fc in (enc.fc_2, enc.fc_3):
        pooled = net.max(dim=1, keepdim=True)[0].expand(net.size())
        net = lin(torch.relu(torch.cat([net, pooled], dim=2)), fc.weight, fc.bias)
    net = net.max(dim=1)[0]
    return lin(net, enc.fc_mean.weight, enc.fc_mean.bias), lin(net, enc.fc_logstd.weight, enc.fc_logstd.bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "completion_eval.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=2048)
    args = ap.parse_args()
    from rfdnet_amd import _lib, synthetic
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.occupancy_net import ONet
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    onet = ONet(Config({'data': {'latent_encoder': True}, 'generation': {'resolution_0': 16}}))
    synthetic.load_seeded(onet, 202)
    onet = onet.cuda().eval()
    enc = onet.encoder_latent
    calls = []
    call = _lib.call
    _lib.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
    rows = []
    with torch.no_grad():
        for K in (64, 256):
            rng = np.random.default_rng(K)
            T = args.points
            p = torch.from_numpy(rng.uniform(-0.55, 0.55, (K, T, 3)).astype(np.float32)).cuda()
            occ = (p.pow(2).sum(-1) <= 0.35 ** 2).float()
            c = torch.from_numpy(rng.normal(0, 1, (K, 512)).astype(np.float32)).cuda()
            eps = torch.from_numpy(rng.normal(0, 1, (K, 32)).astype(np.float32)).cuda()
            mine, ref = enc(p, occ, c), torch_encoder(enc, p, occ, c)
            diff = max(float((a - b).abs().max()) for a, b in zip(mine, ref))
            del calls[:]
            enc(p, occ, c)
            n_enc = len(calls)
            del calls[:]
            onet.compute_loss(c, p, occ, None, export_shape=True, eps=eps)
            n_loss = len(calls)
            row = {"K": K, "T": T, "encoder_vs_torch_max_abs_diff": diff,
                   "encoder_forward": dict(zip(("ms", "ms_min", "ms_max"), device_ms(lambda: enc(p, occ, c), args.reps)),
                                           abi_launches=n_enc),
                   "compute_loss_with_voxels": dict(zip(("ms", "ms_min", "ms_max"), device_ms(
                       lambda: onet.compute_loss(c, p, occ, None, export_shape=True, eps=eps), max(args.reps // 4, 1))),
                       abi_launches=n_loss, note="two decoder calls, each with its status read (a stream wait)"),
                   "torch_ops_of_the_reference_module": dict(zip(("ms", "ms_min", "ms_max"), device_ms(
                       lambda: torch_encoder(enc, p, occ, c), args.reps)), torch_ops=TORCH_OPS_OF_THE_MODULE)}
            rows.append(row)
    line = {"tool": "completion_cost", "device": torch.cuda.get_device_name(0), "reps_per_window": args.reps,
            "windows": 5, "rows": rows}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
