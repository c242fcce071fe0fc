"""Cost of the connected-component stage on one GPU -- a record, not a test.

    python tools/components_cost.py [--out profiles/components_cost.json] [--reps 20] [--warmup 3]

The meshes of one synthetic headline scene (80 000 points, 256 proposals, MISE 32 -> 64 with seeded weights: a real
generate_grids, as tools/refine_bench.py takes them).  Per stage of keep_components(keep='largest', measure='area') -- label
(union-find, flatten, roots, labels), measure (two groupings, the sixteen-lane sums), select (selection, flags), compact
(offsets, faces, vertices) -- and for the whole call: device milliseconds (HIP events around the stage, the median, minimum
and maximum of `reps` runs after `warmup`; a stage's host read-back is inside its events), the launches of the stage's own
kernels (the torch sorts and prefix sums between them are not counted) and its host read-backs (counted, not claimed:
Tensor.cpu is wrapped for one run).  Beside them, timed the same way in the same run: the batched marching cubes of the
scene's grids, and the scene's whole reconstruction (detection, selection, skip propagation, completion, extraction) with
the switch off and with set_components('largest')."""
import argparse

import torch

from cost_common import emit, need_gpu_or_exit, timed


def counted(fn):
    """one run of fn -> (its result, launches of the library's kernels, Tensor.cpu calls)"""
    from rfdnet_amd import _lib
    names, copies = [], []
    call, cpu = _lib.call, torch.Tensor.cpu

    def counting_call(name, *args):
        names.append(name)
        return call(name, *args)

    def counting_cpu(self, *args, **kw):
        copies.append(1)
        return cpu(self, *args, **kw)
    _lib.call, torch.Tensor.cpu = counting_call, counting_cpu
    try:
        out = fn()
    finally:
        _lib.call, torch.Tensor.cpu = call, cpu
    return out, len(names), len(copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    need_gpu_or_exit("components_cost")
    from rfdnet_amd import _lib, synthetic
    from rfdnet_amd.iscnet import components as C
    from rfdnet_amd.iscnet.config import Config
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    from rfdnet_amd.iscnet.network import ISCNet

    net = ISCNet(Config({'data': {'num_point': 80000}, 'generation': {'resolution_0': 32, 'upsampling_steps': 1}}))
    synthetic.load_seeded(net, 10)
    net = net.cuda().eval()
    pc = torch.from_numpy(synthetic.synthetic_scene(seed=10, n_points=80000, n_raw=120000)[None]).cuda()
    gen = net.completion.generator

    def scene():
        with torch.no_grad():
            end_points, feats = net.detect(pc)
            ids = net.select_proposals(end_points, 'all', pc)
            return net.reconstruct(end_points, feats, ids, pc)

    with torch.no_grad():
        end_points, feats = net.detect(pc)
        ids = net.select_proposals(end_points, 'all', pc)
        grids = gen.generate_grids(net.object_codes(end_points, feats, ids, pc), net.cls_codes(end_points, ids))
    _lib.device_status()
    n = grids.shape[1]
    box = 1 + gen.padding
    a = box / (n - 1)
    extract = lambda: marching_cubes_batch(grids, gen.logit_threshold(), pad_value=-1e6, return_flat=True,
                                           affine=(a, -1.5 * a - 0.5 * box))
    v, f, vend, tend = extract()
    vend, tend, K, V, F = C._batch(f, vend, tend)
    by, (largest_only, t) = C.parse_measure('area'), C.parse_keep('largest')
    label = lambda: C._label(f, vend, tend, K, V, F)
    lab = label()
    measure = lambda: C._measure(v, lab, F, V)
    measures = measure()
    select = lambda: C._select(lab, measures, K, F, V, by, largest_only, t, False)
    flags = select()
    compact = lambda: C._compact(v, lab, flags, K, F, V)
    whole = lambda: C.keep_components(v, f, vend, tend, keep='largest', measure='area', return_info=True)
    stages = {}
    for name, fn in (("label", label), ("measure", measure), ("select", select), ("compact", compact), ("total", whole)):
        out, launches, read_backs = counted(fn)
        stages[name] = dict(timed(fn, args.reps, args.warmup), launches=launches, host_read_backs=read_backs)
    info = out[4]
    result = {"tool": "components_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "scene": {"points": 80000, "proposals": K, "grid": int(n), "vertices": V, "faces": F,
                        "components": int(lab['C']), "meshes_with_floaters": sum(1 for c in info['found'] if c > 1),
                        "vertices_kept": int(out[2][-1]), "faces_kept": int(out[3][-1])},
              "keep_components": stages, "marching_cubes": timed(extract, args.reps, args.warmup)}
    reps, warmup = max(3, args.reps // 4), min(args.warmup, 2)
    gen.set_components(None)
    result["reconstruction_off"] = timed(scene, reps, warmup)
    gen.set_components('largest')
    result["reconstruction_largest"] = timed(scene, reps, warmup)
    gen.set_components(None)
    result["status_bits"] = _lib.stream_status_bits()
    emit(result, args.out)


if __name__ == "__main__":
    main()
