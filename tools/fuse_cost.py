"""Cost of the watertight path on one GPU -- a record, not a test.

    python tools/fuse_cost.py [--out profiles/fuse_cost.json] [--reps 10] [--warmup 2]
                              [--resolution 256] [--views 200] [--image_size 640]

At the reference's size (256^3 voxels, 200 views of 640 x 640) on the depth maps of a real mesh: one of
tools/render_cost.py's dented marching-cubes spheres (48^3, about 18 600 faces), rendered by watertight's own first stage.

  fuse          device milliseconds of rfd_tsdf_fuse (HIP events around the call; the median, minimum and maximum of `reps`
                calls after `warmup`) for every gather strategy: all views in one launch, and one launch per c views with
                sum and count carried through the volume.  Every strategy must give the same bits as the first.
  torch_ops     the same fusion written as torch operations on the same device (one pass of elementwise kernels and one
                gather per view over the whole volume), the yardstick, and how far its field is from the kernel's
  stages        one watertight() call, stage by stage
  pairs_per_s   voxel-view pairs over the fusion's time
The bytes the gather moves need a counter run of its own (rocprofv3 --pmc, nothing else traced); this tool does not
make one and says so."""
import argparse

import numpy as np
import torch

from cost_common import emit, need_gpu_or_exit, real_mesh, timed

STRATEGIES = (0, 1, 2, 4, 8, 25, 50)          # view_chunk: 0 = all views in one launch


def torch_fuse(depth, K, R, T, res, vx_size, truncation, unobserved):
    """rules 1-5 of include/rfd_fuse.h in torch operations (unknown_is_free = False); torch may contract or reorder
    nothing here either, but its division and its fused kernels are its own: a yardstick for time, not for bits"""
    dev = depth.device
    V, rows, cols = depth.shape
    c = ((torch.arange(res, dtype=torch.float64, device=dev) + 0.5) * float(np.float32(vx_size)) - 0.5).float()
    z, y, x = torch.meshgrid(c, c, c, indexing='ij')
    total = torch.zeros(res, res, res, device=dev)
    count = torch.zeros(res, res, res, dtype=torch.int32, device=dev)
    K, R, T = K.cpu().tolist(), R.cpu().tolist(), T.cpu().tolist()
    flat = depth.reshape(V, -1)
    for v in range(V):
        k, r, t = K[v], R[v], T[v]
        xt = ((r[0] * x + r[1] * y) + r[2] * z) + t[0]
        yt = ((r[3] * x + r[4] * y) + r[5] * z) + t[1]
        zt = ((r[6] * x + r[7] * y) + r[8] * z) + t[2]
        dd = (k[6] * xt + k[7] * yt) + k[8] * zt
        tu = ((k[0] * xt + k[1] * yt) + k[2] * zt) / dd + 0.5
        tv = ((k[3] * xt + k[4] * yt) + k[5] * zt) / dd + 0.5
        on = (tu > -1) & (tu < cols) & (tv > -1) & (tv < rows)
        pix = torch.where(on, tv.to(torch.int64) * cols + tu.to(torch.int64), 0)
        g = flat[v][pix.reshape(-1)].reshape(res, res, res)
        dist = g - dd
        valid = on & (g > 0) & (dist >= -truncation)
        total = torch.where(valid, total + dist.clamp(-truncation, truncation), total)
        count += valid
    return torch.where(count > 0, total / count.clamp(min=1), torch.full_like(total, unobserved)), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--image_size", type=int, default=640)
    args = ap.parse_args()
    need_gpu_or_exit("fuse_cost")
    from rfdnet_amd import watertight as wt
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    res, V, S = args.resolution, args.views, args.image_size
    focal, voxel = float(S), 1. / res
    truncation, offset = 10 * voxel, np.float32(1.5 * voxel)
    v, f = real_mesh()
    rot = wt.views_on_sphere(V)
    K = np.tile(np.float32([focal, 0, S / 2., 0, focal, S / 2., 0, 0, 1]), (V, 1))
    T = np.tile(np.float32([0, 0, 1]), (V, 1))
    dev = v.device
    Kd, Rd, Td = (torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(V, -1)).to(dev) for a in (K, rot, T))

    # ---- the stages of one watertight() call, each between its own pair of events
    state = {}

    def normalise():
        centre, scale = wt.normalisation(v.double(), 0.1)
        state.update(centre=centre, scale=scale, unit=((v.double() - centre) / scale).float().contiguous(),
                     faces=f.to(torch.int32).contiguous())

    def render():
        state["depth"] = wt.render_depthmaps(state["unit"], state["faces"], rot, S, focal, (0.25, 1.75), offset)

    def fuse(chunk=0):
        state["tsdf"] = wt.fuse_depthmaps(state["depth"], Kd, Rd, Td, res, truncation, voxel_size=voxel,
                                          unobserved='+truncation', view_chunk=chunk)

    def extract():
        state["mesh"] = marching_cubes_batch((-state["tsdf"].permute(2, 1, 0))[None], 0., pad_value=-1e6)[0]

    def back():
        state["out"] = ((state["mesh"][0] - 1.) / res - 0.5) * state["scale"] + state["centre"]
    stages = {}
    for name, fn in (("normalise", normalise), ("render_depthmaps", render), ("fuse_depthmaps", fuse),
                     ("marching_cubes", extract), ("map_back", back)):
        stages[name] = timed(fn, max(args.reps // 2, 1), 1)
    whole = timed(lambda: wt.watertight(v, f, resolution=res, n_views=V, image_size=S, focal=focal), max(args.reps // 2, 1), 1)
    depth = state["depth"]
    pairs = float(res) ** 3 * V

    # ---- the gather strategies, alternating, each checked against the first
    first, rows = None, []
    for chunk in STRATEGIES:
        if chunk >= V and chunk:
            continue
        got = wt.fuse_depthmaps(depth, Kd, Rd, Td, res, truncation, voxel_size=voxel, unobserved='+truncation',
                                return_count=True, view_chunk=chunk)
        first = got if first is None else first
        row = {"view_chunk": chunk, "launches": 1 if chunk == 0 else -(-V // chunk),
               "same_bits_as_one_launch": bool(torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]))}
        row.update(timed(lambda: wt.fuse_depthmaps(depth, Kd, Rd, Td, res, truncation, voxel_size=voxel,
                                                   unobserved='+truncation', return_count=True, view_chunk=chunk),
                         args.reps, args.warmup))
        row["pairs_per_s"] = pairs / (row["ms"] * 1e-3)
        rows.append(row)
    second_pass = [dict(view_chunk=r["view_chunk"], **timed(
        lambda c=r["view_chunk"]: wt.fuse_depthmaps(depth, Kd, Rd, Td, res, truncation, voxel_size=voxel,
                                                    unobserved='+truncation', return_count=True, view_chunk=c),
        args.reps, 1)) for r in rows]

    # ---- the yardstick
    ref, ref_count = torch_fuse(depth, Kd, Rd, Td, res, voxel, truncation, truncation)
    yard = timed(lambda: torch_fuse(depth, Kd, Rd, Td, res, voxel, truncation, truncation), max(args.reps // 3, 2), 1)
    yard.update(pairs_per_s=pairs / (yard["ms"] * 1e-3),
                voxels_with_another_count=int((ref_count != first[1]).sum()),
                voxels_with_other_bits=int((ref != first[0]).sum()),
                max_abs_difference=float((ref - first[0]).abs().max()))

    result = {"tool": "fuse_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "resolution": res, "views": V, "image_size": S, "voxel_view_pairs": pairs,
              "depth_stack_bytes": int(depth.numel() * 4), "volume_bytes_sum_and_count": int(res ** 3 * 8),
              "mesh": {"vertices": int(v.shape[0]), "faces": int(f.shape[0]),
                       "observed_voxels": float((first[1] > 0).float().mean()),
                       "watertight_vertices": int(state["mesh"][0].shape[0]), "watertight_faces": int(state["mesh"][1].shape[0])},
              "fuse": rows, "fuse_second_pass": second_pass, "torch_ops": yard, "stages": stages, "watertight_call": whole,
              "gather_bytes": "not measured: needs a counter run of its own"}
    emit(result, args.out)


if __name__ == "__main__":
    main()
