"""What the completion network trains and is scored on, from one watertight mesh, on one GPU (rfdnet_amd.mesh_sample: the
reference's utils/shapenet/2_sample_mesh.py).  It chains behind tools/make_watertight.py.

    python tools/sample_mesh.py IN.{off,obj} --out DIR [--resize] [--pointcloud_size 100000] [--points_size 100000]
                                [--points_uniform_ratio 0.5] [--points_sigma 0.01] [--points_padding 0.1]
                                [--voxels_res 16] [--float16] [--packbits] [--seed 0]

Writes into DIR: pointcloud.npz (surface points and normals), points.npz (query points with inside / outside labels),
voxels_<res>.binvox (surface OR interior voxels) and NAME.off (the mesh as sampled).  --resize moves the mesh into the unit
cube first: loc = the centre of its bounding box, scale = its largest extent (both are stored in every file).  Points and
voxels need a closed mesh: where an edge does not lie in exactly two faces, the tool warns and writes the point cloud and
the mesh only.  The defaults are the reference's.  Prints one JSON line: what was written."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("--out", required=True)
    ap.add_argument("--resize", action="store_true")
    ap.add_argument("--pointcloud_size", type=int, default=100000)
    ap.add_argument("--points_size", type=int, default=100000)
    ap.add_argument("--points_uniform_ratio", type=float, default=0.5)
    ap.add_argument("--points_sigma", type=float, default=0.01)
    ap.add_argument("--points_padding", type=float, default=0.1)
    ap.add_argument("--voxels_res", type=int, nargs="+", default=[16])
    ap.add_argument("--float16", action="store_true")
    ap.add_argument("--packbits", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if os.path.splitext(args.input)[1].lower() not in (".off", ".obj"):
        raise SystemExit("sample_mesh reads .off and .obj, not %s" % args.input)
    if not torch.cuda.is_available():
        raise SystemExit("sample_mesh runs on a GPU: none is visible")
    from rfdnet_amd import io, mesh_sample
    v, f = io.read_mesh(args.input)
    if not len(v) or not len(f):
        raise SystemExit("%s holds no triangles" % args.input)
    loc, scale = np.zeros(3), 1.
    if args.resize:
        v, loc, scale = mesh_sample.unit_cube(torch.from_numpy(v))
        v, loc = v.numpy(), loc.numpy()
    dev = torch.device("cuda")
    vt, ft = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev), torch.from_numpy(f).to(dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    os.makedirs(args.out, exist_ok=True)
    written = []

    def out(name):
        written.append(name)
        return os.path.join(args.out, name)

    # the generator's draws, in this order: the voxels' jitter, the point cloud, the query points
    closed = mesh_sample.is_watertight(ft)
    if not closed:
        print("Warning: %s is not watertight: no points, no voxels" % args.input, file=sys.stderr)
    else:
        for res in args.voxels_res:
            grid = mesh_sample.voxelize_ray(vt, ft, res, generator=gen)
            io.write_binvox(out("voxels_%d.binvox" % res), grid.cpu().numpy(), loc, scale)
    points, _, normals = mesh_sample.sample_surface(vt, ft, args.pointcloud_size, generator=gen, return_normals=True,
                                                    dtype=torch.float64)
    io.write_pointcloud_npz(out("pointcloud.npz"), points.cpu().numpy(), normals.cpu().numpy(), loc, scale, args.float16)
    if closed:
        points, occ = mesh_sample.sample_points(vt, ft, args.points_size, args.points_uniform_ratio, args.points_sigma,
                                                args.points_padding, generator=gen)
        io.write_points_npz(out("points.npz"), points.cpu().numpy(), occ.cpu().numpy(), loc, scale, args.float16,
                            args.packbits)
    io.write_off(out(os.path.splitext(os.path.basename(args.input))[0] + ".off"), v, f)
    print(json.dumps({"tool": "sample_mesh", "vertices": int(len(v)), "faces": int(len(f)), "watertight": closed,
                      "loc": [float(x) for x in loc], "scale": scale, "written": written}))


if __name__ == "__main__":
    main()
