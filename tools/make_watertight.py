"""A watertight mesh from any triangle soup, on one GPU (rfdnet_amd.watertight: the reference's
utils/shapenet/1_fuse_shapenetv2.py, and with --decimate_cells the place of its 3_simplify_fusion.py).

    python tools/make_watertight.py IN.{off,obj,ply} OUT.off [--resolution 256] [--views 200] [--image_size 640]
                                    [--keep_components largest|T [--drop_cavities]] [--decimate_cells N]

The focal length is the image size, as in the reference (640 at 640 x 640).  --decimate_cells N thins the result with the
device decimation (rfdnet_amd.iscnet.decimate) on a grid of N^3 cells over the mesh's bounding cube.  --keep_components
drops the fused mesh's floaters before that (rfdnet_amd.iscnet.components): `largest` keeps the largest connected
component alone, a fraction T every component with at least T times the largest's area; --drop_cavities also drops
inside-out inner shells.  Prints one JSON line: the counts of what was read and what was written."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def keep_components_arg(text):
    if text == 'largest':
        return text
    t = float(text)
    if not 0.0 <= t <= 1.0:
        raise argparse.ArgumentTypeError("largest, or a fraction in [0, 1]")
    return t


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--image_size", type=int, default=640)
    ap.add_argument("--decimate_cells", type=int, default=0)
    ap.add_argument("--keep_components", type=keep_components_arg, default=None, metavar="largest|T")
    ap.add_argument("--drop_cavities", action="store_true")
    return ap


def main():
    args = build_parser().parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("make_watertight runs on a GPU: none is visible")
    from rfdnet_amd import io
    from rfdnet_amd.watertight import watertight
    if os.path.splitext(args.input)[1].lower() not in (".off", ".obj", ".ply"):
        raise SystemExit("make_watertight reads .off, .obj and .ply, not %s" % args.input)
    v, f = io.read_mesh(args.input)
    if not len(v) or not len(f):
        raise SystemExit("%s holds no triangles" % args.input)
    dev = torch.device("cuda")
    vt, ft = watertight(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), resolution=args.resolution,
                        n_views=args.views, image_size=args.image_size, focal=float(args.image_size))
    result = {"tool": "make_watertight", "input": {"vertices": int(len(v)), "faces": int(len(f))},
              "watertight": {"vertices": int(vt.shape[0]), "faces": int(ft.shape[0])}}
    if (args.keep_components is not None or args.drop_cavities) and ft.shape[0]:
        from rfdnet_amd.iscnet.components import keep_components
        keep = 0.0 if args.keep_components is None else args.keep_components      # --drop_cavities alone: the rest stays
        vt, ft, _, _, info = keep_components(vt, ft, [0, vt.shape[0]], [0, ft.shape[0]], keep=keep,
                                             drop_cavities=args.drop_cavities, return_info=True)
        result["components"] = {"found": info["found"][0], "kept": info["kept"][0]}
        result["kept"] = {"vertices": int(vt.shape[0]), "faces": int(ft.shape[0])}
    if args.decimate_cells and ft.shape[0]:
        from rfdnet_amd.iscnet.decimate import decimate_meshes
        lo, hi = vt.amin(0).cpu().numpy(), vt.amax(0).cpu().numpy()
        side = float((hi - lo).max()) * (1 + 1e-6)                     # the highest vertex stays inside the last cell
        vt, ft, _, _ = decimate_meshes(vt, ft, [0, vt.shape[0]], [0, ft.shape[0]], args.decimate_cells,
                                       lo=(lo + hi) / 2 - side / 2, h=side / args.decimate_cells)
        result["decimated"] = {"cells": args.decimate_cells, "vertices": int(vt.shape[0]), "faces": int(ft.shape[0])}
    io.write_off(args.output, vt.double().cpu().numpy(), ft.cpu().numpy())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
