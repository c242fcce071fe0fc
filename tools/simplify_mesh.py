"""Step 3 of the ShapeNet preparation on the device: simplify a watertight mesh to a face budget (the reference's
utils/shapenet/3_simplify_fusion.py: quadric edge collapse to 10 000 faces, topology and normals preserved).

    python tools/simplify_mesh.py IN.off OUT.off [--n_faces 10000] [--report_error [--error_samples 10000]]

Reads .off / .obj / .ply through the shared mesh reader, simplifies with rfdnet_amd.iscnet.simplify (quadric edge
collapse in parallel rounds, link condition and flip guard) and checks the result with mesh_sample.is_watertight; if it is
not watertight the input is written instead, and the JSON line says so (3_simplify_fusion.py:74-80).  Steps 1 and 2 are
tools/make_watertight.py and tools/sample_mesh.py.  Prints one JSON line with the counts; --report_error adds
"rms_error": the two-sided RMS of the exact distances between the input and what was written (samples on each surface
against the other mesh, rfdnet_amd/mesh_distance.py)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--n_faces", type=int, default=10000)
    ap.add_argument("--report_error", action="store_true",
                    help="add the two-sided RMS distance of the input against what is written, computed on the device")
    ap.add_argument("--error_samples", type=int, default=10000)
    return ap


def two_sided_rms(v_in, f_in, v_out, f_out, samples, seed=0):
    """the exact two-sided RMS distance of two meshes on the device (rfdnet_amd.mesh_distance.mesh_metrics' `rms`)"""
    from rfdnet_amd.mesh_distance import MeshDistance, mesh_metrics
    gen = torch.Generator(device=v_in.device).manual_seed(seed)
    m = mesh_metrics(MeshDistance(v_in, f_in), MeshDistance(v_out, f_out), [[0, 0]], samples, generator=gen)
    return float(m['rms'][0])


def choose(v_in, f_in, v_out, f_out):
    """the reference's fallback: the simplified mesh if it is watertight, the input otherwise -> ((v, f), report)"""
    from rfdnet_amd.mesh_sample import is_watertight
    tight = is_watertight(f_out)
    report = {"faces_in": int(f_in.shape[0]), "faces_out": int(f_out.shape[0]), "vertices_in": int(v_in.shape[0]),
              "vertices_out": int(v_out.shape[0]), "watertight": tight, "fallback": not tight}
    return ((v_out, f_out) if tight else (v_in, f_in)), report


def main():
    args = build_parser().parse_args()
    if args.n_faces < 0:
        raise SystemExit("--n_faces must be >= 0")
    if not torch.cuda.is_available():
        raise SystemExit("simplify_mesh runs on a GPU: none is visible")
    from rfdnet_amd import io
    from rfdnet_amd.iscnet.simplify import simplify_meshes
    if os.path.splitext(args.input)[1].lower() not in (".off", ".obj", ".ply"):
        raise SystemExit("simplify_mesh reads .off, .obj and .ply, not %s" % args.input)
    v, f = io.read_mesh(args.input)
    if not len(v) or not len(f):
        raise SystemExit("%s holds no triangles" % args.input)
    dev = torch.device("cuda")
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    stats = {}
    v2, f2, _, _, reached = simplify_meshes(vt, ft, [0, vt.shape[0]], [0, ft.shape[0]], args.n_faces, stats=stats)
    (vo, fo), report = choose(vt, ft, v2, f2)
    report.update(tool="simplify_mesh", n_faces=args.n_faces, reached=bool(reached[0]), rounds=stats["rounds"])
    if report["fallback"]:
        print("simplify_mesh: the result is not watertight; writing the input instead", file=sys.stderr)
    if args.report_error:
        report.update(rms_error=two_sided_rms(vt, ft, vo, fo, args.error_samples), error_samples=args.error_samples)
    io.write_off(args.output, vo.double().cpu().numpy(), fo.cpu().numpy())
    print(json.dumps(report))


if __name__ == "__main__":
    main()
