"""Cost of the mesh distance metrics on one GPU -- a record, not a test.

    python tools/mesh_dist_cost.py [--out profiles/mesh_dist_cost.json] [--reps 20] [--warmup 3] [--scenes demo-sized,headline]

The two scenes of tools/render_cost.py (13 and 256 marching-cubes objects of about 18 600 faces each, placed in the
synthetic scene's boxes) against themselves moved by 2 cm along x, 10 000 samples per object in both directions.  Timed
apart, between HIP events, the median, minimum and maximum of `reps` calls after `warmup`: the build (valid faces, frames,
cell lists of both sides), the samples, the queries of both directions, and the sums.  Beside them the same queries at
cells=1 (every face of the object for every point: `--brute_reps` calls after one, it is slow), and the nearest-VERTEX
search of chamfer_distance.nearest on the same points (one call per object and direction, float32), which is what the
tree had before and is not the distance to the surface."""
import argparse

import torch

from cost_common import emit, need_gpu_or_exit, scene_inputs, timed

COUNT = 10000
SHIFT = 0.02


def measure(label, n_obj, reps, warmup, brute_reps):
    from rfdnet_amd import mesh_distance as md
    from rfdnet_amd.chamfer_distance import nearest
    from rfdnet_amd.iscnet.scene import place_objects
    meshes, ids, parsed, _ = scene_inputs(n_obj)
    A = place_objects(meshes, ids, parsed)
    moved = dict(parsed, pred_corners_3d_upright_camera=parsed['pred_corners_3d_upright_camera'] +
                 torch.tensor([SHIFT, 0., 0.], dtype=torch.float64, device="cuda"))
    B = place_objects(meshes, ids, moved)
    gen = torch.Generator(device="cuda").manual_seed(0)
    K = n_obj
    u_a, u_b = (torch.rand(K, COUNT, 3, dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
    da, db = md.MeshDistance(A), md.MeshDistance(B)
    sa, _, na = md.sample_surface_ragged(da, COUNT, u_a)
    sb, _, nb = md.sample_surface_ragged(db, COUNT, u_b)
    obj = torch.arange(K, device="cuda").repeat_interleave(COUNT)
    pa, pb = sa.reshape(-1, 3), sb.reshape(-1, 3)
    seg = torch.arange(K + 1, dtype=torch.int32, device="cuda") * COUNT

    def queries(x, y):
        return x._query(pb, obj), y._query(pa, obj)
    (d2_ba, f_ba), (d2_ab, f_ab) = queries(da, db)

    def sums():
        md.segment_sums(db, seg, d2_ab, f_ab, na, (0.05, 0.10))
        md.segment_sums(da, seg, d2_ba, f_ba, nb, (0.05, 0.10))
    brute_a, brute_b = md.MeshDistance(A, cells=1), md.MeshDistance(B, cells=1)
    off = A.obj_off.cpu().tolist()
    va = [A.vertices[off[k]:off[k + 1]][None] for k in range(K)]
    vb = [B.vertices[off[k]:off[k + 1]][None] for k in range(K)]
    fa, fb = sa.float(), sb.float()

    def vertex_search():
        for k in range(K):
            nearest(fa[k][None], vb[k])
            nearest(fb[k][None], va[k])
    metrics = md.mesh_metrics(da, db, [[k, k] for k in range(K)], COUNT, u_a=u_a, u_b=u_b)
    return {"scene": label, "objects": K, "faces": da.F, "valid_faces": int(da.n_valid.sum()), "samples_per_object": COUNT,
            "queries": 2 * K * COUNT, "cells_per_axis": [int(da.res.min()), int(da.res.max())],
            "cell_triangle_pairs": da.n_pairs, "shift": SHIFT,
            "mean_accuracy": float(metrics['accuracy'].nanmean()), "mean_chamfer_l1": float(metrics['chamfer_l1'].nanmean()),
            "build_both": timed(lambda: (md.MeshDistance(A), md.MeshDistance(B)), reps, warmup),
            "samples_both": timed(lambda: (md.sample_surface_ragged(da, COUNT, u_a), md.sample_surface_ragged(db, COUNT, u_b)),
                                  reps, warmup),
            "queries_both": timed(lambda: queries(da, db), reps, warmup),
            "sums_both": timed(sums, reps, warmup),
            "mesh_metrics": timed(lambda: md.mesh_metrics(da, db, [[k, k] for k in range(K)], COUNT, u_a=u_a, u_b=u_b),
                                  reps, warmup),
            "queries_both_cells_1": dict(timed(lambda: queries(brute_a, brute_b), brute_reps, 1), reps=brute_reps, warmup=1),
            "nearest_vertex_both": timed(vertex_search, reps, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brute_reps", type=int, default=3)
    ap.add_argument("--scenes", default="demo-sized,headline")
    args = ap.parse_args()
    need_gpu_or_exit("mesh_dist_cost")
    sizes = {"demo-sized": 13, "headline": 256}
    rows = [measure(name, sizes[name], args.reps, args.warmup, args.brute_reps) for name in args.scenes.split(",")]
    emit({"tool": "mesh_dist_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
          "rows": rows}, args.out)


if __name__ == "__main__":
    main()
