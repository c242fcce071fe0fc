"""Cost of the occupancy-sampling path on one GPU -- a record, not a test.

    python tools/sample_cost.py [--out profiles/sample_cost.json] [--reps 20] [--warmup 3] [--points 100000]

Two meshes, both moved into the unit cube as tools/sample_mesh.py --resize does (mesh_sample.unit_cube):
tools/cost_common.py's dented marching-cubes sphere (48^3, about 18 700 faces), and watertight() of it at 256^3 (about
900 000 faces).  Per mesh, device milliseconds between HIP events (the median, minimum and maximum of `reps` calls after
`warmup`):

  build             MeshIntersector(vertices, faces, 512): the mesh check, the rescale, the cell lists (two read-backs)
  pairs             (cell, triangle) pairs in the lists
  query             100 000 points, half uniform in the cube of side 1.1 and half within 0.01 of the surface, walked in
                    the order given (`unsorted`) and in the order of their cells (`sorted`, the sort included)
  voxelize_ray      surface OR interior voxels at 16^3 and 32^3 (each builds an intersector of its own, as the reference)
  sample_surface    100 000 surface points with normals
On the smaller mesh, `torch_ops` is the same containment (rules C2 - C6 of include/rfd_sample.h over ALL triangles) written
as dense float64 torch operations in chunks of points on the same device; the tool asserts that it gives the same booleans."""
import argparse

import torch

from cost_common import emit, need_gpu_or_exit, real_mesh, timed


def torch_contains(mi, points, chunk=2048):
    """rules C2 - C6 over all triangles of the intersector `mi`, dense; torch's kernels evaluate each operation on its
    own, so the booleans are the kernel's"""
    st = torch.tensor(mi._constants, dtype=torch.float64, device=points.device)
    res = mi.resolution
    t1, t2, t3 = (mi.triangles[None, :, c] for c in range(3))
    A00, A10, A01, A11 = t1[..., 0] - t3[..., 0], t1[..., 1] - t3[..., 1], t2[..., 0] - t3[..., 0], t2[..., 1] - t3[..., 1]
    det = A00 * A11 - A01 * A10
    s, ad = torch.sign(det), det.abs()
    v1, v2 = t3 - t1, t2 - t1
    nn0 = v1[..., 1] * v2[..., 2] - v1[..., 2] * v2[..., 1]
    nn1 = v1[..., 2] * v2[..., 0] - v1[..., 0] * v2[..., 2]
    nn2 = v1[..., 0] * v2[..., 1] - v1[..., 1] * v2[..., 0]
    an, sn = nn2.abs(), torch.sign(nn2)
    out = []
    for a in range(0, points.shape[0], chunk):
        p = st[:3] * points[a:a + chunk] + st[3:]
        candidate = ((p >= 0) & (p <= res)).all(1) & (p[:, 0] < res) & (p[:, 1] < res)
        q = p[:, None, :]
        y0, y1 = q[..., 0] - t3[..., 0], q[..., 1] - t3[..., 1]
        u = (A11 * y0 - A01 * y1) * s
        v = (-A10 * y0 + A00 * y1) * s
        w = u + v
        hit = (det != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < w) & (w < ad) & (nn2 != 0)
        alpha = nn0 * (t1[..., 0] - q[..., 0]) + nn1 * (t1[..., 1] - q[..., 1])
        depth, rhs = t1[..., 2] * an + alpha * sn, q[..., 2] * an
        n0, n1 = (hit & (depth >= rhs)).sum(1), (hit & (depth < rhs)).sum(1)
        out.append(candidate & (n0 % 2 == 1) & (n1 % 2 == 1))
    return torch.cat(out)


def measure(name, v, f, args, yardstick):
    from rfdnet_amd import mesh_sample as ms
    gen = torch.Generator(device=v.device).manual_seed(7)
    n = args.points
    uniform = 1.1 * (torch.rand(n // 2, 3, dtype=torch.float64, device=v.device, generator=gen) - 0.5)
    near = ms.sample_surface(v, f, n - n // 2, generator=gen, dtype=torch.float64)[0]
    near = near + 0.01 * torch.randn(n - n // 2, 3, dtype=torch.float64, device=v.device, generator=gen)
    points = torch.cat([uniform, near])
    mi = ms.MeshIntersector(v, f, 512)
    first = mi.query(points, sort_points=False)
    assert torch.equal(first, mi.query(points, sort_points=True))
    row = {"mesh": name, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "watertight": ms.is_watertight(f),
           "points": n, "inside": int(first.sum()), "pairs": mi.n_pairs,
           "longest_cell_list": int((mi.offsets[1:] - mi.offsets[:-1]).max()),
           "build": timed(lambda: ms.MeshIntersector(v, f, 512), args.reps, args.warmup),
           "query_unsorted": timed(lambda: mi.query(points, sort_points=False), args.reps, args.warmup),
           "query_sorted": timed(lambda: mi.query(points, sort_points=True), args.reps, args.warmup),
           "cell_order_alone": timed(lambda: mi.cell_order(points), args.reps, args.warmup),
           "voxelize_surface_16": timed(lambda: ms.voxelize_surface(v, f, 16), args.reps, args.warmup),
           "voxelize_surface_32": timed(lambda: ms.voxelize_surface(v, f, 32), args.reps, args.warmup),
           "voxelize_ray_16": timed(lambda: ms.voxelize_ray(v, f, 16, generator=gen), args.reps, args.warmup),
           "voxelize_ray_32": timed(lambda: ms.voxelize_ray(v, f, 32, generator=gen), args.reps, args.warmup),
           "sample_surface": timed(lambda: ms.sample_surface(v, f, n, generator=gen, return_normals=True), args.reps,
                                   args.warmup)}
    row["query_unsorted_second_pass"] = timed(lambda: mi.query(points, sort_points=False), args.reps, 1)
    row["query_sorted_second_pass"] = timed(lambda: mi.query(points, sort_points=True), args.reps, 1)
    if yardstick:
        dense = torch_contains(mi, points)
        assert torch.equal(dense, first), "dense torch containment differs in %d points" % int((dense != first).sum())
        row["torch_ops"] = dict(timed(lambda: torch_contains(mi, points), max(args.reps // 5, 2), 1),
                                point_triangle_pairs=float(n) * int(f.shape[0]), same_booleans=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--resolution", type=int, default=256, help="of the watertight() that makes the larger mesh")
    args = ap.parse_args()
    need_gpu_or_exit("sample_cost")
    from rfdnet_amd.mesh_sample import unit_cube
    from rfdnet_amd.watertight import watertight
    unit = lambda v: unit_cube(v.double())[0].contiguous()
    v, f = real_mesh()
    rows = [measure("dented sphere 48^3", unit(v), f.to(torch.int32).contiguous(), args, True)]
    wv, wf = watertight(v, f, resolution=args.resolution)
    rows.append(measure("watertight() of it at %d^3" % args.resolution, unit(wv), wf.contiguous(), args, False))
    result = {"tool": "sample_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "hash_resolution": 512, "meshes": rows}
    emit(result, args.out)


if __name__ == "__main__":
    main()
