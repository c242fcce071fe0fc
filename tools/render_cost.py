"""Cost of the scene render on one GPU -- a record, not a test.

    python tools/render_cost.py [--out profiles/render_cost.json] [--reps 20] [--warmup 3]

Two scenes at 1024x768 with 80 000 scan points (rfdnet_amd.synthetic, seed 100): the demo-sized one with 13 objects and
the headline one with 256.  The objects are marching-cubes meshes of dented spheres at 48^3 (about 18 600 faces each,
the order of the generator's meshes), in the synthetic scene's boxes (used again with other centres and headings as often
as needed).  Per scene: device milliseconds of render_scene (HIP events around the call, the median, minimum and maximum of
`reps` calls after `warmup`), of place_objects the same way, the primitive counts, the covered pixels, and beside them
the scene's own reconstruction time from the benchmark records profiles/r06_bench_demo.json / r06_bench_headline.json."""
import argparse
import json
import os
import torch

from cost_common import ROOT, emit, need_gpu_or_exit, scene_inputs, timed


def measure(label, n_obj, record, reps, warmup):
    from rfdnet_amd import render
    from rfdnet_amd.iscnet.scene import place_objects
    meshes, ids, parsed, scan = scene_inputs(n_obj)
    camera = render.Camera.fit(scan, width=1024, height=768)
    scene = place_objects(meshes, ids, parsed)
    out = render.render_scene(scene, scan, camera)
    F = int(scene.faces.shape[0])
    row = {"scene": label, "objects": n_obj, "vertices": int(scene.vertices.shape[0]), "faces": F,
           "scan_points": int(scan.shape[1]), "image": [1024, 768], "point_px": 3, "launches": 3, "clears": 1,
           "pixels_on_faces": int(((out.ids >= 0) & (out.ids < F)).sum()), "pixels_on_points": int((out.ids >= F).sum()),
           "render_scene": timed(lambda: render.render_scene(scene, scan, camera), reps, warmup),
           "place_objects": timed(lambda: place_objects(meshes, ids, parsed), reps, warmup)}
    with open(os.path.join(ROOT, "profiles", record)) as f:
        bench = json.load(f)
    row["reconstruction"] = {"record": "profiles/" + record, "ms_per_step": bench["ms_per_step"], "metric": bench["metric"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    need_gpu_or_exit("render_cost")
    rows = [measure("demo-sized", 13, "r06_bench_demo.json", args.reps, args.warmup),
            measure("headline", 256, "r06_bench_headline.json", args.reps, args.warmup)]
    result = {"tool": "render_cost", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "rows": rows}
    emit(result, args.out)


if __name__ == "__main__":
    main()
