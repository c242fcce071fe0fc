"""GPU: the rasteriser (csrc/raster.hip through rfdnet_amd.render.render_scene) against the float64 / int64 restatement
tests/render_f64.py.  `ids` must be EQUAL (tests/test_render_cpu.py shows that every scene is admissible for that), depth
within one f32 unit in the last place (one rounding of an f64 quotient whose own last bit may differ), the picture within
one level per channel (f32 shading against f64)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from rfdnet_amd import io, render

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cases as cases  # noqa: E402
import render_f64  # noqa: E402
from render_cases import PALETTE, SMALL_CASES, ragged_inputs, read_png  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_scene(c):
    dev = torch.device("cuda")
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)
    scene = types.SimpleNamespace(vertices=t(c['vertices'], torch.float32), faces=t(c['faces'], torch.int32),
                                  face_obj=t(c['face_obj'], torch.int32), obj_class=t(c['obj_class'], torch.int32))
    return scene, None if c['points'] is None else t(c['points'], torch.float32)


def run(c):
    scene, pts = device_scene(c)
    return render.render_scene(scene, pts, c['camera'], palette=PALETTE, point_px=c['point_px'])


def compare(got, want):
    ids, depth, image = got.ids.cpu().numpy(), got.depth.cpu().numpy(), got.image.cpu().numpy()
    assert ids.dtype == np.int32 and depth.dtype == np.float32 and image.dtype == np.uint8
    differing = int((ids != want['ids']).sum())
    print("pixels: %d, covered: %d, ids differing: %d" % (ids.size, (want['ids'] >= 0).sum(), differing))
    assert differing == 0
    background = want['ids'] < 0
    assert np.isposinf(depth[background]).all() and (image[background] == 255).all()
    step = np.abs(depth[~background].view(np.int32).astype(np.int64) - want['depth'][~background].view(np.int32))
    level = np.abs(image.astype(np.int64) - want['image'])
    print("depth: max %d ulp; image: max %d levels" % (step.max() if step.size else 0, level.max()))
    assert (step <= 1).all() and (level <= 1).all()
    return ids


@pytest.mark.parametrize("name, make", SMALL_CASES, ids=[n for n, _ in SMALL_CASES])
def test_case_matches_the_restatement(hip, name, make):
    """1 the fill rule, 2 the depth test (with the reversed order and the coplanar duplicate), 3 the large-triangle path
    at two image sizes, 4 the rejections, 5 the points at three widths; then 1 and 2 again on the per-thread path
    (*_small), boxes on both sides of SMALL_BOX, both paths and the points mixed in three workgroups, images one pixel
    wide and the widest point square (tests/render_cases.py 7 to 9)"""
    c, want = cases.restated(name)
    assert render_f64.admissible(want)
    print("large triangles (face, workgroup, thread):", cases.large_triangles(c))
    ids = compare(run(c), want)
    if name.startswith("shared_edge_small"):
        assert (ids >= 0).sum() == cases.shared_edge_small_pixels(name.endswith("on_centres"))
    elif name.startswith("shared_edge"):
        assert (ids >= 0).sum() == cases.shared_edge_pixels(name.endswith("on_centres"))
    if name in ("mixed", "mixed_no_points"):
        assert (ids == cases.MIXED_TWIN[0]).any() and not (ids == cases.MIXED_TWIN[1]).any()
    if name.startswith("large"):
        assert (ids == 0).all()
    if name == "rejections":
        assert set(np.unique(ids)) == {-1, 0, 1, 2}                  # nothing of cases.REJECTED, the neighbours whole
        assert not set(cases.REJECTED.values()) & set(np.unique(ids))


def test_reversed_order_relabels_and_a_duplicate_loses_to_the_lower_index(hip):
    for overlap in (cases.overlap, cases.overlap_small):             # on the shared path, on the per-thread path
        plain, back, dup = (run(c) for c in (overlap(), overlap(order=(2, 1, 0)), overlap(duplicate=True)))
        ids = plain.ids.cpu().numpy()
        assert set(np.unique(ids)) == {-1, 0, 1, 2}
        np.testing.assert_array_equal(np.where(back.ids.cpu().numpy() >= 0, 2 - back.ids.cpu().numpy(), -1), ids)
        assert torch.equal(back.image, plain.image) and torch.equal(back.depth, plain.depth)
        d = dup.ids.cpu().numpy()
        assert 1 not in d
        np.testing.assert_array_equal(np.where(d > 0, d - 1, d), ids)


# ---------------------------------------------------------------------- both triangle paths and the points in one launch ----
def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def reordered(c, face_order, point_order):
    """the case with its primitives in another order: new face k is old face face_order[k], points likewise"""
    return dict(c, faces=c['faces'][face_order], face_obj=c['face_obj'][face_order], points=c['points'][point_order])


@pytest.mark.parametrize("order", ["reversed", "permuted"])
def test_mixed_does_not_depend_on_who_draws_what(hip, order):
    """another primitive order gives every triangle another thread, another workgroup and other neighbours in it, and a
    large one other company in the workgroup's list: the ids follow the order, depth and picture keep every bit"""
    c, want = cases.restated("mixed_no_twin")
    F, N = len(c['faces']), len(c['points'])
    if order == "reversed":
        face_order, point_order = np.arange(F)[::-1].copy(), np.arange(N)[::-1].copy()
    else:
        rng = np.random.default_rng(5)
        face_order, point_order = rng.permutation(F), rng.permutation(N)
    moved = reordered(c, face_order, point_order)
    print("large triangles (face, workgroup, thread):", cases.large_triangles(moved))
    assert cases.large_triangles(moved) != cases.large_triangles(c)
    plain, got = run(c), run(moved)
    ids = got.ids.cpu().numpy()
    back = np.concatenate([[-1], face_order, F + point_order])                 # new id -> old id, -1 -> -1
    np.testing.assert_array_equal(back[ids + 1], want['ids'])
    assert torch.equal(got.depth, plain.depth) and torch.equal(got.image, plain.image)


def test_mixed_twice_and_with_the_scan_read_in_place(hip):
    c, want = cases.restated("mixed")
    scene, pts = device_scene(c)
    draw = lambda p: render.render_scene(scene, p, c['camera'], palette=PALETTE, point_px=c['point_px'])
    first = draw(pts)
    compare(first, want)
    assert same_bits(first, draw(pts))
    # the scan as columns 2..5 of a wider buffer: rows 9 floats apart, the first one 8 bytes into the allocation
    buf = torch.full((pts.shape[0], 9), float('nan'), device=pts.device)
    buf[:, 2:6] = pts
    view = buf[:, 2:6]
    assert view.stride() == (9, 1) and view.data_ptr() == buf.data_ptr() + 8 and not view.is_contiguous()
    assert same_bits(first, draw(view)) and same_bits(first, draw(view.contiguous()))


def test_rasterise_on_a_reused_scratch_gives_the_restated_keys(hip):
    """watertight()'s route: render.rasterise with point_px = 1, no points and the scratch of the call before"""
    c, want = cases.restated("mixed_no_points")
    scene, _ = device_scene(c)
    cam = c['camera']
    scratch = render.rasterise(scene.vertices, scene.faces, cam.params, cam.near, cam.width, cam.height, point_px=1)
    first = scratch.keys.clone()
    again = render.rasterise(scene.vertices, scene.faces, cam.params, cam.near, cam.width, cam.height, point_px=1,
                             scratch=scratch)
    assert again.keys.data_ptr() == scratch.keys.data_ptr() and torch.equal(again.keys, first)
    keys = first.cpu().numpy()
    assert keys.dtype == np.int64 and keys.shape == want['ids'].shape and (keys > 0).all()
    np.testing.assert_array_equal(0xffffffff - (keys & 0xffffffff), want['ids'])
    step = np.abs((keys >> 32) - want['invz_bits'])
    print("1/z: max %d ulp" % step.max())
    assert (step <= 1).all()
    assert not (0xffffffff - (keys & 0xffffffff) == cases.MIXED_TWIN[1]).any()


@pytest.fixture(scope="module")
def ragged(hip):
    """three marching-cubes spheres at 8^3 (the third flattened: not finite once placed), their boxes, 500 scan points"""
    from rfdnet_amd.iscnet.mcubes import marching_cubes_batch
    from rfdnet_amd.iscnet.scene import place_objects
    dev = torch.device("cuda")
    grids = torch.from_numpy(np.stack([cases.sphere_grid(r, c) for r, c in cases.SPHERES])).to(dev)
    meshes = [(v - 1., f) for v, f in marching_cubes_batch(grids, 0.)]          # back to the unpadded grid's index space
    meshes[2] = (torch.from_numpy(cases.flattened(meshes[2][0].cpu().numpy())).to(dev), meshes[2][1])
    objs, ids, parsed, scan = ragged_inputs([(v.cpu().numpy(), f.cpu().numpy()) for v, f in meshes])
    objs = [types.SimpleNamespace(vertices=v, faces=f) for v, f in meshes]
    scene = place_objects(objs, ids, parsed)
    assert scene.vertices.is_cuda and len({m[0].shape[0] for m in meshes}) == 3
    return scene, torch.from_numpy(scan).to(dev), render.Camera.fit(scan, width=96, height=64)


def restate_scene(scene, scan, cam, point_px=3):
    return render_f64.rasterise(scene.vertices.cpu().numpy(), scene.faces.cpu().numpy(),
                                None if scan is None else scan.cpu().numpy(), cam.params, cam.near, cam.width, cam.height,
                                point_px, scene.face_obj.cpu().numpy(), scene.obj_class.cpu().numpy(),
                                render.DEFAULT_PALETTE, cam.eye)


def test_ragged_scene_through_the_public_path(ragged):
    scene, scan, cam = ragged
    want = restate_scene(scene, scan, cam)
    print("min_key_gap %s, min_snap_margin %s" % (want['min_key_gap'], want['min_snap_margin']))
    assert render_f64.admissible(want)
    first = render.render_scene(scene, scan, cam)
    ids = compare(first, want)
    F = scene.faces.shape[0]
    assert list(np.unique(scene.face_obj.cpu().numpy()[ids[(ids >= 0) & (ids < F)]])) == [0, 1]      # not the NaN object
    assert (ids >= F).any()
    again = render.render_scene(scene, scan[None], cam)                                               # (1,N,4) as the demo has it
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_ragged_scene_edges(ragged):
    scene, scan, cam = ragged
    compare(render.render_scene(scene, None, cam), restate_scene(scene, None, cam))                   # N = 0
    empty = types.SimpleNamespace(vertices=scene.vertices[:0], faces=scene.faces[:0], face_obj=scene.face_obj[:0],
                                  obj_class=scene.obj_class[:0])
    ids = compare(render.render_scene(empty, scan, cam), restate_scene(empty, scan, cam))             # F = 0
    assert ids.max() >= 0 and ids.max() < scan.shape[0]
    one = render.Camera.fit(scan, width=1, height=1)
    compare(render.render_scene(scene, scan, one), restate_scene(scene, scan, one))                   # W = H = 1
    from rfdnet_amd._lib import RfdHipError
    with pytest.raises(RfdHipError, match="8192"):
        render.render_scene(scene, scan, render.Camera.fit(scan, width=8193, height=4))
    with pytest.raises(RfdHipError, match="point_px"):
        render.render_scene(scene, scan, cam, point_px=4)
    compare(render.render_scene(scene, scan, cam), restate_scene(scene, scan, cam))                   # and it still works


def test_demo_renders_the_scene_in_a_fresh_process(hip, tmp_path):
    out = str(tmp_path / "demo")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--synthetic", "10", "--resolution_0", "16",
                           "--render", "--render_size", "160", "120", "--post_processing", "--allow-placeholder-sizes",
                           "--out", out], cwd=ROOT, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode()[-2000:]
    picture = read_png(os.path.join(out, "pred.png"))
    assert picture.shape == (120, 160, 3)
    v, f = io.read_mesh_ply(os.path.join(out, "scene_objects.ply"))
    meshes = [io.read_mesh_ply(os.path.join(out, n)) for n in sorted(os.listdir(out)) if n.startswith("proposal_")]
    assert f.shape[0] == sum(m[1].shape[0] for m in meshes) and v.shape[0] == sum(m[0].shape[0] for m in meshes)
    assert (picture != 255).any()                                    # the scan at least, and whatever was selected
    if f.shape[0]:
        assert f.min() >= 0 and f.max() < v.shape[0]
