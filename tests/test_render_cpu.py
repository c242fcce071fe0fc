"""CPU: the scene render's host side -- place_objects against a per-object numpy loop, write_png, Camera.fit -- and the
admissibility of every scene that tests/test_gpu_render.py compares by equality (tests/render_f64.py explains the two
margins).  No GPU is touched: the rasteriser itself is checked there."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from rfdnet_amd import io, render
from rfdnet_amd.iscnet.scene import place_objects

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cases as cases  # noqa: E402
from render_cases import SMALL_CASES, ragged_inputs, read_png, restate  # noqa: E402
import render_f64  # noqa: E402
from mc_ref import index_soup, marching_cubes_soup  # noqa: E402


# ------------------------------------------------------------------------------------------------ admissibility ----
@pytest.mark.parametrize("name, make", SMALL_CASES, ids=[n for n, _ in SMALL_CASES])
def test_every_case_is_admissible(name, make):
    c, res = cases.restated(name)
    print(name, res['min_key_gap'], res['min_snap_margin'], res['candidates'])
    assert render_f64.admissible(res), (res['min_key_gap'], res['min_snap_margin'])
    assert (res['ids'] >= 0).any()
    print("large triangles (face, workgroup, thread):", cases.large_triangles(c))


def test_the_restatement_covers_a_shared_edge_once_and_breaks_ties_by_index():
    for on_centres in (False, True):
        res = restate(cases.shared_edge(on_centres))
        assert res['candidates'] == (res['ids'] >= 0).sum() == cases.shared_edge_pixels(on_centres)
        assert set(np.unique(res['ids'])) == {-1, 0, 1}
        res = restate(cases.shared_edge_small(on_centres))
        assert res['candidates'] == (res['ids'] >= 0).sum() == cases.shared_edge_small_pixels(on_centres)
        assert set(np.unique(res['ids'])) == {-1, 0, 1}
    assert restate(cases.shared_edge(True))['ids'][2, 2] >= 0 and restate(cases.shared_edge(True))['ids'][13, 13] == -1
    assert restate(cases.shared_edge_small(True))['ids'][2, 2] >= 0 and restate(cases.shared_edge_small(True))['ids'][9, 9] == -1
    for overlap in (cases.overlap, cases.overlap_small):
        dup = restate(overlap(duplicate=True))
        plain = restate(overlap())
        assert set(np.unique(plain['ids'])) == {-1, 0, 1, 2}
        assert 1 not in dup['ids']                                 # face 1 is face 0 again: the lower index wins
        np.testing.assert_array_equal(np.where(dup['ids'] > 0, dup['ids'] - 1, dup['ids']), plain['ids'])
        back = restate(overlap(order=(2, 1, 0)))
        np.testing.assert_array_equal(np.where(back['ids'] >= 0, 2 - back['ids'], -1), plain['ids'])
        np.testing.assert_array_equal(back['image'], plain['image'])
    rej = restate(cases.rejections())
    assert set(np.unique(rej['ids'])) == {-1, 0, 1, 2}


# ------------------------------------------------------------------------------- which path draws which triangle ----
def test_the_small_scenes_stay_on_the_per_thread_path_and_the_old_ones_on_the_shared_path():
    """the fill rule and the ties are tested once on each path: every box of the *_small scenes is within SMALL_BOX
    (the shared-edge halves exactly on it), every drawn box of the scenes they were shrunk from is beyond it"""
    for on_centres in (False, True):
        assert cases.box_pixels(cases.shared_edge_small(on_centres)).tolist() == [cases.SMALL_BOX] * 2
        assert (cases.box_pixels(cases.shared_edge(on_centres)) > cases.SMALL_BOX).all()
    for kwargs in ({}, {'order': (2, 1, 0)}, {'duplicate': True}):
        small, large = cases.box_pixels(cases.overlap_small(**kwargs)), cases.box_pixels(cases.overlap(**kwargs))
        assert (small > 0).all() and (small <= cases.SMALL_BOX).all() and (large > cases.SMALL_BOX).all()
    assert sorted(cases.box_pixels(cases.overlap_small()).tolist()) == [48, 49, 64]
    rej = cases.box_pixels(cases.rejections())
    assert (rej[:3] > 0).all() and not rej[3:].any()                # 0 for whatever rule 2 or 3 rejects


def test_threshold_has_the_boxes_it_is_named_for():
    c, res = cases.restated("threshold")
    boxes = cases.box_pixels(c)
    assert boxes.tolist() == cases.THRESHOLD_BOXES
    assert sorted(set(boxes.tolist())) == [63, 64, 65, 66]
    _, ix, iy, _, _ = render_f64.project(c['vertices'], c['camera'].params, c['camera'].near)
    far_out = c['faces'][16:18]                                     # the pair that the left and the upper border cut
    assert (ix[far_out].min(1) < -80 * 256).all() and (iy[far_out].min(1) < -80 * 256).all()
    assert (ix[c['faces'][18:]].max(1) > 2 * 80 * 256).all()        # the pair that the right border cuts
    # unclamped, the last pair's boxes would have 5 rows of 133 and 233 pixels: 13 x 5 is the image's width at work
    wins = np.bincount(res['ids'][res['ids'] >= 0], minlength=20)
    print("pixels won:", wins.tolist())
    assert (wins > 0).all()                                         # both of every pair show
    for a in range(0, 20, 2):                                       # and the nearer one owns all it covers
        pix, bits, prim = res['cand']
        front = a if c['vertices'][c['faces'][a, 0], 2] == 2. else a + 1
        assert (res['ids'].reshape(-1)[pix[prim == front]] == front).all()


def test_mixed_puts_both_paths_and_the_points_side_by_side():
    c, res = cases.restated("mixed")
    F, N = len(c['faces']), len(c['points'])
    assert (F, N) == (528, 100) and F % cases.RASTER_THREADS == 16          # workgroup 2: 16 triangles, then points
    boxes = cases.box_pixels(c)
    assert tuple(np.nonzero(boxes > cases.SMALL_BOX)[0]) == cases.MIXED_LARGE
    assert (boxes[boxes <= cases.SMALL_BOX] == 16).all()
    assert [(w, t) for _, w, t in cases.large_triangles(c)] == [(0, 0), (0, 255), (1, 0), (1, 1), (1, 144), (1, 255),
                                                                (2, 0), (2, 15)]
    assert boxes[400] == 96 * 64                                             # larger than the image
    first, twin = cases.MIXED_TWIN
    for name in ("mixed", "mixed_no_points"):
        ids = cases.restated(name)[1]['ids']
        assert (ids == first).sum() > 100 and (ids == twin).sum() == 0       # the twin wins nothing
    np.testing.assert_array_equal(c['vertices'][c['faces'][first]], c['vertices'][c['faces'][twin]])
    assert not set(c['faces'][first]) & set(c['faces'][twin])                # its own vertices, the same numbers
    ids = res['ids'].reshape(-1)
    kinds = [(ids < 0).sum(), (boxes[ids[(ids >= 0) & (ids < F)]] <= cases.SMALL_BOX).sum(),
             (boxes[ids[(ids >= 0) & (ids < F)]] > cases.SMALL_BOX).sum(), (ids >= F).sum()]
    print("winners: background %d, small %d, large %d, point %d" % tuple(kinds))
    assert min(kinds[1:]) > 200
    for f in cases.MIXED_LARGE:
        assert f == twin or (ids == f).sum() > 100, f                        # every other large triangle shows
    z = c['points'][:, 2]
    assert len(np.unique(z)) == N and (z < 1.).any() and ((z > 2.) & (z < 8.)).any()
    pairs = cases.winner_pairs(c, res)
    print(sorted(pairs))
    for pair in (('small', 'large'), ('large', 'small'), ('large', 'large+'), ('point', 'large'), ('large', 'point'),
                 ('small', 'point'), ('point', 'small')):
        assert pair in pairs, pair
    # without the twin the other seven keep their neighbours: one index lower from 257 on
    no_twin = cases.restated("mixed_no_twin")[0]
    assert [f for f, _, _ in cases.large_triangles(no_twin)] == [0, 255, 256, 399, 510, 511, 526]


def test_strips_and_wide_points_are_what_they_are_named_for():
    for upright in (True, False):
        c, res = cases.restated("strip_1x130" if upright else "strip_130x1")
        assert (c['camera'].width, c['camera'].height) == ((1, 130) if upright else (130, 1))
        assert cases.box_pixels(c).tolist() == [20, cases.SMALL_BOX, 130]
        ids = np.unique(res['ids'])
        assert {0, 1, 2} <= set(ids) and (ids >= 3).sum() >= 3 and ids.min() >= 0
        wide = cases.restated("strip_1x130_px63" if upright else "strip_130x1_px63")[1]
        assert (wide['ids'] >= 3).sum() > (res['ids'] >= 3).sum()
    c, res = cases.restated("points_63")
    F, (H, W) = 1, res['ids'].shape
    centre, corner, other_corner, from_outside, from_below, far, behind, back = (F + n for n in range(8))
    pix, _, prim = res['cand']
    assert (prim == centre).sum() == H * W                                   # cut by all four borders at once
    for n, rows, cols in ((corner, 34, 34), (other_corner, 33, 33), (from_outside, 36, 11), (from_below, 7, 40)):
        assert (prim == n).sum() == rows * cols, n                           # ... by two, by three of them
    assert not np.isin(prim, (far, behind)).any()
    assert {0, corner, other_corner, from_outside, from_below} <= set(np.unique(res['ids']))


def sphere_meshes():
    out = []
    for k, (radius, centre) in enumerate(cases.SPHERES):
        v, f = index_soup(marching_cubes_soup(cases.sphere_grid(radius, centre), 0.))
        out.append((cases.flattened(v) if k == 2 else v, f))
    return out


def test_the_ragged_scene_is_admissible():
    objs, ids, parsed, scan = ragged_inputs(sphere_meshes())
    scene = place_objects(objs, ids, parsed)
    assert not np.isfinite(scene.vertices[scene.obj_off[2]:].numpy()).any()       # the flattened mesh
    assert np.isfinite(scene.vertices[:scene.obj_off[2]].numpy()).all()
    cam = render.Camera.fit(scan, width=96, height=64)
    res = render_f64.rasterise(scene.vertices.numpy(), scene.faces.numpy(), scan, cam.params, cam.near, 96, 64, 3,
                               scene.face_obj.numpy(), scene.obj_class.numpy(), render.DEFAULT_PALETTE, cam.eye)
    print(res['min_key_gap'], res['min_snap_margin'], res['candidates'])
    assert render_f64.admissible(res), (res['min_key_gap'], res['min_snap_margin'])
    F = scene.faces.shape[0]
    shown = np.unique(scene.face_obj.numpy()[res['ids'][(res['ids'] >= 0) & (res['ids'] < F)]])
    assert list(shown) == [0, 1] and (res['ids'] >= F).any()


# ---------------------------------------------------------------------------------------------------- placement ----
def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("theta", [0., 2.5, -np.pi])
def test_place_objects_matches_the_per_object_loop(theta):
    rng = np.random.default_rng(3)
    n_v = [37, 0, 10000, 5]
    verts = [rng.uniform(-0.5, 0.5, (n, 3)) * (0.9, 0.6, 0.8) for n in n_v]
    faces = [rng.integers(0, max(n, 1), (2 * n, 3)) for n in n_v]
    normals = [rng.normal(size=(n, 3)) for n in n_v]
    normals[3][2] = np.nan
    boxes = np.stack([cases.get_3d_box_cam((0.5 + 0.3 * k, 1.2 - 0.2 * k, 0.7), theta + 0.3 * k, (k - 1.5, 0.5 * k, 0.4))
                      for k in range(4)])
    corners = np.zeros((1, 9, 8, 3))
    ids = np.array([7, 2, 5, 0])
    corners[0, ids] = boxes
    sem = np.arange(9)[None] + 3
    objs = [types.SimpleNamespace(vertices=torch.from_numpy(v), faces=torch.from_numpy(f), vertex_normals=torch.from_numpy(n))
            for v, f, n in zip(verts, faces, normals)]
    parsed = {'pred_corners_3d_upright_camera': torch.from_numpy(corners), 'pred_sem_cls': torch.from_numpy(sem)}
    got = place_objects(objs, torch.from_numpy(ids).view(1, 4, 1), parsed, with_normals=True)
    want = render_f64.place_loop(verts, faces, boxes, normals)
    for name in ('faces', 'face_obj', 'obj_off', 'face_off'):
        assert getattr(got, name).dtype == torch.int32
        np.testing.assert_array_equal(getattr(got, name).numpy(), want[name], err_msg=name)
    np.testing.assert_array_equal(got.obj_class.numpy(), sem[0, ids])
    assert got.vertices.dtype == torch.float32 and got.vertices.shape == (sum(n_v), 3)
    err = np.abs(got.vertices.numpy().astype(np.float64) - want['vertices'])
    assert (err <= ulp32(want['vertices'])).all(), (err / ulp32(want['vertices'])).max()
    gn, wn = got.normals.numpy().astype(np.float64), want['normals']
    nan_row = n_v[0] + n_v[2] + 2
    assert np.isnan(gn[nan_row]).all() and np.isnan(wn[nan_row]).all()
    keep = np.arange(len(gn)) != nan_row
    assert (np.abs(gn - wn)[keep] <= ulp32(wn[keep])).all()
    np.testing.assert_allclose(np.linalg.norm(gn[keep], axis=1), 1., atol=1e-6)
    # the placed mesh fills its box: the extent along the box's own axes is its sizes
    k, (lo, hi) = 2, (n_v[0], n_v[0] + n_v[2])
    centre, sizes, heading = render_f64.box_from_corners(boxes[k])
    local = (want['vertices'][lo:hi] - centre) @ np.array([[np.cos(heading), -np.sin(heading), 0.],
                                                           [np.sin(heading), np.cos(heading), 0.], [0., 0., 1.]])
    np.testing.assert_allclose(local.max(0) - local.min(0), sizes, rtol=1e-12)


def test_place_objects_without_meshes_and_with_a_flat_mesh():
    parsed = {'pred_corners_3d_upright_camera': torch.zeros(1, 4, 8, 3, dtype=torch.float64)}
    empty = place_objects([], torch.zeros(1, 0, 1, dtype=torch.int64), parsed, with_normals=True)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.normals.shape == (0, 3)
    assert empty.obj_off.tolist() == [0] and empty.face_off.tolist() == [0]
    flat = np.random.default_rng(0).uniform(-1, 1, (6, 3))
    flat[:, 0] = 0.25
    boxes = cases.ragged_boxes()[:1]
    got = place_objects([types.SimpleNamespace(vertices=torch.from_numpy(flat), faces=torch.tensor([[0, 1, 2]]))],
                        torch.zeros(1, 1, 1, dtype=torch.int64), {'pred_corners_3d_upright_camera': torch.from_numpy(boxes[None])})
    want = render_f64.place_loop([flat], [np.array([[0, 1, 2]])], boxes)
    assert not np.isfinite(want['vertices']).any()                                 # numpy's dot spreads the NaN axis
    np.testing.assert_array_equal(np.isnan(got.vertices.numpy()), np.isnan(want['vertices']))
    assert got.obj_class.tolist() == [0]


def test_render_scene_refuses_cpu_tensors():
    objs, ids, parsed, scan = ragged_inputs([(np.eye(3), np.array([[0, 1, 2]]))] * 3)
    scene = place_objects(objs, ids, parsed)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        render.render_scene(scene, torch.from_numpy(scan), render.Camera.fit(scan, 32, 24))


# ----------------------------------------------------------------------------------------------------------- png ----
@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (640, 480)])
def test_write_png_round_trip(tmp_path, w, h):
    img = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    io.write_png(path, img)
    np.testing.assert_array_equal(read_png(path), img)
    with pytest.raises(ValueError):
        io.write_png(path, img.astype(np.float32))


def test_save_scene_writes_the_two_files(tmp_path):
    objs, ids, parsed, scan = ragged_inputs([(np.eye(3) + k, np.array([[0, 1, 2]])) for k in range(3)])
    scene = place_objects(objs, ids, parsed)
    io.save_scene(str(tmp_path / "a"), scene)
    assert os.listdir(tmp_path / "a") == ['scene_objects.ply']
    picture = types.SimpleNamespace(image=torch.full((4, 6, 3), 9, dtype=torch.uint8))
    io.save_scene(str(tmp_path / "b"), scene, picture)
    assert sorted(os.listdir(tmp_path / "b")) == ['pred.png', 'scene_objects.ply']
    v, f = io.read_mesh_ply(str(tmp_path / "b" / "scene_objects.ply"))
    np.testing.assert_array_equal(v, scene.vertices.numpy())
    np.testing.assert_array_equal(f, scene.faces.numpy())
    assert read_png(str(tmp_path / "b" / "pred.png")).shape == (4, 6, 3)


# -------------------------------------------------------------------------------------------------------- camera ----
@pytest.mark.parametrize("w, h", [(1024, 768), (96, 64), (120, 400)])
def test_camera_fit_keeps_the_scans_box_in_the_image(w, h):
    scan = cases.ragged_scan() * np.float32([1., 2.5, 0.7, 1.])
    cam = render.Camera.fit(scan, width=w, height=h)
    lo, hi = scan[:, :3].min(0), scan[:, :3].max(0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    xy, z = cam.project(corners)
    assert (z >= cam.near).all()
    assert (xy >= 0).all() and (xy[:, 0] <= w).all() and (xy[:, 1] <= h).all()
    centre_xy, _ = cam.project(((lo + hi) / 2.)[None])
    np.testing.assert_allclose(centre_xy[0], [w / 2., h / 2.], atol=1e-9)
    direction = (cam.eye - (lo + hi) / 2.) / np.linalg.norm(cam.eye - (lo + hi) / 2.)
    np.testing.assert_allclose(direction, np.array([0., -1., 1.]) / np.sqrt(2.), atol=1e-12)
    top, _ = cam.project(((lo + hi) / 2. + [0., 0., 0.1])[None])
    assert top[0, 1] < h / 2.                                                      # +z of the scan is up in the picture
    same = render.Camera.fit(torch.from_numpy(scan)[None], width=w, height=h)
    np.testing.assert_array_equal(same.params, cam.params)


def test_camera_params_is_the_array_the_rasteriser_takes():
    from rfdnet_amd.watertight import views_on_sphere
    cam = render.Camera.fit(cases.ragged_scan(), width=96, height=64)
    got = render.camera_params(cam.world_to_view, cam.fx, cam.fy, cam.cx, cam.cy)
    assert got.dtype == np.float64 and got.shape == (16,) and got.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(got, cam.params)
    # render_depthmaps' convention: [R | (0,0,1)], fx = fy = focal, the principal point at S / 2 + 0.5
    R = views_on_sphere(3)[1]
    want = np.array([R[0, 0], R[0, 1], R[0, 2], 0., R[1, 0], R[1, 1], R[1, 2], 0., R[2, 0], R[2, 1], R[2, 2], 1.,
                     48., 48., 24.5, 24.5])
    got = render.camera_params(np.concatenate([R, [[0.], [0.], [1.]]], 1), 48, 48, 48 / 2. + 0.5, 48 / 2. + 0.5)
    assert got.dtype == np.float64 and got.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(got, want)
