"""The scenes of the rasteriser's tests and the helpers its two tiers share (no test in here): tests/test_render_cpu.py shows on the CPU that each of them is
admissible for a comparison by equality (tests/render_f64.py), tests/test_gpu_render.py renders them on the device.

The small cases use a camera at the origin that looks along +z with y down and a focal length that is a power of two,
so a vertex meant for screen position (sx, sy) at depth Z is ((sx - cx) Z / f, (sy - cy) Z / f, Z), and with sx, sy on
multiples of 1/4 pixel and Z a power of two the projection is exact: pixel centres lie exactly ON the edges where a case
wants them to, and every snapped coordinate is half a step away from its rounding boundary."""
import struct
import types
import zlib

import numpy as np
import torch

import render_f64

NEAR = 0.25
# The two constants of rfdnet_amd/csrc/raster.hip (raster_triangles_kernel) that the cases from 7 on are aimed at:
# primitive p is thread p % RASTER_THREADS of workgroup p // RASTER_THREADS, and a triangle whose clamped pixel box has
# more than SMALL_BOX pixels is not walked by its own thread but by all the threads of its workgroup together.
SMALL_BOX = 64
RASTER_THREADS = 256


def camera(width, height, focal=None):
    """the 16 doubles, the eye and the size, with the attributes rfdnet_amd.render.render_scene reads"""
    f = float(focal or width)
    params = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, f, f, width / 2., height / 2.], np.float64)
    return types.SimpleNamespace(params=params, eye=np.zeros(3), width=width, height=height, near=NEAR)


def at(cam, sx, sy, z):
    f, cx, cy = cam.params[12], cam.params[14], cam.params[15]
    return [(sx - cx) * z / f, (sy - cy) * z / f, z]


def case(cam, vertices, faces, points=None, point_px=3, obj_class=(3,), face_obj=None):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return dict(camera=cam, vertices=np.asarray(vertices, np.float32).reshape(-1, 3), faces=faces,
                points=None if points is None else np.asarray(points, np.float32), point_px=point_px,
                obj_class=np.asarray(obj_class, np.int32),
                face_obj=np.zeros(len(faces), np.int32) if face_obj is None else np.asarray(face_obj, np.int32))


# 1 ------------------------------------------------------------------------------------------------ the fill rule ----
def shared_edge(on_centres):
    """a square cut along its diagonal, which runs through pixel centres.  on_centres: the square's own edges run through
    pixel centres too (2.5 .. 13.5: rows and columns 2..12 are covered, 13 is not); else between them (2 .. 14)."""
    cam = camera(16, 16)
    lo, hi = (2.5, 13.5) if on_centres else (2., 14.)
    v = [at(cam, lo, lo, 2.), at(cam, hi, lo, 2.), at(cam, hi, hi, 2.), at(cam, lo, hi, 2.)]
    return case(cam, v, [[0, 1, 2], [0, 2, 3]])


def shared_edge_pixels(on_centres):
    return 11 * 11 if on_centres else 12 * 12


def shared_edge_small(on_centres):
    """shared_edge() shrunk until each half is walked by its own thread: 2.5 .. 9.5 (rows and columns 2..8 are covered,
    9 is not) or 2 .. 10; either way both triangles have a box of exactly 8 x 8 = SMALL_BOX pixels"""
    cam = camera(16, 16)
    lo, hi = (2.5, 9.5) if on_centres else (2., 10.)
    v = [at(cam, lo, lo, 2.), at(cam, hi, lo, 2.), at(cam, hi, hi, 2.), at(cam, lo, hi, 2.)]
    return case(cam, v, [[0, 1, 2], [0, 2, 3]])


def shared_edge_small_pixels(on_centres):
    return 7 * 7 if on_centres else 8 * 8


# 2 --------------------------------------------------------------------------------------------------- the depth test ----
def overlap(order=(0, 1, 2), duplicate=False):
    """two tilted triangles that cross over each other's depth range and a third behind both; `order`: the primitive
    order; duplicate: the first triangle twice (coplanar, bit-equal 1/z: the lower index must win everywhere)"""
    cam = camera(32, 32)
    v = [at(cam, 3.25, 4.25, 1.), at(cam, 28.25, 6.25, 2.), at(cam, 9.25, 27.25, 1.5),
         at(cam, 27.25, 3.25, 1.25), at(cam, 29.25, 25.25, 1.75), at(cam, 2.25, 16.25, 2.25),
         at(cam, 1.25, 1.25, 4.), at(cam, 30.25, 2.25, 4.), at(cam, 15.25, 30.25, 3.)]
    order = list(order[:1]) + list(order) if duplicate else list(order)
    return case(cam, v, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])[order], obj_class=(1, 5, 9), face_obj=order)


def overlap_small(order=(0, 1, 2), duplicate=False):
    """overlap() with every clamped box within SMALL_BOX pixels (7 x 7, 8 x 6, 8 x 8): the same crossing, the same
    reversed order and the same coplanar duplicate, each triangle walked by its own thread"""
    cam = camera(16, 16)
    v = [at(cam, 1.25, 1.25, 1.), at(cam, 8.25, 2.25, 2.), at(cam, 3.25, 8.25, 1.5),
         at(cam, 8.25, 1.25, 1.25), at(cam, 8.75, 7.25, 1.75), at(cam, 1.25, 5.25, 2.25),
         at(cam, 0.75, 0.75, 4.), at(cam, 8.75, 1.25, 4.), at(cam, 4.25, 8.75, 3.)]
    order = list(order[:1]) + list(order) if duplicate else list(order)
    return case(cam, v, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])[order], obj_class=(1, 5, 9), face_obj=order)


# 3 ------------------------------------------------------------------------------------------- the large-triangle path ----
def larger_than_image(width, height):
    cam = camera(width, height, focal=1024.)
    v = [at(cam, -1.75 * width, -1.25 * height, 2.), at(cam, 3.25 * width, -0.75 * height, 4.),
         at(cam, -0.25 * width, 4.25 * height, 1.)]
    return case(cam, v, [[0, 1, 2]])


# 4 ------------------------------------------------------------------------------------------------------ rejections ----
REJECTED = {'behind_near': 3, 'nan': 4, 'inf': 5, 'beyond_2^20': 6, 'zero_area': 7, 'repeated_vertex': 8}


def rejections():
    """three good triangles (faces 0..2) and six that must leave no trace (REJECTED), each overlapping a good one"""
    cam = camera(32, 32)
    v = [at(cam, 2.25, 2.25, 2.), at(cam, 14.25, 3.25, 2.), at(cam, 5.25, 13.25, 2.),            # 0..2
         at(cam, 17.25, 2.25, 3.), at(cam, 30.25, 4.25, 3.), at(cam, 20.25, 14.25, 3.),           # 3..5
         at(cam, 4.25, 17.25, 1.5), at(cam, 28.25, 18.25, 1.5), at(cam, 15.25, 30.25, 1.5),       # 6..8
         [0., 0., 0.125],                                                                          # 9: nearer than `near`
         [np.nan, 0., 1.], [0., np.inf, 1.], [1e6, 0., 1.],                                        # 10..12
         at(cam, 10.25, 10.25, 1.), at(cam, 20.25, 20.25, 1.)]                                     # 13, 14
    v.append(at(cam, 15.25, 15.25, 1.))                                                            # 15: midpoint of 13, 14
    faces = [[0, 1, 2], [3, 4, 5], [6, 7, 8],
             [0, 1, 9], [3, 10, 5], [6, 11, 8], [0, 12, 2], [13, 15, 14], [7, 7, 8]]
    return case(cam, v, faces)


# 5 ---------------------------------------------------------------------------------------------------------- points ----
def points(point_px):
    """a tilted triangle; points (x y z height) in front of it, behind it, on the image's border and corner, just outside
    the image (its square reaches in when it is wide enough), outside by far, and behind the camera"""
    cam = camera(24, 16)
    v = [at(cam, 3.25, 2.25, 2.), at(cam, 21.25, 3.25, 4.), at(cam, 8.25, 14.25, 2.)]
    pts = [at(cam, 8.3, 6.3, 1.), at(cam, 12.3, 7.3, 8.), at(cam, 0.3, 5.3, 1.5), at(cam, 23.6, 15.6, 1.5),
           at(cam, -1.7, 11.3, 1.5), at(cam, 100.3, 7.3, 1.5), [0., 0., -1.], at(cam, 9.3, 6.7, 1.25)]
    return case(cam, v, [[0, 1, 2]], points=np.concatenate([np.asarray(pts), np.ones((len(pts), 1))], 1),
                point_px=point_px)


# 6 ---------------------------------------------------------------------------------------------- the ragged scene ----
SPHERE_N = 8
SPHERES = ((2.9, (3.5, 3.5, 3.5)), (2.2, (3.2, 3.9, 3.4)), (3.3, (3.6, 3.4, 3.7)))      # radius, centre, in grid steps


def sphere_grid(radius, centre):
    """(8,8,8) f32: radius - distance to `centre`: positive inside; marching cubes at 0 gives the sphere"""
    g = np.stack(np.meshgrid(*[np.arange(SPHERE_N, dtype=np.float64)] * 3, indexing='ij'), -1)
    return (radius - np.linalg.norm(g - np.asarray(centre), axis=-1)).astype(np.float32)


def get_3d_box_cam(size, heading, centre_depth):
    """(8,3) upright-camera corners of the box with depth-frame centre, sizes (l,w,h) and heading angle (the layout of
    parsed_predictions['pred_corners_3d_upright_camera']; net_utils/box_util.py:183-198 with heading -> -heading)"""
    l, w, h = size
    c, s = np.cos(-heading), np.sin(-heading)
    x = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * l / 2.
    y = np.array([1, 1, 1, 1, -1, -1, -1, -1]) * h / 2.
    z = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * w / 2.
    centre_cam = np.array([centre_depth[0], -centre_depth[2], centre_depth[1]])
    return np.stack([c * x + s * z, y, -s * x + c * z], 1) + centre_cam


def flattened(vertices):
    """the mesh with no extent along its second axis: placing it divides 0 by 0, its vertices are not finite"""
    v = np.array(vertices, copy=True)
    v[:, 1] = 3.5
    return v


def ragged_boxes():
    """(3,8,3): different headings and sizes"""
    return np.stack([get_3d_box_cam((1.1, 0.7, 0.9), 0.4, (-0.8, 0.3, 0.5)),
                     get_3d_box_cam((0.6, 1.3, 0.5), -2.1, (0.9, -0.4, 0.3)),
                     get_3d_box_cam((0.8, 0.9, 0.7), 1.0, (0.1, 0.9, 0.4))])


def ragged_scan(n=500, seed=0):
    """(n,4) f32: a floor and two walls around the boxes, with the height column of the demo's input.  The seed is one of
    those at which the scene seen from Camera.fit is admissible (about one in three is: a few thousand coordinates, each
    within 1e-6 pixel of a rounding boundary with probability 5e-4); test_render_cpu.py holds it to that."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-2., 2., (n, 3))
    p[: n // 2, 2] = 0.
    p[n // 2: 3 * n // 4, 1] = 2.
    p[3 * n // 4:, 0] = -2.
    p[n // 2:, 2] = np.abs(p[n // 2:, 2])
    return np.concatenate([p, p[:, 2:3]], 1).astype(np.float32)


# 7 ------------------------------------------------------------------------------- both sides of the SMALL_BOX threshold ----
def box_pixels(c):
    """(F,) int: the pixels of every face's clamped box as include/rfd_render.h rule 3 defines it -- the pixels whose
    centre 256 i + 128 lies within the snapped corners' extent, cut to the image -- from render_f64.project's snapped
    coordinates; 0 for a face that is rejected (an invalid or missing corner, no area, an empty box)"""
    cam, V = c['camera'], len(c['vertices'])
    _, ix, iy, valid, _ = render_f64.project(c['vertices'], cam.params, cam.near)
    out = np.zeros(len(c['faces']), np.int64)
    for f, tri in enumerate(c['faces']):
        if (tri < 0).any() or (tri >= V).any() or not valid[tri].all():
            continue
        x, y = [int(v) for v in ix[tri]], [int(v) for v in iy[tri]]
        if (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) == 0:
            continue
        i0, i1 = max(-((128 - min(x)) // 256), 0), min((max(x) - 128) // 256, cam.width - 1)
        j0, j1 = max(-((128 - min(y)) // 256), 0), min((max(y) - 128) // 256, cam.height - 1)
        out[f] = max(i1 - i0 + 1, 0) * max(j1 - j0 + 1, 0)
    return out


def large_triangles(c):
    """[(face, workgroup, thread)] of the faces that raster_triangles_kernel leaves to the whole workgroup"""
    return [(int(f), int(f) // RASTER_THREADS, int(f) % RASTER_THREADS) for f in np.nonzero(box_pixels(c) > SMALL_BOX)[0]]


# the clamped boxes of threshold()'s faces, pair by pair (the CPU tier holds the geometry to them)
THRESHOLD_BOXES = [7 * 9, 7 * 9, 8 * 8, 8 * 8, 5 * 13, 5 * 13, 6 * 11, 6 * 11, 1 * 64, 1 * 64, 64 * 1, 64 * 1,
                   1 * 65, 1 * 65, 65 * 1, 65 * 1, 8 * 8, 8 * 8, 13 * 5, 13 * 5]


def threshold():
    """pairs of triangles with the same clamped box at separate places of one 80 x 80 image, the boxes on both sides of
    SMALL_BOX (THRESHOLD_BOXES).  The two of a pair overlap, one at depth 2 and one at depth 4 (which of them has the
    lower index alternates), so every pixel has a definite winner.  The last two pairs are clamped by the image: one
    reaches far out over the left and the upper border (negative snapped coordinates) and keeps 8 x 8 pixels, one reaches
    far out over the right border and keeps 13 x 5 = 65 only because the image is 80 wide."""
    cam = camera(80, 80, focal=64.)
    v, faces = [], []

    def pair(a, b, front_first):
        for tri, z in ((a, 2. if front_first else 4.), (b, 4. if front_first else 2.)):
            faces.append([len(v), len(v) + 1, len(v) + 2])
            v.extend(at(cam, sx, sy, z) for sx, sy in tri)

    def halves(x0, y0, x1, y1, front_first):
        """the upper-left and the upper-right half of a rectangle: they share its upper quarter"""
        pair([(x0, y0), (x1, y0), (x0, y1)], [(x0, y0), (x1, y0), (x1, y1)], front_first)

    halves(16.25, 2.25, 23.25, 11.25, True)                                   # columns 16..22, rows 2..10: 7 x 9
    halves(28.25, 2.25, 36.25, 10.25, False)                                  # 8 x 8
    halves(40.25, 2.25, 45.25, 15.25, True)                                   # 5 x 13
    halves(50.25, 2.25, 56.25, 13.25, False)                                  # 6 x 11
    pair([(10.25, 10.25), (11.25, 10.25), (10.75, 74.25)], [(10.25, 74.25), (11.25, 74.25), (10.75, 10.25)], True)   # column 10, rows 10..73
    pair([(8.25, 77.25), (8.25, 78.25), (72.25, 77.75)], [(72.25, 77.25), (72.25, 78.25), (8.25, 77.75)], False)     # row 77, columns 8..71
    pair([(12.25, 9.25), (13.25, 9.25), (12.75, 74.25)], [(12.25, 74.25), (13.25, 74.25), (12.75, 9.25)], False)     # column 12, rows 9..73
    pair([(8.25, 75.25), (8.25, 76.25), (73.25, 75.75)], [(73.25, 75.25), (73.25, 76.25), (8.25, 75.75)], True)      # row 75, columns 8..72
    pair([(-120.25, -90.25), (7.75, 2.25), (2.25, 7.75)], [(-90.25, -120.25), (7.75, 3.25), (3.25, 7.75)], True)     # columns, rows 0..7
    pair([(67.25, 30.25), (200.25, 30.25), (73.25, 35.25)], [(67.25, 30.25), (300.25, 35.25), (67.25, 35.25)], True)   # columns 67..79, rows 30..34
    return case(cam, v, faces)


# 8 --------------------------------------------------------------------------------------------- mixed workgroups ----
MIXED_LARGE = (0, 255, 256, 257, 400, 511, 512, 527)         # where mixed() has its large triangles
MIXED_TWIN = (255, 257)                                       # 257 is 255 again


def mixed(twin=True, points=True):
    """96 x 64.  Small: a 20 x 13 grid of quads of 4 x 4 pixels, each cut in two, at depth 2 (520 triangles with a box of
    16 pixels).  Large: eight triangles spliced in at MIXED_LARGE -- the first and the last thread of workgroups 0 and 1,
    two more inside workgroup 1, the first thread of workgroup 2 and, as the last face (F = 528), the thread next to the
    first scan point's -- six of them tilted through the grid's depth, 400 larger than the image at depth 8 behind
    everything, 257 a bit-equal twin of 255 (its own three vertices, the same numbers) in another workgroup, which must
    win no pixel.  Points: 100 squares of 3 x 3 on a lattice, each at a depth of its own between 0.78 and 6.97: in front of
    everything, between the layers, behind the grid.  They share workgroup 2 with the last 16 triangles.
    twin=False leaves face 257 out (F = 527), points=False the scan."""
    cam = camera(96, 64, focal=128.)
    v = [at(cam, 8.25 + 4 * a, 6.25 + 4 * b, 2.) for b in range(14) for a in range(21)]
    small = []
    for b in range(13):
        for a in range(20):
            k = 21 * b + a
            small += [[k, k + 1, k + 22], [k, k + 22, k + 21]]
    large = {0: [(4.25, 3.25, 1.), (90.25, 10.25, 4.), (20.25, 60.25, 2.)],
             255: [(92.25, 5.25, 1.), (10.25, 30.25, 4.), (80.25, 61.25, 4.)],
             256: [(50.25, 2.25, 4.), (93.25, 50.25, 1.), (30.25, 62.25, 2.)],
             400: [(-168.25, -80.25, 8.), (312.25, -48.25, 8.), (-24.25, 272.25, 8.)],
             511: [(2.25, 40.25, 1.), (60.25, 20.25, 4.), (70.25, 63.25, 1.)],
             512: [(30.25, 8.25, 1.), (85.25, 30.25, 2.), (40.25, 55.25, 4.)],
             527: [(60.25, 4.25, 4.), (94.25, 40.25, 1.), (55.25, 50.25, 1.)]}
    large[MIXED_TWIN[1]] = large[MIXED_TWIN[0]]
    faces, small = [], iter(small)
    for f in range(len(MIXED_LARGE) + 520):
        if f in large:
            faces.append([len(v), len(v) + 1, len(v) + 2])
            v.extend(at(cam, *corner) for corner in large[f])
        else:
            faces.append(next(small))
    if not twin:
        del faces[MIXED_TWIN[1]]
    pts = None
    if points:
        pts = [at(cam, 6.5 + 9 * (n % 10), 4.5 + 6 * (n // 10), 0.78125 + (37 * n % 100) / 16.) + [1.] for n in range(100)]
    return case(cam, v, faces, points=pts, point_px=3, obj_class=(2, 6), face_obj=np.arange(len(faces)) % 2)


# 9 ----------------------------------------------------------------------------------------- strips and point edges ----
def strip(upright, point_px=3):
    """an image one pixel wide, 1 x 130 (upright) or 130 x 1: a tilted triangle whose clamped box is the whole line of 130
    pixels, two small ones in front of it (20 pixels, and exactly SMALL_BOX: it is three pixels wide before the image cuts
    it) and points in front, in between, on both ends, just outside, outside by far and behind the camera"""
    cam = camera(1, 130, focal=64.) if upright else camera(130, 1, focal=64.)
    put = (lambda x, y, z: at(cam, x, y, z)) if upright else (lambda x, y, z: at(cam, y, x, z))
    v = [put(-1.25, -3.25, 4.), put(3.25, -3.25, 4.), put(-1.25, 400.25, 2.),
         put(-0.75, 10.25, 2.), put(1.75, 10.25, 2.), put(0.25, 30.25, 2.),
         put(-0.75, 40.25, 2.), put(1.75, 40.25, 2.), put(0.25, 104.25, 1.)]
    pts = [put(0.3, 5.3, 1.5), put(0.6, 129.6, 1.25), put(0.4, 64.4, 3.5), put(0.3, 20.3, 2.5), put(-1.7, 80.3, 1.75),
           put(0.3, -1.7, 1.125), put(100.3, 7.3, 1.5), put(0.3, 300.3, 1.5), [0., 0., -1.], put(0.7, 110.3, 0.75)]
    return case(cam, v, [[3, 4, 5], [6, 7, 8], [0, 1, 2]], points=np.concatenate([np.asarray(pts), np.ones((len(pts), 1))], 1),
                point_px=point_px)                                             # the large one last: thread 2


def points_63():
    """the widest square, 63 x 63, on a 40 x 36 image: cut by all four borders at once (the point in the middle covers
    the whole image), by two of them in the corners, reaching in from outside, outside by far, behind the camera; a
    tilted triangle between the points' depths"""
    cam = camera(40, 36, focal=32.)
    v = [at(cam, 3.25, 2.25, 2.), at(cam, 37.25, 3.25, 4.), at(cam, 8.25, 33.25, 2.)]
    pts = [at(cam, 20.3, 18.3, 6.), at(cam, 2.3, 2.3, 1.25), at(cam, 38.6, 34.6, 5.), at(cam, -20.7, 10.3, 1.125),
           at(cam, 30.3, 60.7, 3.), at(cam, 80.3, 7.3, 1.5), [0., 0., -1.], at(cam, 25.3, 5.7, 8.)]
    return case(cam, v, [[0, 1, 2]], points=np.concatenate([np.asarray(pts), np.ones((len(pts), 1))], 1), point_px=63)


# ------------------------------------------------------------------------------------------- what both tiers share ----
PALETTE = ((0.9, 0.1, 0.1), (0.1, 0.8, 0.2), (0.2, 0.3, 0.9), (0.8, 0.8, 0.1), (0.1, 0.7, 0.7), (0.7, 0.2, 0.8),
           (0.5, 0.5, 0.5), (0.9, 0.5, 0.1), (0.3, 0.6, 0.3), (0.6, 0.3, 0.3), (0.2, 0.2, 0.5), (0.4, 0.9, 0.6))


def restate(c, **over):
    c = dict(c, **over)
    cam = c['camera']
    return render_f64.rasterise(c['vertices'], c['faces'], c['points'], cam.params, cam.near, cam.width, cam.height,
                                c['point_px'], c['face_obj'], c['obj_class'], PALETTE, cam.eye)


SMALL_CASES = [("shared_edge", lambda: shared_edge(False)), ("shared_edge_on_centres", lambda: shared_edge(True)),
               ("overlap", overlap), ("overlap_reversed", lambda: overlap(order=(2, 1, 0))),
               ("overlap_duplicate", lambda: overlap(duplicate=True)),
               ("large_64x48", lambda: larger_than_image(64, 48)),
               ("large_1024x768", lambda: larger_than_image(1024, 768)), ("rejections", rejections),
               ("points_1", lambda: points(1)), ("points_3", lambda: points(3)),
               ("points_5", lambda: points(5)),
               ("shared_edge_small", lambda: shared_edge_small(False)),
               ("shared_edge_small_on_centres", lambda: shared_edge_small(True)),
               ("overlap_small", overlap_small), ("overlap_small_reversed", lambda: overlap_small(order=(2, 1, 0))),
               ("overlap_small_duplicate", lambda: overlap_small(duplicate=True)),
               ("threshold", threshold), ("mixed", mixed), ("mixed_no_twin", lambda: mixed(twin=False)),
               ("mixed_no_points", lambda: mixed(points=False)),
               ("strip_1x130", lambda: strip(True)), ("strip_130x1", lambda: strip(False)),
               ("strip_1x130_px63", lambda: strip(True, 63)), ("strip_130x1_px63", lambda: strip(False, 63)),
               ("points_63", points_63)]
_restated = {}


def restated(name):
    """(the case of that name in SMALL_CASES, its restatement): made once and shared by the tests of both tiers, none of
    which writes to either"""
    if name not in _restated:
        c = dict(SMALL_CASES)[name]()
        _restated[name] = (c, restate(c))
    return _restated[name]


def winner_pairs(c, res):
    """the (winner, loser) pairs of kinds that meet at one pixel at least, from the restatement's candidate list; a kind
    is 'small', 'large' (box_pixels > SMALL_BOX) or 'point', and 'large+' is a large loser in another workgroup than
    the (large) winner's"""
    F = len(c['faces'])
    n_points = 0 if c['points'] is None else len(c['points'])
    kind = np.concatenate([np.where(box_pixels(c) > SMALL_BOX, 1, 0), np.full(n_points, 2)])
    pix, _, prim = res['cand']
    win = res['ids'].reshape(-1)[pix].astype(np.int64)
    lost = prim != win
    win, prim = win[lost], prim[lost]
    names = ('small', 'large', 'point')
    pairs = {(names[a], names[b]) for a, b in set(zip(kind[win].tolist(), kind[prim].tolist()))}
    if ((kind[win] == 1) & (kind[prim] == 1) & (win // RASTER_THREADS != prim // RASTER_THREADS)).any():
        pairs.add(('large', 'large+'))
    return pairs


def ragged_inputs(meshes):
    """meshes: three (vertices, faces) numpy pairs -> (Mesh-like objects, proposal ids, parsed predictions, scan) as
    place_objects and render_scene take them, on the CPU"""
    objs = [types.SimpleNamespace(vertices=torch.from_numpy(np.asarray(v, np.float64)),
                                  faces=torch.from_numpy(np.asarray(f, np.int32))) for v, f in meshes]
    corners = np.zeros((1, 6, 8, 3))
    ids = np.array([4, 1, 3])
    corners[0, ids] = ragged_boxes()
    sem = np.zeros((1, 6), np.int64)
    sem[0, ids] = (2, 7, 11)
    parsed = {'pred_corners_3d_upright_camera': torch.from_numpy(corners), 'pred_sem_cls': torch.from_numpy(sem)}
    return objs, torch.from_numpy(ids).view(1, 3, 1), parsed, ragged_scan()


def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()                                                  # filter type None on every row
    return raw[:, 1:].reshape(h, w, 3)
