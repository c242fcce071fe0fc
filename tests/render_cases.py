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
               ("points_5", lambda: points(5))]


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
