"""The scene render restated in numpy float64 / int64 (no test in here; tests/test_render_cpu.py and
tests/test_gpu_render.py import it).  It follows the written rules -- rfdnet_amd/iscnet/scene.py for the placement,
include/rfd_render.h for the rasteriser -- literally and shares no code with the package: every pixel of a primitive's
clamped bounding box is tested and every covering candidate is kept, so that beside the three buffers two margins can be
reported that say whether a comparison for EQUALITY with another implementation is fair:

  min_key_gap      the smallest distance, over the pixels with more than one candidate, between the winner's f32 1/z and
                   the best other candidate's, in f32 units in the last place.  A candidate that is the winner's twin
                   (the same snapped corners and the same q in the same order: its 1/z is the same expression of the same
                   numbers, so it is bit-equal on every IEEE machine and the tie goes to the lower index by rule) does
                   not count as "other".  None: no pixel has two candidates.
  min_snap_margin  the smallest distance, in pixels, of a valid projected coordinate from the point where its snap to
                   1/256 pixel rounds the other way.  None: nothing valid.

A case is admissible if min_key_gap >= 4 (or None) and min_snap_margin >= 1e-6: float64 evaluated in another order (or
with a differently rounded last bit of a quotient) moves a coordinate by some 1e-13 pixels and a 1/z by a fraction of
one f32 unit, so neither a snapped coordinate nor a depth test can come out differently."""
import numpy as np

TRANSFORM_SHAPENET = np.array([[0., 0., -1.], [-1., 0., 0.], [0., 1., 0.]])
POINT_GREY = 0.55
SCREEN_LIMIT = 2.0 ** 20
MIN_KEY_GAP, MIN_SNAP_MARGIN = 4, 1e-6


# ------------------------------------------------------------------------------------------------------ placement ----
def box_from_corners(corners_cam):
    """(8,3) upright-camera corners -> centre (3), sizes (3), heading: depth frame (demo.py:297-310)"""
    c = np.asarray(corners_cam, np.float64)
    d = np.stack([c[:, 0], c[:, 2], -c[:, 1]], 1)
    centre = (d.max(0) + d.min(0)) / 2.
    fwd, left, up = d[1] - d[2], d[0] - d[1], d[6] - d[2]
    return centre, np.array([np.linalg.norm(fwd), np.linalg.norm(left), np.linalg.norm(up)]), np.arctan2(fwd[1], fwd[0])


def place_loop(vertices, faces, corners, normals=None):
    """The six operations of demo.py:351-360, one object at a time.  vertices / faces / normals: lists of (V_k,3) /
    (F_k,3) arrays, corners (K,8,3) -> dict of the SceneMesh fields as numpy arrays (vertices and normals still f64)."""
    out_v, out_f, out_n, face_obj, obj_off, face_off = [], [], [], [], [0], [0]
    with np.errstate(all='ignore'):
        for k, (v, f) in enumerate(zip(vertices, faces)):
            v = np.asarray(v, np.float64).reshape(-1, 3)
            if v.shape[0]:
                centre, sizes, theta = box_from_corners(corners[k])
                rot = np.array([[np.cos(theta), np.sin(theta), 0.], [-np.sin(theta), np.cos(theta), 0.], [0., 0., 1.]])
                p = v - (v.max(0) + v.min(0)) / 2.                            # 1
                p = p.dot(TRANSFORM_SHAPENET.T)                               # 2
                extent = p.max(0) - p.min(0)
                p = p / extent                                                # 3
                p = p * sizes                                                 # 4
                p = p.dot(rot)                                                # 5
                out_v.append(p + centre)                                      # 6
                out_f.append(np.asarray(f, np.int64).reshape(-1, 3) + obj_off[-1])
                face_obj.append(np.full(out_f[-1].shape[0], k, np.int64))
                if normals is not None:
                    n = np.asarray(normals[k], np.float64).dot(TRANSFORM_SHAPENET.T) * (extent / sizes)
                    n = n.dot(rot)
                    out_n.append(n / np.linalg.norm(n, axis=1, keepdims=True))
            obj_off.append(obj_off[-1] + v.shape[0])
            face_off.append(face_off[-1] + (out_f[-1].shape[0] if v.shape[0] else 0))
    cat = lambda parts, shape, dtype: np.concatenate(parts) if parts else np.zeros(shape, dtype)
    return {'vertices': cat(out_v, (0, 3), np.float64), 'faces': cat(out_f, (0, 3), np.int64),
            'face_obj': cat(face_obj, (0,), np.int64), 'obj_off': np.asarray(obj_off), 'face_off': np.asarray(face_off),
            'normals': cat(out_n, (0, 3), np.float64) if normals is not None else None}


# ----------------------------------------------------------------------------------------------------- rasteriser ----
def project(xyz, camera, near):
    """rules 1 and 2 -> q (n) f64, ix, iy (n) int64, valid (n) bool, and the smallest snap margin in pixels (or None)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    m, (fx, fy, cx, cy) = np.asarray(camera, np.float64)[:12].reshape(3, 4), np.asarray(camera, np.float64)[12:]
    X, Y, Z = (xyz[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all='ignore'):
        xv, yv, zv = (((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * Z) + m[r, 3] for r in range(3))
        valid = np.isfinite(xyz).all(1) & (zv >= near)
        q = 1.0 / zv
        sx, sy = (fx * xv) * q + cx, (fy * yv) * q + cy
        valid &= (np.abs(sx) <= SCREEN_LIMIT) & (np.abs(sy) <= SCREEN_LIMIT)
    sx, sy, q = (np.where(valid, a, 0.) for a in (sx, sy, q))
    tx, ty = 256. * sx + 0.5, 256. * sy + 0.5
    ix, iy = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
    ix[~valid], iy[~valid] = 0, 0
    margin = None
    if valid.any():
        frac = np.concatenate([(tx - np.floor(tx))[valid], (ty - np.floor(ty))[valid]])
        margin = float(np.minimum(frac, 1. - frac).min() / 256.)
    return q, ix, iy, valid, margin


def rasterise(vertices, faces, points, camera, near, width, height, point_px=3, face_obj=None, obj_class=None,
              palette=None, eye=(0., 0., 0.)):
    """vertices (V,3) f32, faces (F,3), points (N,3+) or None, camera: the 16 doubles -> {'ids' (H,W) i32, 'depth' (H,W)
    f32, 'image' (H,W,3) u8, 'min_key_gap', 'min_snap_margin', 'candidates': how many (pixel, primitive) pairs,
    'invz_bits' (H,W) i64: the bits of the winner's f32 1/z, the key's high word (0 on the background), 'cand': the
    candidate list itself, three (candidates,) i64 arrays: pixel j W + i, bits of the f32 1/z, primitive}"""
    W, H = int(width), int(height)
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    pts = np.zeros((0, 3), np.float32) if points is None else np.asarray(points, np.float32)[:, :3]
    V, F, N = vertices.shape[0], faces.shape[0], pts.shape[0]
    q, ix, iy, valid, margin = project(np.concatenate([vertices, pts]), camera, near)

    cand_pix, cand_bits, cand_prim, canon, twins = [], [], [], np.arange(F + N), {}

    def twin_of(prim, signature):
        canon[prim] = twins.setdefault(signature, prim)

    for f in range(F):                                                        # rule 3
        tri = faces[f]
        if (tri < 0).any() or (tri >= V).any() or not valid[tri].all():
            continue
        x, y, qq = [int(v) for v in ix[tri]], [int(v) for v in iy[tri]], q[tri]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0:
            continue
        sign = -1 if area < 0 else 1
        i0, i1 = max(-((128 - min(x)) // 256), 0), min((max(x) - 128) // 256, W - 1)       # ceil, floor
        j0, j1 = max(-((128 - min(y)) // 256), 0), min((max(y) - 128) // 256, H - 1)
        if i1 < i0 or j1 < j0:
            continue
        twin_of(f, ('t',) + tuple(x) + tuple(y) + tuple(float(v) for v in qq))
        px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
        py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
        covered, E = np.ones((j1 - j0 + 1, i1 - i0 + 1), bool), []
        for e in range(3):
            a, b = (e + 1) % 3, (e + 2) % 3
            dx, dy = sign * (x[b] - x[a]), sign * (y[b] - y[a])
            Ee = sign * ((x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a]))
            covered &= (Ee > 0) | ((Ee == 0) & bool(dy < 0 or (dy == 0 and dx > 0)))
            E.append(Ee)
        if not covered.any():
            continue
        A = float(sign * area)
        w = [Ee[covered].astype(np.float64) / A for Ee in E]
        invz = ((w[0] * qq[0] + w[1] * qq[1]) + w[2] * qq[2]).astype(np.float32)
        jj, ii = np.nonzero(covered)
        cand_pix.append((jj + j0) * W + (ii + i0))
        cand_bits.append(invz.view(np.uint32).astype(np.int64))
        cand_prim.append(np.full(invz.shape[0], f, np.int64))

    h = int(point_px) // 2
    for n in range(N):                                                        # rule 4
        r = V + n
        if not valid[r]:
            continue
        ci, cj = int(ix[r]) >> 8, int(iy[r]) >> 8
        i0, i1, j0, j1 = max(ci - h, 0), min(ci + h, W - 1), max(cj - h, 0), min(cj + h, H - 1)
        if i1 < i0 or j1 < j0:
            continue
        twin_of(F + n, ('p', ci, cj, float(q[r])))
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing='ij')
        cand_pix.append((jj * W + ii).reshape(-1))
        bits = int(np.float32(q[r]).view(np.uint32))
        cand_bits.append(np.full(jj.size, bits, np.int64))
        cand_prim.append(np.full(jj.size, F + n, np.int64))

    ids = np.full(H * W, -1, np.int32)
    depth = np.full(H * W, np.inf, np.float32)
    gap, n_cand = None, 0
    invz_bits, cand = np.zeros(H * W, np.int64), (np.zeros(0, np.int64),) * 3
    if cand_pix:
        pix, bits, prim = np.concatenate(cand_pix), np.concatenate(cand_bits), np.concatenate(cand_prim)
        n_cand = len(pix)
        key = (bits << 32) | (0xffffffff - prim)                              # < 2^63: 1/z is positive
        best = np.zeros(H * W, np.int64)
        np.maximum.at(best, pix, key)
        hit = best != 0
        win_prim = 0xffffffff - (best & 0xffffffff)
        win_bits = best >> 32
        invz_bits, cand = win_bits, (pix, bits, prim)
        ids[hit] = win_prim[hit].astype(np.int32)
        with np.errstate(all='ignore'):
            depth[hit] = (1.0 / win_bits[hit].astype(np.uint32).view(np.float32).astype(np.float64)).astype(np.float32)
        other = canon[prim] != canon[np.where(hit, win_prim, 0)[pix]]
        if other.any():
            second = np.full(H * W, -1, np.int64)
            np.maximum.at(second, pix[other], bits[other])
            gap = int((win_bits - second)[second >= 0].min())

    image = np.full((H * W, 3), 255, np.uint8)                                 # rule 5
    pal = None if palette is None else np.asarray(palette, np.float32).reshape(-1, 3).astype(np.float64)
    eye = np.asarray(eye, np.float64).astype(np.float32).astype(np.float64)
    to_u8 = lambda c: np.clip(np.floor(255. * c + 0.5), 0, 255).astype(np.uint8)
    is_point = ids >= F
    image[is_point] = to_u8(np.float64(np.float32(POINT_GREY)))
    on_face = np.nonzero((ids >= 0) & ~is_point)[0]
    if len(on_face):
        tri = faces[ids[on_face]]
        a, b, c = (vertices[tri[:, k]].astype(np.float64) for k in range(3))
        nrm = np.cross(b - a, c - a)
        view = eye - ((a + b) + c) / 3.
        with np.errstate(all='ignore'):
            s = 0.3 + 0.7 * np.abs((nrm * view).sum(1)) / (np.sqrt((nrm * nrm).sum(1)) * np.sqrt((view * view).sum(1)))
        s = np.where(np.isnan(s), 0.3, s)
        K, C = len(obj_class), pal.shape[0]
        obj = np.clip(np.asarray(face_obj, np.int64)[ids[on_face]], 0, K - 1)
        cls = np.clip(np.asarray(obj_class, np.int64)[obj], 0, C - 1)
        image[on_face] = to_u8(pal[cls] * s[:, None])
    return {'ids': ids.reshape(H, W), 'depth': depth.reshape(H, W), 'image': image.reshape(H, W, 3), 'min_key_gap': gap,
            'min_snap_margin': margin, 'candidates': n_cand, 'invz_bits': invz_bits.reshape(H, W), 'cand': cand}


def admissible(result):
    return (result['min_key_gap'] is None or result['min_key_gap'] >= MIN_KEY_GAP) and \
        (result['min_snap_margin'] is None or result['min_snap_margin'] >= MIN_SNAP_MARGIN)
