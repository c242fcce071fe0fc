"""Numpy restatements of include/rfd_sample.h (no test in here; tests/test_mesh_sample_cpu.py and
tests/test_gpu_mesh_sample.py import it): containment C1 - C6 over ALL triangles (no cells: they only filter), the surface
voxels V1 - V4 in float32, the surface samples S1 - S4.  numpy evaluates every operation on its own (no fused
multiply-add), which is what the rules ask for."""
import numpy as np


def rescale_constants(vertices, faces, resolution):
    """rule C1 -> scale (3,), translate (3,)"""
    tri = np.asarray(vertices, np.float64)[np.asarray(faces)].reshape(-1, 3)
    lo, hi = tri.min(0), tri.max(0)
    scale = (resolution - 1) / (hi - lo)
    return scale, 0.5 - scale * lo


def contains(vertices, faces, points, resolution=512, chunk=2048):
    """-> contains (n,) bool, n0 (n,) i32, n1 (n,) i32"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    n = points.shape[0]
    n0, n1 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if faces.shape[0] == 0 or n == 0:
        return np.zeros(n, bool), n0, n1
    scale, translate = rescale_constants(vertices, faces, resolution)
    tri = scale * np.asarray(vertices, np.float64)[faces] + translate                 # C2
    with np.errstate(invalid='ignore'):
        p = scale * points + translate
        candidate = ((0 <= p) & (p <= resolution)).all(1) & (p[:, 0] < resolution) & (p[:, 1] < resolution)      # C3
    t1, t2, t3 = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    A00, A10, A01, A11 = t1[..., 0] - t3[..., 0], t1[..., 1] - t3[..., 1], t2[..., 0] - t3[..., 0], t2[..., 1] - t3[..., 1]
    det = A00 * A11 - A01 * A10                                                        # C4
    s, ad = np.sign(det), np.abs(det)
    v1, v2 = t3 - t1, t2 - t1                                                          # C5
    nn0 = v1[..., 1] * v2[..., 2] - v1[..., 2] * v2[..., 1]
    nn1 = v1[..., 2] * v2[..., 0] - v1[..., 0] * v2[..., 2]
    nn2 = v1[..., 0] * v2[..., 1] - v1[..., 1] * v2[..., 0]
    an, sn = np.abs(nn2), np.sign(nn2)
    idx = np.nonzero(candidate)[0]
    for a in range(0, len(idx), chunk):
        rows = idx[a:a + chunk]
        q = p[rows][:, None, :]
        y0, y1 = q[..., 0] - t3[..., 0], q[..., 1] - t3[..., 1]
        u = (A11 * y0 - A01 * y1) * s
        v = (-A10 * y0 + A00 * y1) * s
        w = u + v
        hit = (det != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < w) & (w < ad)
        alpha = nn0 * (t1[..., 0] - q[..., 0]) + nn1 * (t1[..., 1] - q[..., 1])
        depth = t1[..., 2] * an + alpha * sn
        rhs = q[..., 2] * an
        hit &= nn2 != 0
        n0[rows] = (hit & (depth >= rhs)).sum(1)
        n1[rows] = (hit & (depth < rhs)).sum(1)
    return (n0 % 2 == 1) & (n1 % 2 == 1), n0, n1                                       # C6


def _cell(x, last):
    """(int)x clamped to [0, last] for finite x within the int range"""
    return np.clip(np.trunc(x).astype(np.int64), 0, last)


def tri_box_overlap(tri, centre):
    """rule V3: tri (..., 3, 3) f32 against unit voxels with centre (..., 3) f32 -> bool"""
    f = np.float32
    h = f(0.5)
    v0, v1, v2 = (tri[..., c, :] - centre for c in range(3))
    e0, e1, e2 = v1 - v0, v2 - v1, v0 - v2
    X, Y, Z = 0, 1, 2
    ok = np.ones(v0.shape[:-1], bool)

    def axis(pa, pb, fa, fb):
        mn, mx = np.where(pa < pb, pa, pb), np.where(pa < pb, pb, pa)
        rad = fa * h + fb * h
        return ~((mn > rad) | (mx < -rad))

    def x_test(e, va, vb):
        a, b = e[..., Z], e[..., Y]
        return axis(a * va[..., Y] - b * va[..., Z], a * vb[..., Y] - b * vb[..., Z], np.abs(a), np.abs(b))

    def y_test(e, va, vb):
        a, b = e[..., Z], e[..., X]
        return axis(-a * va[..., X] + b * va[..., Z], -a * vb[..., X] + b * vb[..., Z], np.abs(a), np.abs(b))

    def z_test(e, va, vb):
        a, b = e[..., Y], e[..., X]
        return axis(a * va[..., X] - b * va[..., Y], a * vb[..., X] - b * vb[..., Y], np.abs(a), np.abs(b))

    ok &= x_test(e0, v0, v2) & y_test(e0, v0, v2) & z_test(e0, v1, v2)
    ok &= x_test(e1, v0, v2) & y_test(e1, v0, v2) & z_test(e1, v0, v1)
    ok &= x_test(e2, v0, v1) & y_test(e2, v0, v1) & z_test(e2, v1, v2)
    for a in range(3):
        c = np.stack([v0[..., a], v1[..., a], v2[..., a]])
        ok &= ~((c.min(0) > h) | (c.max(0) < -h))
    n0 = e0[..., Y] * e1[..., Z] - e0[..., Z] * e1[..., Y]
    n1 = e0[..., Z] * e1[..., X] - e0[..., X] * e1[..., Z]
    n2 = e0[..., X] * e1[..., Y] - e0[..., Y] * e1[..., X]
    d = -((n0 * v0[..., X] + n1 * v0[..., Y]) + n2 * v0[..., Z])
    m0, m1, m2 = (np.where(n > 0, -h, h).astype(f) for n in (n0, n1, n2))
    ok &= ~(((n0 * m0 + n1 * m1) + n2 * m2) + d > 0)
    ok &= ((n0 * -m0 + n1 * -m1) + n2 * -m2) + d >= 0
    return ok


def voxelize_surface(vertices, faces, resolution):
    """rules V1 - V4 -> (R,R,R) bool"""
    R = int(resolution)
    occ = np.zeros((R, R, R), bool)
    faces = np.asarray(faces).reshape(-1, 3)
    if faces.shape[0] == 0:
        return occ
    tri = ((np.asarray(vertices, np.float64) + 0.5) * R)[faces].astype(np.float32)      # V1
    lo, hi = _cell(tri.min(1), R - 1), _cell(tri.max(1), R - 1)                             # V2
    for t, a, b in zip(tri, lo, hi):
        ijk = np.stack(np.meshgrid(*[np.arange(a[c], b[c] + 1) for c in range(3)], indexing='ij'), -1).reshape(-1, 3)
        centre = (ijk + 0.5).astype(np.float32)
        hit = tri_box_overlap(t[None], centre)                                              # V3
        occ[tuple(ijk[hit].T)] = True                                                       # V4
    return occ


def grid_points(resolution, jitter):
    R = int(resolution)
    c = (np.arange(R, dtype=np.float32) + np.float32(0.5)).astype(np.float64)
    grid = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    return (grid + np.asarray(jitter, np.float64)) / R - 0.5


def voxelize_interior(vertices, faces, resolution, jitter):
    return contains(vertices, faces, grid_points(resolution, jitter))[0].reshape((int(resolution),) * 3)


def face_cross(tri):
    a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def face_areas(vertices, faces):
    """rule S1"""
    c = face_cross(np.asarray(vertices, np.float64)[np.asarray(faces).reshape(-1, 3)])
    return 0.5 * np.sqrt((c[:, 0] ** 2 + c[:, 1] ** 2) + c[:, 2] ** 2)


def sequential_prefix(areas):
    """the inclusive prefix summed one term after the other (np.cumsum's order)"""
    return np.cumsum(np.asarray(areas, np.float64))


def pick_faces(cum, u0):
    """rule S2"""
    return np.minimum(np.searchsorted(cum, u0 * cum[-1], side='left'), len(cum) - 1)


def sample_at(vertices, faces, face_index, u):
    """rules S3, S4 at the given faces -> points (n,3) f64, normals (n,3) f64"""
    tri = np.asarray(vertices, np.float64)[np.asarray(faces).reshape(-1, 3)][face_index]
    a, b = u[:, 1].copy(), u[:, 2].copy()
    flip = a + b > 1
    a[flip], b[flip] = np.abs(a[flip] - 1), np.abs(b[flip] - 1)
    p = tri[:, 0] + ((tri[:, 1] - tri[:, 0]) * a[:, None] + (tri[:, 2] - tri[:, 0]) * b[:, None])
    c = face_cross(tri)
    length = np.sqrt((c[:, 0] ** 2 + c[:, 1] ** 2) + c[:, 2] ** 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(length[:, None] == 0, 0., c / length[:, None])
    return p, normals
