"""Meshes of the connected-component tests (no test in here; tests/test_components_cpu.py and
tests/test_gpu_components.py import it): built once, never changed.  Every builder returns (vertices (n,3) f64, faces
(m,3) int64, local indices); the small ones build on tests/decimate_cases.py."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_cases as dcases  # noqa: E402

batch = dcases.batch
ONE_FACE = (np.array([[1., 1., 1.], [10., 1., 1.], [1., 10., 1.]]), np.array([[0, 1, 2]]))
EMPTY = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
LOOSE_VERTICES = (np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]), np.zeros((0, 3), np.int64))


def join(parts):
    """[(v, f)] -> ONE mesh: the parts back to back with shifted indices, so one component (at least) per part"""
    v = np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 3) for p in parts])
    at = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    f = np.concatenate([np.asarray(p[1], np.int64).reshape(-1, 3) + at[i] for i, p in enumerate(parts)])
    return v, f


def two_parts(second_first=False):
    """the sphere and the ellipsoid of the decimation tests in ONE mesh: two components that overlap in space.
    second_first: the ellipsoid's faces come first (its vertices still come last): numbering goes by vertex index"""
    s, e = dcases.sphere(), dcases.ellipsoid()
    v, f = join([s, e])
    if second_first:
        f = np.concatenate([f[len(s[1]):], f[:len(s[1])]])
    return v, f


def cavity():
    """the sphere with a copy of half its size inside whose faces are flipped: an inside-out inner shell"""
    v, f = dcases.sphere()
    centre = np.array([7.5, 7.5, 7.5])
    return join([(v, f), (centre + 0.5 * (v - centre), f[:, ::-1])])


FAN_SIZES = (1, 15, 16, 17, 33)


def fans():
    """fans of 1, 15, 16, 17 and 33 faces as the components of one mesh: the tails of the sixteen partial sums"""
    return join([dcases.fan(n, z=0.1 + 0.05 * i, hub=(3. * i, 0.5, 1. + 0.25 * i), phase=0.1 * i)
                 for i, n in enumerate(FAN_SIZES)])


def twins():
    """two fans of five faces and one of three: a tie under `faces`, none under area or volume"""
    return join([dcases.fan(3, z=0.2, hub=(0., 0., 1.)), dcases.fan(5, z=0.3, hub=(3., 0., 1.5)),
                 dcases.fan(5, z=-0.2, hub=(6., 1., 0.5), phase=0.3)])


def bad():
    """seven vertices, the last one NaN; faces: a good one, one with the index -1, one with the index n_v, a degenerate one
    (a, a, b) and one that names the NaN vertex.  Components: {0, 1, 2} and {4, 5, 6}; vertex 3 is in none"""
    v = np.array([[0.5, 0.25, 1.], [1.5, 0.25, 1.], [0.5, 1.25, 2.], [3., 3., 3.], [4., 0., 1.], [5., 1., 1.],
                  [np.nan, 2., 0.5]])
    f = np.array([[0, 1, 2], [2, 3, -1], [3, 4, 7], [4, 4, 5], [5, 6, 4]], np.int64)
    return v, f


def small_meshes():
    """the ragged batch of all the small cases"""
    return [two_parts(), two_parts(True), cavity(), fans(), twins(), bad(), LOOSE_VERTICES, EMPTY, ONE_FACE]


FRACTION = 0.3             # the fraction mode of the selection tests
STRIP_FACES = 20000          # 79 workgroups of 256 threads: all eight XCDs, long chains, contended roots
NUMBERINGS = ('natural', 'reversed', 'bit-reversed', 'random')


def numbering(n, how):
    """-> p (n,) int64, a permutation: vertex i of the natural order becomes vertex p[i]"""
    i = np.arange(n, dtype=np.int64)
    if how == 'natural':
        return i
    if how == 'reversed':
        return i[::-1].copy()
    if how == 'bit-reversed':
        bits = max(1, int(n - 1).bit_length())
        rev = np.zeros(n, np.int64)
        for b in range(bits):
            rev |= ((i >> b) & 1) << (bits - 1 - b)
        rank = np.empty(n, np.int64)
        rank[np.argsort(rev, kind='stable')] = i
        return rank
    if how == 'random':
        return np.random.default_rng(20).permutation(n).astype(np.int64)
    raise ValueError(how)


def renumbered(v, f, p):
    out = np.empty_like(v)
    out[p] = v
    return out, p[f]


@functools.lru_cache(maxsize=None)
def strip(how='natural', pieces=1):
    """a triangle strip of STRIP_FACES faces, face i = (i, i + 1, i + 2) in the natural numbering, cut into `pieces` strips
    of equal length that share no vertex, its vertices renumbered by numbering(., how)"""
    per = STRIP_FACES // pieces
    assert per * pieces == STRIP_FACES
    i = np.arange(per + 2)
    one_v = np.stack([(i // 2).astype(np.float64), (i % 2).astype(np.float64), 0.01 * i], 1)
    one_f = np.stack([i[:-2], i[1:-1], i[2:]], 1).astype(np.int64)
    v = np.concatenate([one_v + [0., 2. * k, 0.] for k in range(pieces)])
    f = np.concatenate([one_f + (per + 2) * k for k in range(pieces)])
    v, f = renumbered(v, f, numbering(len(v), how))
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f
