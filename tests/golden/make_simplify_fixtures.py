"""Writes tests/golden/F_SIMPLIFY.npz: what the reference's own simplifier (external/libsimplify: Simplify.h behind
simplify_mesh.pyx) makes of three closed marching-cubes meshes, and how far its result and the result of this project's
clustering decimation lie from the input.

    python tests/golden/make_simplify_fixtures.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

The .pyx is cythonized into a temporary directory and mesh_simplify(v, f, target) is called on it as it lies; neither a
binary nor any reference text is kept.

The meshes are the marching cubes (tests/mc_ref.py, welded) of three analytic fields on a 32^3 grid in the cube
[-0.5, 0.5]^3: a blobby sphere, a torus and a union of two rounded boxes, a few thousand faces each.  Per mesh, CELLS is
the grid of the clustering decimation (tests/decimate_f64.py over the cube [-0.55, 0.55]^3) and the target is the number
of faces that decimation leaves, so both simplifiers spend the same budget.  Stored per mesh: the input (_v, _f), _cells,
_target, the reference's output (_ref_v, _ref_f), the clustering's (_clu_v, _clu_f), SAMPLES fixed points on each of the
three surfaces (_s_in, _s_ref, _s_clu; tests/simplify_cases.surface_samples, seeds 1, 2, 3) and the two errors
  _E_r, _E_c = simplify_cases.two_sided_rms(input, its samples, result, its samples):
the RMS of the exact point-to-triangle distances in both directions, float64 numpy.  E_r < E_c is checked here."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import decimate_f64 as D  # noqa: E402
import mc_ref  # noqa: E402
import simplify_cases as C  # noqa: E402

GRID, SAMPLES = 32, 1000
CELLS = {"blobby_sphere": 16, "torus": 20, "rounded_boxes": 16}

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
import numpy
ref = %r
setup(ext_modules=cythonize([
    Extension('simplify_mesh', [ref + '/external/libsimplify/simplify_mesh.pyx'], language='c++',
              include_dirs=[numpy.get_include(), ref + '/external/libsimplify'])],
    build_dir=%r, language_level=3))
"""


def fields():
    ax = np.linspace(-0.5, 0.5, GRID)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')

    def rounded_box(cx, cy, cz, hx, hy, hz, r):
        q = np.stack([np.abs(x - cx) - hx, np.abs(y - cy) - hy, np.abs(z - cz) - hz], -1)
        return -(np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0) - r)
    return {
        "blobby_sphere": 0.3 + 0.04 * (np.sin(11 * x) + np.sin(11 * y + 1) + np.sin(11 * z + 2)) - np.sqrt(x * x + y * y + z * z),
        "torus": 0.1 - np.sqrt((np.sqrt(x * x + y * y) - 0.28) ** 2 + z * z),
        "rounded_boxes": np.maximum(rounded_box(-0.08, 0., 0., 0.2, 0.12, 0.1, 0.05),
                                    rounded_box(0.12, 0.05, 0.08, 0.1, 0.2, 0.14, 0.04)),
    }


def mesh_of(field):
    v, f = mc_ref.index_soup(mc_ref.marching_cubes_soup(field, 0.0))
    keep = np.array([len(set(t)) == 3 for t in f.tolist()])               # welding may close a sliver
    return (v - 1.0) / (GRID - 1) - 0.5, f[keep].astype(np.int64)        # the soup is padded by one cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (it holds external/libsimplify)")
    ap.add_argument("--out", default=os.path.join(HERE, "F_SIMPLIFY.npz"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    out = {"names": np.array(list(CELLS))}
    with tempfile.TemporaryDirectory() as tmp:
        setup = os.path.join(tmp, "setup.py")
        with open(setup, "w") as fh:
            fh.write(SETUP % (ref, os.path.join(tmp, "build")))
        subprocess.check_call([sys.executable, setup, "build_ext", "--build-lib", tmp, "--build-temp", os.path.join(tmp, "tmp")],
                              cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        sys.path.insert(0, tmp)
        mesh_simplify = importlib.import_module("simplify_mesh").mesh_simplify
        for name, field in fields().items():
            v, f = mesh_of(field)
            assert C.is_closed_oriented_manifold(f), name
            cells = CELLS[name]
            clu = D.decimate(v, f, [0, len(v)], [0, len(f)], cells)
            cv, cf = clu['v'].astype(np.float64), clu['f']
            target = len(cf)
            rv, rf = mesh_simplify(np.ascontiguousarray(v), np.ascontiguousarray(f), target)
            rv, rf = np.asarray(rv), np.asarray(rf)
            used = np.unique(rf)                                            # the reference leaves unused vertices in
            rv, rf = rv[used], np.searchsorted(used, rf)
            s_in, s_ref, s_clu = (C.surface_samples(a, b, SAMPLES, seed) for a, b, seed in ((v, f, 1), (rv, rf, 2), (cv, cf, 3)))
            E_r = C.two_sided_rms(v, f, s_in, rv, rf, s_ref)
            E_c = C.two_sided_rms(v, f, s_in, cv, cf, s_clu)
            print("%s: %d faces, cells %d -> target %d; reference %d faces; E_r %.6g  E_c %.6g"
                  % (name, len(f), cells, target, len(rf), E_r, E_c))
            assert E_r < E_c, name
            for key, val in (("v", v), ("f", f.astype(np.int32)), ("cells", cells), ("target", target), ("ref_v", rv),
                             ("ref_f", rf.astype(np.int32)), ("clu_v", cv), ("clu_f", cf.astype(np.int32)), ("s_in", s_in),
                             ("s_ref", s_ref), ("s_clu", s_clu), ("E_r", E_r), ("E_c", E_c)):
                out["%s_%s" % (name, key)] = np.asarray(val)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
