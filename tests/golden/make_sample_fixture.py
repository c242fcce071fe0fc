"""Writes tests/golden/F_SMP.npz: what the reference's own code answers about three small closed meshes: is a point inside
(external/libmesh: inside_mesh.py over triangle_hash.pyx), which voxels does the surface touch (external/voxels.py over
libvoxelize/voxelize.pyx and tribox2.h), and the bytes of a .binvox file (external/binvox_rw.py).

    python tests/golden/make_sample_fixture.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

The two .pyx files are cythonized into a temporary directory (the voxeliser with -ffp-contract=off, so that its float32
arithmetic is the source's), the imports that are absent here (trimesh, skimage, the reference's kd-tree) are stubbed, and
the reference's Python runs on them as it lies; neither a binary nor any reference text is kept.

The meshes, the query points and their order are those of tests/mesh_sample_cases.py; the fixture stores the meshes, the
two shared random arrays and the reference's answers."""
import argparse
import importlib
import io
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mesh_sample_cases as cases  # noqa: E402

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
import numpy
ref = %r
setup(ext_modules=cythonize([
    Extension('triangle_hash', [ref + '/external/libmesh/triangle_hash.pyx'], language='c++',
              include_dirs=[numpy.get_include()]),
    Extension('voxelize', [ref + '/external/libvoxelize/voxelize.pyx'],
              include_dirs=[ref + '/external/libvoxelize'], extra_compile_args=['-ffp-contract=off'])],
    build_dir=%r, language_level=3))
"""


def ns(name, path=None):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    sys.modules[name] = m
    return m


def mount_reference(ref, tmp):
    """-> (inside_mesh, voxels, binvox_rw): the reference's modules over the two extensions built in `tmp`"""
    setup = os.path.join(tmp, "setup.py")
    with open(setup, "w") as f:
        f.write(SETUP % (ref, os.path.join(tmp, "build")))
    subprocess.check_call([sys.executable, setup, "build_ext", "--build-lib", tmp, "--build-temp", os.path.join(tmp, "tmp")],
                          cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    import scipy.ndimage  # noqa: F401  (before the aliases: numpy.ma reads np.bool while it loads)
    import torch  # noqa: F401
    np.bool, np.int = np.bool_, int                                     # the reference was written for an older numpy
    ext = ref + "/external"
    ns('external', ext)
    ns('external.libmesh', ext + '/libmesh')
    ns('external.libvoxelize', ext + '/libvoxelize')
    sys.modules['external.libmesh.triangle_hash'] = importlib.import_module("triangle_hash")
    sys.modules['external.libvoxelize.voxelize'] = importlib.import_module("voxelize")
    ns('trimesh')
    ns('skimage')
    ns('skimage.measure').block_reduce = None
    ns('external.libkdtree')
    ns('external.libkdtree.pykdtree')
    ns('external.libkdtree.pykdtree.kdtree').KDTree = None
    inside_mesh = importlib.import_module('external.libmesh.inside_mesh')
    sys.modules['external.libmesh'].check_mesh_contains = inside_mesh.check_mesh_contains
    return inside_mesh, importlib.import_module('external.voxels'), importlib.import_module('external.binvox_rw')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (it holds external/libmesh)")
    ap.add_argument("--out", default=cases.GOLDEN)
    args = ap.parse_args()
    rng = np.random.default_rng(31)
    rand = rng.random((cases.GRID ** 3, 3))
    jitter = 0.1 * (rand - 0.5)                  # what voxelize_interior adds when np.random.rand returns `rand`
    uniform = rng.uniform(-0.55, 0.55, (2000, 3))
    out = {"jitter": jitter, "uniform": uniform}
    with tempfile.TemporaryDirectory() as tmp:
        inside_mesh, voxels, binvox_rw = mount_reference(os.path.abspath(args.reference), tmp)
        np.random.rand = lambda *shape: rand.reshape(shape)
        for name in cases.MESHES:
            v, f = cases.normalised(name)
            mesh = types.SimpleNamespace(vertices=v, faces=f)
            out[name + "_v"], out[name + "_f"] = v, f.astype(np.int32)
            points = cases.query_points(v, f, jitter, uniform)
            for res in cases.HASH_RESOLUTIONS:
                with np.errstate(invalid='ignore'):
                    got = inside_mesh.check_mesh_contains(mesh, points, hash_resolution=res)
                out["%s_contains_%d" % (name, res)] = np.packbits(got)
                print(name, "hash", res, "inside:", int(got.sum()), "of", len(points))
            for R in cases.SURFACE_RESOLUTIONS:
                occ = voxels.voxelize_surface(mesh, R)
                out["%s_surface_%d" % (name, R)] = np.packbits(occ)
                print(name, "surface", R, "voxels:", int(occ.sum()))
            interior = voxels.voxelize_interior(mesh, cases.GRID)
            out[name + "_interior"] = np.packbits(interior)
            out[name + "_ray"] = np.packbits(voxels.voxelize_ray(mesh, cases.GRID))
            print(name, "interior:", int(interior.sum()))
        R = cases.GRID
        grid = np.unpackbits(out["sphere_ray"])[:R ** 3].reshape(R, R, R).astype(bool)
        buf = io.BytesIO()
        binvox_rw.Voxels(grid, (R,) * 3, translate=cases.BINVOX_TRANSLATE, scale=cases.BINVOX_SCALE,
                         axis_order='xyz').write(buf)
        out["binvox"] = np.frombuffer(buf.getvalue(), np.uint8)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
