"""Writes tests/golden/F_FUSE.npz: what the reference's CPU fusion (external/pyfusion: fusion.cpp + fusion.h) makes of a
small stack of depth maps.

    python tests/golden/make_fuse_fixture.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

A driver of this project's own (below: a `main` that reads arrays from a file, calls fusion_tsdf_cpu and
fusion_tsdfmask_cpu, writes arrays to a file) is written into a temporary directory and compiled there with g++ -O2
against the reference's two files; neither the binary nor any reference text is kept.

The set-up: a volume of (11, 20, 15) voxels (not a cube; 3300 is no multiple of 64) of size 1/16, so that it reaches
beyond what the views see; the first 5 of views_on_sphere(7) at distance 1 with images of 40 x 56 and
K = [[40, 0, 27.5], [0, 40, 20.25], [0, 0, 1]]; the depth of a sphere of radius 0.3 around the origin in front of a
background at 1.75, with noise of 0.01, 3 % of the pixels set to -1 and 3 % to 0."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SHAPE = (11, 20, 15)
VX_SIZE = 1. / 16
TRUNCATION = 0.15
ROWS, COLS, VIEWS = 40, 56, 5
FOCAL, CX, CY = 40., 27.5, 20.25

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fusion.h"

static void read_all(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv) {
  if (argc != 3) return 1;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 1;
  int head[6];                                   // views, rows, cols, D, H, W
  float scal[2];                                 // vx_size, truncation
  read_all(in, head, sizeof head);
  read_all(in, scal, sizeof scal);
  const size_t V = head[0], pix = (size_t)head[1] * head[2], vox = (size_t)head[3] * head[4] * head[5];
  std::vector<float> depth(V * pix), K(V * 9), R(V * 9), T(V * 3), out(vox);
  read_all(in, depth.data(), depth.size() * 4);
  read_all(in, K.data(), K.size() * 4);
  read_all(in, R.data(), R.size() * 4);
  read_all(in, T.data(), T.size() * 4);
  fclose(in);
  Views views;
  views.n_views_ = head[0], views.rows_ = head[1], views.cols_ = head[2];
  views.depthmaps_ = depth.data(), views.Ks_ = K.data(), views.Rs_ = R.data(), views.Ts_ = T.data();
  Volume vol;
  vol.channels_ = 1, vol.depth_ = head[3], vol.height_ = head[4], vol.width_ = head[5], vol.data_ = out.data();
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 1;
  for (int free_ = 0; free_ < 2; ++free_) {      // tsdf, mask for unknown_is_free = 0, then for 1
    fusion_tsdf_cpu(views, scal[0], scal[1], free_ != 0, 1, vol);
    fwrite(out.data(), 4, vox, o);
    fusion_tsdfmask_cpu(views, scal[0], scal[1], free_ != 0, 1, vol);
    fwrite(out.data(), 4, vox, o);
  }
  fclose(o);
  return 0;
}
"""


def depth_maps(rng):
    v, u = np.meshgrid(np.arange(ROWS, dtype=np.float64), np.arange(COLS, dtype=np.float64), indexing='ij')
    ray = np.stack([(u - CX) / FOCAL, (v - CY) / FOCAL, np.ones_like(u)], -1)          # points at depth 1 (z = 1)
    # |t ray - (0,0,1)|^2 = 0.3^2, the nearer root; t is the depth since ray_z = 1
    a, b, c = (ray ** 2).sum(-1), -2 * ray[..., 2], 1 - 0.3 ** 2
    disc = b ** 2 - 4 * a * c
    sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 1.75)
    maps = np.repeat(sphere[None], VIEWS, 0) + rng.normal(0, 0.01, (VIEWS, ROWS, COLS))
    draw = rng.uniform(0, 1, maps.shape)
    maps[draw < 0.03] = -1.
    maps[draw > 0.97] = 0.
    return maps.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (it holds external/pyfusion)")
    ap.add_argument("--out", default=os.path.join(HERE, "F_FUSE.npz"))
    args = ap.parse_args()
    from rfdnet_amd.watertight import views_on_sphere
    fusion = os.path.join(args.reference, "external", "pyfusion")
    rng = np.random.default_rng(20)
    depth = depth_maps(rng)
    R = views_on_sphere(7)[:VIEWS].astype(np.float32).reshape(VIEWS, 9)
    K = np.tile(np.array([FOCAL, 0, CX, 0, FOCAL, CY, 0, 0, 1], np.float32), (VIEWS, 1))
    T = np.tile(np.array([0, 0, 1], np.float32), (VIEWS, 1))
    vox = int(np.prod(SHAPE))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, n) for n in ("driver.cpp", "driver", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O2", "-I" + fusion, src, os.path.join(fusion, "fusion.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.array([VIEWS, ROWS, COLS] + list(SHAPE), np.int32).tobytes())
            f.write(np.array([VX_SIZE, TRUNCATION], np.float32).tobytes())
            for a in (depth, K, R, T):
                f.write(a.tobytes())
        subprocess.check_call([exe, fin, fout])
        out = np.fromfile(fout, np.float32).reshape(4, *SHAPE)
    assert out.size == 4 * vox
    np.savez_compressed(args.out, depth=depth, K=K, R=R, T=T, shape=np.array(SHAPE, np.int32),
                        vx_size=np.float32(VX_SIZE), truncation=np.float32(TRUNCATION),
                        tsdf_free0=out[0], mask_free0=out[1].astype(np.uint8), tsdf_free1=out[2],
                        mask_free1=out[3].astype(np.uint8))
    for k in (0, 1):
        mask = out[2 * k + 1]
        print("unknown_is_free=%d: observed %.1f %%" % (k, 100 * mask.mean()))
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
