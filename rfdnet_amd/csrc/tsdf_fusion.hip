// tsdf_fusion.hip -- depth maps out of the rasteriser's key buffer and their fusion into a truncated signed distance
// field (include/rfd_fuse.h; the rules are spelled out there and restated in tests/fuse_ref.py).  The library is built
// with -ffp-contract=off, so every expression below is evaluated as written, and hipcc's f32 division is the correctly
// rounded one.
//
// The fusion is one thread per voxel with the view loop inside: sum and count stay in registers, the view index is the
// same for the whole wave (K, R and T of a view come through scalar loads), and the one irregular access is the gather
// of a depth pixel.  A wave owns a 4x4x4 brick of voxels, so what it gathers from one view is a patch a few pixels
// square, not a line 64 voxels long; a workgroup is four bricks side by side along w, and workgroup ids are dealt so
// that the workgroups that share an L2 hold a contiguous piece of the volume.  No atomics, no LDS, nothing waits.
#include "common.h"
#include "../../include/rfd_fuse.h"

namespace {

constexpr int FUSE_THREADS = 256;
constexpr int BRICK = 4;                   // a wave's voxels: BRICK^3 = 64
constexpr int BRICKS_W = FUSE_THREADS / 64;  // bricks of a workgroup, along w
constexpr int VIEW_BATCH = 4;              // views whose gathers are in flight together
constexpr int MAX_IMAGE = 8192;
constexpr int XCDS = 8;

// rules 2 and 3 for one view (the same for every lane: K, R and T come through scalar loads): the voxel's depth along
// the view and the index of its pixel in the stack, or of the view's first pixel where the voxel is off the image (`on`
// false: the value loaded there is never used), so that the gather itself needs no branch
__device__ __forceinline__ void project(int v, int rows, int cols, float fcols, float frows, const float *__restrict__ Ks,
                                        const float *__restrict__ Rs, const float *__restrict__ Ts, float x, float y,
                                        float z, float &dd, bool &on, unsigned &pixel) {
  const float *K = Ks + 9 * (size_t)v, *R = Rs + 9 * (size_t)v, *T = Ts + 3 * (size_t)v;
  const float xt = ((R[0] * x + R[1] * y) + R[2] * z) + T[0];
  const float yt = ((R[3] * x + R[4] * y) + R[5] * z) + T[1];
  const float zt = ((R[6] * x + R[7] * y) + R[8] * z) + T[2];
  float pu = (K[0] * xt + K[1] * yt) + K[2] * zt;
  float pv = (K[3] * xt + K[4] * yt) + K[5] * zt;
  dd = (K[6] * xt + K[7] * yt) + K[8] * zt;
  pu = pu / dd, pv = pv / dd;
  const float tu = pu + 0.5f, tv = pv + 0.5f;
  on = (tu > -1.f) & (tu < fcols) & (tv > -1.f) & (tv < frows);      // false for a NaN
  // only a float that passed becomes an integer: 0 <= (int)t < size <= 8192, so 24-bit arithmetic holds the product;
  // V rows cols < 2^31
  const int row = (int)(on ? tv : 0.f), col = (int)(on ? tu : 0.f);
  pixel = (unsigned)v * (unsigned)(rows * cols) + (unsigned)__mul24(row, cols) + (unsigned)col;
}

// rule 4
__device__ __forceinline__ void sample(float g, float dd, bool on, float truncation, int unknown_is_free, float &sum,
                                       int &n) {
  if (unknown_is_free && g < 0.f) g = 1e9f;
  const float dist = g - dd;
  const bool valid = on & (g > 0.f) & (dist >= -truncation);
  sum = valid ? sum + fminf(truncation, fmaxf(-truncation, dist)) : sum;
  n += valid ? 1 : 0;
}

// the views [v0, v1) of the stack; first: sum and count start at 0, else they are read from tsdf / count; last: the
// result is written (rule 5), else sum and count go back to tsdf / count
__global__ __launch_bounds__(FUSE_THREADS) void tsdf_fuse_kernel(
    int v0, int v1, int first, int last, int rows, int cols, const float *__restrict__ depth,
    const float *__restrict__ Ks, const float *__restrict__ Rs, const float *__restrict__ Ts, int D, int H, int W,
    int tiles_w, int tiles_h, unsigned n_tiles, float vx_size, float truncation, int unknown_is_free,
    float unobserved_value, float *__restrict__ tsdf, int *__restrict__ count) {
  // workgroups that differ by a multiple of XCDS share an L2: give each of the XCDS classes one contiguous run of tiles
  const unsigned per = n_tiles / XCDS;
  unsigned tile = blockIdx.x;
  if (tile < per * XCDS) tile = (tile % XCDS) * per + tile / XCDS;
  const int tw = (int)(tile % (unsigned)tiles_w), th = (int)((tile / (unsigned)tiles_w) % (unsigned)tiles_h),
            td = (int)(tile / ((unsigned)tiles_w * (unsigned)tiles_h));
  const int lane = threadIdx.x & 63, brick = threadIdx.x >> 6;
  const int w = (tw * BRICKS_W + brick) * BRICK + (lane & 3), h = th * BRICK + ((lane >> 2) & 3),
            d = td * BRICK + (lane >> 4);
  if (w >= W || h >= H || d >= D) return;
  const size_t vox = ((size_t)d * H + h) * W + w;
  const float x = (float)((w + 0.5) * (double)vx_size - 0.5);
  const float y = (float)((h + 0.5) * (double)vx_size - 0.5);
  const float z = (float)((d + 0.5) * (double)vx_size - 0.5);
  float sum = 0.f;
  int n = 0;
  if (!first) sum = tsdf[vox], n = count[vox];
  const float fcols = (float)cols, frows = (float)rows;
  int v = v0;
  for (; v + VIEW_BATCH <= v1; v += VIEW_BATCH) {   // the gathers of VIEW_BATCH views are in flight together
    float g[VIEW_BATCH], dd[VIEW_BATCH];
    bool on[VIEW_BATCH];
#pragma unroll
    for (int j = 0; j < VIEW_BATCH; ++j) {
      unsigned pixel;
      project(v + j, rows, cols, fcols, frows, Ks, Rs, Ts, x, y, z, dd[j], on[j], pixel);
      g[j] = depth[pixel];
    }
#pragma unroll
    for (int j = 0; j < VIEW_BATCH; ++j) sample(g[j], dd[j], on[j], truncation, unknown_is_free, sum, n);   // in view order
  }
  for (; v < v1; ++v) {
    float dd;
    bool on;
    unsigned pixel;
    project(v, rows, cols, fcols, frows, Ks, Rs, Ts, x, y, z, dd, on, pixel);
    sample(depth[pixel], dd, on, truncation, unknown_is_free, sum, n);
  }
  if (last) {
    tsdf[vox] = n > 0 ? sum / (float)n : unobserved_value;
    if (count) count[vox] = n;
  } else {
    tsdf[vox] = sum, count[vox] = n;
  }
}

__device__ __forceinline__ float key_depth(unsigned long long key, float far, float offset) {
  float z = far;
  if (key != 0) {
    z = (float)(1.0 / (double)__uint_as_float((unsigned)(key >> 32)));
    if (z > far) z = far;
  }
  return z - offset;
}

// rule 6: one thread per pixel
__global__ __launch_bounds__(FUSE_THREADS) void depth_from_keys_kernel(int W, int H,
                                                                       const unsigned long long *__restrict__ keys,
                                                                       float far, float offset,
                                                                       float *__restrict__ depth) {
  const int pix = blockIdx.x * FUSE_THREADS + threadIdx.x;      // W H <= 2^26
  if (pix >= W * H) return;
  const int i = pix % W, j = pix / W;
  const int i0 = max(i - 1, 0), i1 = min(i + 1, W - 1), j0 = max(j - 1, 0), j1 = min(j + 1, H - 1);
  float m = key_depth(keys[pix], far, offset);
  for (int jj = j0; jj <= j1; ++jj)
    for (int ii = i0; ii <= i1; ++ii) m = fminf(m, key_depth(keys[(size_t)jj * W + ii], far, offset));
  depth[pix] = m;
}

}  // namespace

RFD_API int rfd_depth_from_keys(int W, int H, const unsigned long long *keys, float far, float offset, float *depth,
                                void *stream) {
  if (W < 1 || H < 1 || W > MAX_IMAGE || H > MAX_IMAGE) return rfd_invalid("rfd_depth_from_keys: 1 <= W, H <= 8192");
  if (!keys || !depth) return rfd_invalid("rfd_depth_from_keys: no keys or no depth");
  depth_from_keys_kernel<<<(unsigned)ceil_div(W * H, FUSE_THREADS), FUSE_THREADS, 0, (hipStream_t)stream>>>(
      W, H, keys, far, offset, depth);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_tsdf_fuse(int V, int rows, int cols, const float *depth, const float *K, const float *R, const float *T,
                          int D, int H, int W, float vx_size, float truncation, int unknown_is_free,
                          float unobserved_value, int view_chunk, float *tsdf, int *count, void *stream) {
  if (V < 0 || D < 0 || H < 0 || W < 0 || view_chunk < 0) return rfd_invalid("rfd_tsdf_fuse: a negative size");
  if (rows < 1 || cols < 1 || rows > MAX_IMAGE || cols > MAX_IMAGE)
    return rfd_invalid("rfd_tsdf_fuse: 1 <= rows, cols <= 8192");
  if ((long)D * H > INT_MAX || (long)D * H * W > INT_MAX) return rfd_invalid("rfd_tsdf_fuse: D H W must stay below 2^31");
  if ((long)V * rows * cols > INT_MAX) return rfd_invalid("rfd_tsdf_fuse: V rows cols must stay below 2^31");
  if ((long)D * H * W == 0) return 0;
  if (!tsdf) return rfd_invalid("rfd_tsdf_fuse: no tsdf");
  if (V > 0 && (!depth || !K || !R || !T)) return rfd_invalid("rfd_tsdf_fuse: no depth, K, R or T");
  const int tiles_w = ceil_div(W, BRICK * BRICKS_W), tiles_h = ceil_div(H, BRICK), tiles_d = ceil_div(D, BRICK);
  const long n_tiles = (long)tiles_w * tiles_h * tiles_d;      // <= 2^31 / 4 + a rim: below 2^31 (a 1 x 1 x D volume)
  if (n_tiles > INT_MAX) return rfd_invalid("rfd_tsdf_fuse: too many tiles");
  // the library's choice: one launch over every view ("Watertight": the measured alternatives)
  const int chunk = (view_chunk == 0 || !count || view_chunk >= V) ? (V > 0 ? V : 1) : view_chunk;
  int v0 = 0;
  do {
    const int v1 = v0 + chunk < V ? v0 + chunk : V;
    tsdf_fuse_kernel<<<(unsigned)n_tiles, FUSE_THREADS, 0, (hipStream_t)stream>>>(
        v0, v1, v0 == 0, v1 == V, rows, cols, depth, K, R, T, D, H, W, tiles_w, tiles_h, (unsigned)n_tiles, vx_size,
        truncation, unknown_is_free, unobserved_value, tsdf, count);
    RFD_CHECK_LAUNCH();
    v0 = v1;
  } while (v0 < V);
  return 0;
}
