// mesh_iou.hip -- mesh IoU on per-object voxel grids (include/rfd_mesh_eval.h, rules M1 - M5).
//
// Replaces the reference's compute_mesh_iou (net_utils/eval_det.py:27-83), which a 16-process pool
// calls once per (prediction, ground truth) pair: the filled voxel centres of one object are looked
// up in the other object's grid -- another origin, cell size and dimension -- and the other way
// round.  Here every object's grid is a bit set (64 voxels along z per word), one workgroup takes one
// (pair, direction), and a pair of cubes that do not meet -- nearly every pair of a scene -- costs one
// comparison.  The arithmetic is f64 VALU in the order the header writes it (-ffp-contract=off), the
// results are integers: the same on every run.
#include "common.h"

namespace {

constexpr int MIOU_THREADS = 256;
constexpr int MIOU_WAVES = MIOU_THREADS / 64;
constexpr int MIOU_MAX_D = 256, MIOU_MAX_P = 1024, MIOU_MAX_G = 256;
constexpr int PACK_MAX_BLOCKS = 2048;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                            // lane 0 holds the sum
}

// One wave per word: lane l reads voxel z = 64 w + l of the row, the ballot IS the word.
__global__ __launch_bounds__(MIOU_THREADS) void objgrid_pack_kernel(
    int D, int W, const unsigned char *__restrict__ S, const unsigned char *__restrict__ I,
    unsigned long long *__restrict__ words, int *__restrict__ cnt) {
  __shared__ int s_n[MIOU_WAVES], s_s[MIOU_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long total = (long)D * D * W;
  int nU = 0, nS = 0;                                  // meaningful in lane 0
  for (long w = (long)blockIdx.x * MIOU_WAVES + wave; w < total; w += (long)gridDim.x * MIOU_WAVES) {
    const long row = w / W;
    const int z = (int)(w - row * W) * 64 + lane;
    bool s = false, u = false;
    if (z < D) {
      const size_t at = (size_t)row * D + z;
      s = S[at] != 0;
      u = s || I[at] != 0;
    }
    const unsigned long long ws = __ballot(s), wu = __ballot(u);
    if (lane == 0) {
      words[w] = wu;
      nU += __popcll(wu);
      nS += __popcll(ws);
    }
  }
  if (lane == 0) { s_n[wave] = nU; s_s[wave] = nS; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < MIOU_WAVES; ++i) { a += s_n[i]; b += s_s[i]; }
    if (a) atomicAdd(cnt + 0, a);
    if (b) atomicAdd(cnt + 1, b);
  }
}

struct Obj {
  double lo[3], cell;
  int D, W;
  const unsigned long long *words;
};

// -> false: no grid (the table row is taken as such unless everything about it is in range)
__device__ __forceinline__ bool load_obj(Obj &o, int i, const double *frame, const int *dim, const long long *off,
                                         const unsigned long long *words, long long n_words) {
  o.D = dim[i];
  if (o.D < 2 || o.D > MIOU_MAX_D) return false;
  o.W = (o.D + 63) >> 6;
  const long long at = off[i], need = (long long)o.D * o.D * o.W;
  if (at < 0 || at > n_words - need) return false;
  o.words = words + at;
  o.lo[0] = frame[4 * i + 0]; o.lo[1] = frame[4 * i + 1]; o.lo[2] = frame[4 * i + 2];
  o.cell = frame[4 * i + 3];
  const double big = 1.0e300;
  return fabs(o.lo[0]) < big && fabs(o.lo[1]) < big && fabs(o.lo[2]) < big && o.cell > 0.0 && o.cell < big;
}

// M4 on one axis: -> t, or -1 where the point is outside (or NaN)
__device__ __forceinline__ int lookup_axis(double p, double lo, double cell, int D) {
  const double t = floor((p - lo) / cell);
  return (t >= 0.0 && t < (double)D) ? (int)t : -1;
}

// source indices whose centre can fall into [blo, bhi]: a conservative clip, one cell wider on each side
__device__ __forceinline__ void clip_axis(double alo, double acell, int D, double blo, double bhi, int &i0, int &i1) {
  const double f0 = floor((blo - alo) / acell - 0.5) - 1.0;
  const double f1 = ceil((bhi - alo) / acell - 0.5) + 1.0;
  i0 = (int)fmin(fmax(f0, 0.0), (double)D);            // D: an empty range
  i1 = (int)fmin(fmax(f1, -1.0), (double)(D - 1));
}

// blockIdx.x: the pair p * G + g, blockIdx.y: 0 = prediction into ground truth (a_AB), 1 = the other way (a_BA)
__global__ __launch_bounds__(MIOU_THREADS) void mesh_iou_counts_kernel(
    int G, const double *__restrict__ frame_p, const int *__restrict__ dim_p, const long long *__restrict__ off_p,
    const unsigned long long *__restrict__ words_p, long long n_words_p,
    const double *__restrict__ frame_g, const int *__restrict__ dim_g, const long long *__restrict__ off_g,
    const unsigned long long *__restrict__ words_g, long long n_words_g, int *__restrict__ counts) {
  __shared__ int s_part[MIOU_WAVES];
  const int pair = blockIdx.x, dir = blockIdx.y;
  const int p = pair / G, g = pair - p * G;
  int *out = counts + (size_t)pair * 2 + dir;
  Obj P_, G_;
  const bool okp = load_obj(P_, p, frame_p, dim_p, off_p, words_p, n_words_p);
  const bool okg = load_obj(G_, g, frame_g, dim_g, off_g, words_g, n_words_g);
  if (!okp || !okg) {                                  // uniform over the workgroup
    if (threadIdx.x == 0) *out = 0;
    return;
  }
  const Obj &A = dir ? G_ : P_, &B = dir ? P_ : G_;    // A: source, B: target
  const double LA = A.cell * A.D, LB = B.cell * B.D;
  int i0[3], i1[3];
  bool any = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // the early-out: the cubes are apart on this axis (NaN compares false: it falls through to M4)
    if (A.lo[a] + LA < B.lo[a] || B.lo[a] + LB < A.lo[a]) any = false;
    clip_axis(A.lo[a], A.cell, A.D, B.lo[a], B.lo[a] + LB, i0[a], i1[a]);
    if (i0[a] > i1[a]) any = false;
  }
  if (!any) {
    if (threadIdx.x == 0) *out = 0;
    return;
  }
  const int w0 = i0[2] >> 6, w1 = i1[2] >> 6;
  const int nj = i1[1] - i0[1] + 1, nw = w1 - w0 + 1;
  const long items = (long)(i1[0] - i0[0] + 1) * nj * nw;
  int mine = 0;
  for (long it = threadIdx.x; it < items; it += MIOU_THREADS) {
    const int w = w0 + (int)(it % nw);
    const long r = it / nw;
    const int j = i0[1] + (int)(r % nj), i = i0[0] + (int)(r / nj);
    unsigned long long word = A.words[((size_t)i * A.D + j) * A.W + w];
    if (!word) continue;
    const int tx = lookup_axis(A.lo[0] + (i + 0.5) * A.cell, B.lo[0], B.cell, B.D);
    const int ty = lookup_axis(A.lo[1] + (j + 0.5) * A.cell, B.lo[1], B.cell, B.D);
    if (tx < 0 || ty < 0) continue;
    const unsigned long long *brow = B.words + ((size_t)tx * B.D + ty) * B.W;
    while (word) {
      const int k = w * 64 + __ffsll((long long)word) - 1;
      word &= word - 1;
      const int tz = lookup_axis(A.lo[2] + (k + 0.5) * A.cell, B.lo[2], B.cell, B.D);
      if (tz >= 0) mine += (int)((brow[tz >> 6] >> (tz & 63)) & 1ull);
    }
  }
  mine = wave_sum(mine);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < MIOU_WAVES; ++i) total += s_part[i];
    *out = total;
  }
}

__global__ __launch_bounds__(MIOU_THREADS) void mesh_iou_finalize_kernel(
    int P, int G, const int *__restrict__ counts, const int *__restrict__ cnt_p, const int *__restrict__ cnt_g,
    const int *__restrict__ rows_p, const int *__restrict__ rows_g, int K_out, int G_out, double *__restrict__ iou) {
  const int pair = blockIdx.x * MIOU_THREADS + threadIdx.x;
  if (pair >= P * G) return;
  const int p = pair / G, g = pair - p * G;
  const int r = rows_p ? rows_p[p] : p, c = rows_g ? rows_g[g] : g;
  if (r < 0 || r >= K_out || c < 0 || c >= G_out) return;
  const int a_ab = counts[2 * pair], a_ba = counts[2 * pair + 1];
  const int n_a = cnt_p[2 * p], s_a = cnt_p[2 * p + 1], n_b = cnt_g[2 * g], s_b = cnt_g[2 * g + 1];
  double v = 0.0;
  if (s_a > 0 && s_b > 0 && a_ab > 0 && a_ba > 0 && n_a > 0 && n_b > 0) {
    const double a1 = (double)a_ab / (double)n_a, a2 = (double)a_ba / (double)n_b;
    v = (a1 * a2) / (a1 + a2 - a1 * a2);
  }
  iou[(size_t)r * G_out + c] = v;
}

}  // namespace

RFD_API int rfd_objgrid_pack(int D, const unsigned char *S, const unsigned char *I, unsigned long long *words,
                             long long off, long long n_words, int *cnt, void *stream) {
  if (D < 2 || D > MIOU_MAX_D) return rfd_invalid("rfd_objgrid_pack: need 2 <= D <= 256");
  const int W = (D + 63) / 64;
  const long long need = (long long)D * D * W;
  if (off < 0 || n_words < need || off > n_words - need) {
    return rfd_invalid("rfd_objgrid_pack: the object's words do not lie inside the buffer");
  }
  const long long blocks = (need + MIOU_WAVES - 1) / MIOU_WAVES;
  hipLaunchKernelGGL(objgrid_pack_kernel, dim3((unsigned)(blocks < PACK_MAX_BLOCKS ? blocks : PACK_MAX_BLOCKS)),
                     dim3(MIOU_THREADS), 0, (hipStream_t)stream, D, W, S, I, words + off, cnt);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mesh_iou_counts(int P, int G,
                                const double *frame_p, const int *dim_p, const long long *off_p,
                                const unsigned long long *words_p, long long n_words_p,
                                const double *frame_g, const int *dim_g, const long long *off_g,
                                const unsigned long long *words_g, long long n_words_g,
                                int *counts, void *stream) {
  if (P < 0 || G < 0 || P > MIOU_MAX_P || G > MIOU_MAX_G || n_words_p < 0 || n_words_g < 0) {
    return rfd_invalid("rfd_mesh_iou_counts: need 0 <= P <= 1024, 0 <= G <= 256, word counts >= 0");
  }
  if (P == 0 || G == 0) return 0;
  hipLaunchKernelGGL(mesh_iou_counts_kernel, dim3((unsigned)(P * G), 2), dim3(MIOU_THREADS), 0, (hipStream_t)stream,
                     G, frame_p, dim_p, off_p, words_p, n_words_p, frame_g, dim_g, off_g, words_g, n_words_g, counts);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mesh_iou_finalize(int P, int G, const int *counts, const int *cnt_p, const int *cnt_g,
                                  const int *rows_p, const int *rows_g, int K_out, int G_out, double *iou,
                                  void *stream) {
  if (P < 0 || G < 0 || P > MIOU_MAX_P || G > MIOU_MAX_G || K_out < 0 || G_out < 0) {
    return rfd_invalid("rfd_mesh_iou_finalize: need 0 <= P <= 1024, 0 <= G <= 256, K_out and G_out >= 0");
  }
  if (P == 0 || G == 0 || K_out == 0 || G_out == 0) return 0;
  hipLaunchKernelGGL(mesh_iou_finalize_kernel, dim3((unsigned)((P * G + MIOU_THREADS - 1) / MIOU_THREADS)),
                     dim3(MIOU_THREADS), 0, (hipStream_t)stream, P, G, counts, cnt_p, cnt_g, rows_p, rows_g, K_out,
                     G_out, iou);
  RFD_CHECK_LAUNCH();
  return 0;
}
