// scan_labels.hip -- scan ground truth on the device: instance boxes, CAD box extents, CAD-to-instance matching, point
// votes and the dataloader's per-point sample.  The rules (A, E, K, M, P, S) are written out in include/rfd_labels.h
// and restated in numpy in tests/scan_labels_f64.py; the reference's own output is tests/golden/F_SCAN.npz.
//
// The stages are memory-light (a 150 000-vertex scan is 3.6 MB of f32 rows): what matters here is that the two
// reductions give the same bits on every run.  Both reduce in registers, across the wave with shuffles and across the
// workgroup in LDS, and end in ONE integer atomic min / max per destination and workgroup on order-preserving keys
// (rule K); there is no float atomic in this file.
#include "common.h"
#include "../../include/rfd_labels.h"
#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

// ---- rule K ----------------------------------------------------------------------------------------------------------
constexpr unsigned SIGN32 = 0x80000000u;
constexpr unsigned long long SIGN64 = 0x8000000000000000ull;

__device__ __forceinline__ unsigned key32(float x) {
  const unsigned b = __float_as_uint(x + 0.f);
  return (b & SIGN32) ? ~b : (b ^ SIGN32);
}
__device__ __forceinline__ float unkey32(unsigned k) { return __uint_as_float((k & SIGN32) ? (k ^ SIGN32) : ~k); }
__device__ __forceinline__ unsigned long long key64(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x + 0.);
  return (b & SIGN64) ? ~b : (b ^ SIGN64);
}
__device__ __forceinline__ double unkey64(unsigned long long k) {
  return __longlong_as_double((long long)((k & SIGN64) ? (k ^ SIGN64) : ~k));
}

// ---- rule A: instance boxes ------------------------------------------------------------------------------------------
constexpr int AABB_PER_THREAD = 8;      // vertices per thread: a workgroup covers 2048 consecutive vertices
constexpr int AABB_TABLE = 256;         // instances 1 .. 256 have a row in LDS, later ones go to global memory directly

// keys (rows,6): the first three of a row are minima (all ones), the last three maxima (0)
__global__ __launch_bounds__(THREADS) void aabb_init_kernel(int n, unsigned *__restrict__ keys) {
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e < n) keys[e] = (e % 6 < 3) ? ~0u : 0u;
}

// one instance's six keys into its row: LDS for a row of the table, global memory otherwise
__device__ __forceinline__ void aabb_put(unsigned *s_key, unsigned *keys, int row, const unsigned lo[3],
                                         const unsigned hi[3]) {
  unsigned *dst = row < AABB_TABLE ? s_key + row * 6 : keys + (size_t)row * 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(dst + a, lo[a]);
    atomicMax(dst + 3 + a, hi[a]);
  }
}

__global__ __launch_bounds__(THREADS) void instance_aabb_kernel(int N, int I, int stride, const float *__restrict__ v,
                                                                const unsigned *__restrict__ ids,
                                                                unsigned *__restrict__ keys) {
  __shared__ unsigned s_key[AABB_TABLE * 6];
  const int tid = threadIdx.x;
  const int table = (I < AABB_TABLE ? I : AABB_TABLE) * 6;
  for (int e = tid; e < table; e += THREADS) s_key[e] = (e % 6 < 3) ? ~0u : 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * (THREADS * AABB_PER_THREAD);
  for (int k = 0; k < AABB_PER_THREAD; ++k) {                       // every lane runs every round (the shuffles below)
    const long long i = base + (long long)k * THREADS + tid;
    unsigned id = 0;
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    if (i < N) {
      id = ids[i];
      if (id >= 1u && id <= (unsigned)I) {
        const float *p = v + (size_t)i * stride;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = key32(p[a]);
      } else {
        id = 0;
      }
    }
    const unsigned first = __shfl(id, 0);
    if (__all(id == first)) {                                       // a scan's vertices mostly come instance by instance
      if (first != 0) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const unsigned l = __shfl_xor(lo[a], off), h = __shfl_xor(hi[a], off);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
          }
        }
        if ((tid & 63) == 0) aabb_put(s_key, keys, (int)first - 1, lo, hi);
      }
    } else if (id != 0) {
      aabb_put(s_key, keys, (int)id - 1, lo, hi);
    }
  }
  __syncthreads();
  for (int e = tid; e < table; e += THREADS) {                      // the table's rows are the first rows of `keys`
    const unsigned k = s_key[e];
    if (e % 6 < 3) {
      if (k != ~0u) atomicMin(keys + e, k);
    } else {
      if (k != 0u) atomicMax(keys + e, k);
    }
  }
}

__global__ __launch_bounds__(THREADS) void aabb_finish_kernel(int n, const unsigned *__restrict__ keys,
                                                              float *__restrict__ box) {
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e < n) box[e] = keys[(e / 6) * 6] == ~0u ? 0.f : unkey32(keys[e]);
}

// ---- rule E: CAD extents ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void extents_init_kernel(int n, unsigned long long *__restrict__ keys) {
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e < n) keys[e] = ((e % 12) / 3) % 2 == 0 ? ~0ull : 0ull;     // min p, max p, min q, max q
}

__global__ __launch_bounds__(THREADS) void cad_extents_kernel(int M, int step, const double *__restrict__ pts,
                                                              const int *__restrict__ off, const int *__restrict__ owner,
                                                              const int *__restrict__ start, const double *__restrict__ L,
                                                              unsigned long long *__restrict__ keys) {
  __shared__ unsigned long long s_part[WAVES][12];
  const int tid = threadIdx.x, r = blockIdx.x;
  const int m = owner[r];
  if (m < 0 || m >= M) return;                                      // uniform: the whole workgroup leaves
  const int beg = start[r], lim = off[m + 1];
  if (beg < off[m]) return;
  const int end = (long long)beg + step < lim ? beg + step : lim;
  double l[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) l[j] = L[(size_t)m * 9 + j];
  double lo[6], hi[6];
  bool any = false;
  for (int i = beg + tid; i < end; i += THREADS) {
    const double *p = pts + (size_t)i * 3;
    const double x = p[0], y = p[1], z = p[2];
    const double val[6] = {x, y, z, (l[0] * x + l[1] * y) + l[2] * z, (l[3] * x + l[4] * y) + l[5] * z,
                           (l[6] * x + l[7] * y) + l[8] * z};
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      lo[a] = any ? fmin(lo[a], val[a]) : val[a];
      hi[a] = any ? fmax(hi[a], val[a]) : val[a];
    }
    any = true;
  }
  unsigned long long k[12];                                         // the order of ext: min p, max p, min q, max q
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    k[a] = any ? key64(lo[a]) : ~0ull;
    k[3 + a] = any ? key64(hi[a]) : 0ull;
    k[6 + a] = any ? key64(lo[3 + a]) : ~0ull;
    k[9 + a] = any ? key64(hi[3 + a]) : 0ull;
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
#pragma unroll
    for (int a = 0; a < 12; ++a) {
      const unsigned long long o = __shfl_xor(k[a], sh);
      const bool is_min = (a / 3) % 2 == 0;
      k[a] = is_min ? (o < k[a] ? o : k[a]) : (o > k[a] ? o : k[a]);
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 12; ++a) s_part[tid >> 6][a] = k[a];
  }
  __syncthreads();
  if (tid < 12) {
    const bool is_min = (tid / 3) % 2 == 0;
    unsigned long long best = s_part[0][tid];
    for (int w = 1; w < WAVES; ++w) {
      const unsigned long long o = s_part[w][tid];
      best = is_min ? (o < best ? o : best) : (o > best ? o : best);
    }
    if (is_min) atomicMin(keys + (size_t)m * 12 + tid, best);
    else atomicMax(keys + (size_t)m * 12 + tid, best);
  }
}

__global__ __launch_bounds__(THREADS) void extents_finish_kernel(int n, const unsigned long long *__restrict__ keys,
                                                                 double *__restrict__ ext) {
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e < n) ext[e] = unkey64(keys[e]);
}

// ---- rule M: matching ------------------------------------------------------------------------------------------------
struct P2 {
  double x, y;
};
constexpr int CLIP_CAP = 12;            // a quadrilateral cut by four half-planes has at most 8 corners

// keep the side v >= bound (ge) or v <= bound of the polygon in[0 .. n) on axis 0 (x) or 1 (y) -> the corner count
__device__ int clip_half_plane(const P2 *in, int n, P2 *out, int axis, double bound, bool ge) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const P2 p = in[i], q = in[i + 1 < n ? i + 1 : 0];
    const double pv = axis ? p.y : p.x, qv = axis ? q.y : q.x;
    const bool pin = ge ? pv >= bound : pv <= bound, qin = ge ? qv >= bound : qv <= bound;
    if (pin && m < CLIP_CAP) out[m++] = p;
    if (pin != qin && m < CLIP_CAP) {
      const double t = (bound - pv) / (qv - pv);
      P2 c;
      c.x = axis ? p.x + (q.x - p.x) * t : bound;
      c.y = axis ? bound : p.y + (q.y - p.y) * t;
      out[m++] = c;
    }
  }
  return m;
}

__device__ double shoelace_area(const P2 *p, int n) {
  double a = 0.;
  for (int i = 0; i < n; ++i) {
    const P2 u = p[i], w = p[i + 1 < n ? i + 1 : 0];
    a += u.x * w.y - w.x * u.y;
  }
  return 0.5 * fabs(a);
}

__device__ double cuboid_iou(const double *b, const double *a) {
  const double hx = b[3] / 2., hy = b[4] / 2., hz = b[5] / 2., ca = cos(b[6]), sa = sin(b[6]);
  const double v0x = hx * ca, v0y = hx * sa, v1x = -(hy * sa), v1y = hy * ca;
  P2 buf0[CLIP_CAP], buf1[CLIP_CAP];
  buf0[0].x = b[0] - v0x - v1x; buf0[0].y = b[1] - v0y - v1y;
  buf0[1].x = b[0] + v0x - v1x; buf0[1].y = b[1] + v0y - v1y;
  buf0[2].x = b[0] + v0x + v1x; buf0[2].y = b[1] + v0y + v1y;
  buf0[3].x = b[0] - v0x + v1x; buf0[3].y = b[1] - v0y + v1y;
  const double bz0 = b[2] - hz, bz1 = b[2] + hz;
  const double ax0 = a[0] - a[3] / 2., ax1 = a[0] + a[3] / 2., ay0 = a[1] - a[4] / 2., ay1 = a[1] + a[4] / 2.;
  const double az0 = a[2] - a[5] / 2., az1 = a[2] + a[5] / 2.;
  const double vol_b = shoelace_area(buf0, 4) * (bz1 - bz0);
  const double vol_a = (ax1 - ax0) * (ay1 - ay0) * (az1 - az0);
  int n = clip_half_plane(buf0, 4, buf1, 0, ax0, true);
  n = clip_half_plane(buf1, n, buf0, 0, ax1, false);
  n = clip_half_plane(buf0, n, buf1, 1, ay0, true);
  n = clip_half_plane(buf1, n, buf0, 1, ay1, false);
  const double area = n >= 3 ? shoelace_area(buf0, n) : 0.;
  const double h = fmax(0., fmin(bz1, az1) - fmax(bz0, az0));
  const double inter = area * h;
  return inter / (vol_b + vol_a - inter);
}

// one wave per CAD box
__global__ __launch_bounds__(64) void match_kernel(int I, const double *__restrict__ cad, const double *__restrict__ inst,
                                                   double *__restrict__ best_iou, int *__restrict__ best_id,
                                                   double *__restrict__ second_iou) {
  const int m = blockIdx.x, lane = threadIdx.x;
  double b[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) b[j] = cad[(size_t)m * 7 + j];
  double best = 0., second = 0.;
  int id = 0;
  for (int i = lane; i < I; i += 64) {                              // ascending: a strict > keeps the first of equals
    double a[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = inst[(size_t)i * 6 + j];
    const double iou = cuboid_iou(b, a);
    if (iou > best) {
      second = best;
      best = iou;
      id = i + 1;
    } else if (iou > second) {
      second = iou;
    }
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    const double ob = __shfl_xor(best, sh), os = __shfl_xor(second, sh);
    const int oi = __shfl_xor(id, sh);
    const bool take = ob > best || (ob == best && ob > 0. && oi < id);
    const double loser = take ? best : ob;
    if (take) {
      best = ob;
      id = oi;
    }
    second = fmax(fmax(second, os), loser);
  }
  if (lane == 0) {
    best_iou[m] = best;
    best_id[m] = id;
    second_iou[m] = second;
  }
}

// ---- rule P: votes ---------------------------------------------------------------------------------------------------
constexpr int VOTE_BOXES = 64;          // boxes staged per round

__global__ __launch_bounds__(THREADS) void point_votes_kernel(int N, int M, int stride, const float *__restrict__ v,
                                                              const double *__restrict__ boxes,
                                                              double *__restrict__ votes, int *__restrict__ hits) {
  __shared__ double s_box[VOTE_BOXES * 8];                          // centre, half sizes, cos, sin
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * THREADS + tid;
  const bool in = i < N;
  double px = 0., py = 0., pz = 0.;
  if (in) {
    const float *p = v + (size_t)i * stride;
    px = (double)p[0]; py = (double)p[1]; pz = (double)p[2];
  }
  double w1x = 0., w1y = 0., w1z = 0., w2x = 0., w2y = 0., w2z = 0., w3x = 0., w3y = 0., w3z = 0.;
  int h = 0;
  for (int m0 = 0; m0 < M; m0 += VOTE_BOXES) {
    const int nb = M - m0 < VOTE_BOXES ? M - m0 : VOTE_BOXES;
    __syncthreads();                                                // the last round's readers are done
    if (tid < nb) {
      const double *b = boxes + (size_t)(m0 + tid) * 7;
      double *s = s_box + tid * 8;
      s[0] = b[0]; s[1] = b[1]; s[2] = b[2];
      s[3] = fabs(0.5 * b[3]); s[4] = fabs(0.5 * b[4]); s[5] = fabs(0.5 * b[5]);
      s[6] = cos(b[6]); s[7] = sin(b[6]);
    }
    __syncthreads();
    if (in) {
      for (int k = 0; k < nb; ++k) {
        const double *s = s_box + k * 8;
        const double dx = px - s[0], dy = py - s[1], dz = pz - s[2];
        const double u = dx * s[6] + dy * s[7], w = -dx * s[7] + dy * s[6];
        if (fabs(u) <= s[3] && fabs(w) <= s[4] && fabs(dz) <= s[5]) {
          const double vx = s[0] - px, vy = s[1] - py, vz = s[2] - pz;
          if (h == 0) {
            w1x = w2x = w3x = vx; w1y = w2y = w3y = vy; w1z = w2z = w3z = vz;
          } else if (h == 1) {
            w2x = vx; w2y = vy; w2z = vz;
          } else {
            w3x = vx; w3y = vy; w3z = vz;
          }
          ++h;
        }
      }
    }
  }
  if (in) {
    double *o = votes + (size_t)i * 10;
    o[0] = h > 0 ? 1. : 0.;
    o[1] = w1x; o[2] = w1y; o[3] = w1z;
    o[4] = w2x; o[5] = w2y; o[6] = w2z;
    o[7] = w3x; o[8] = w3y; o[9] = w3z;
    hits[i] = h;
  }
}

// ---- rule S: sample --------------------------------------------------------------------------------------------------
struct SampleArgs {
  int P, N, stride, n_color, use_height, augment, flip_x, flip_y;
  double c, s, mean[3];
  float floor_height;
};

__global__ __launch_bounds__(THREADS) void sample_kernel(SampleArgs g, const float *__restrict__ v,
                                                         const double *__restrict__ votes,
                                                         const unsigned *__restrict__ ids,
                                                         const long long *__restrict__ choices,
                                                         float *__restrict__ points, float *__restrict__ vote_label,
                                                         long long *__restrict__ vote_mask,
                                                         float *__restrict__ instance) {
  const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (r >= g.P) return;
  const int C = 3 + g.n_color + (g.use_height ? 1 : 0);
  float *o = points + (size_t)r * C;
  float *ol = vote_label + (size_t)r * 9;
  const long long j = choices[r];
  if (j < 0 || j >= g.N) {
    for (int k = 0; k < C; ++k) o[k] = 0.f;
    for (int k = 0; k < 9; ++k) ol[k] = 0.f;
    vote_mask[r] = 0;
    instance[r] = 0.f;
    return;
  }
  const float *p = v + (size_t)j * g.stride;
  const double *w = votes + (size_t)j * 10;
  const float xf = p[0], yf = p[1], zf = p[2];
  for (int k = 0; k < g.n_color; ++k) o[3 + k] = (float)(((double)p[3 + k] - g.mean[k]) / 256.0);
  if (g.use_height) o[3 + g.n_color] = zf - g.floor_height;
  if (!g.augment) {
    o[0] = xf; o[1] = yf; o[2] = zf;
    for (int k = 0; k < 9; ++k) ol[k] = (float)w[1 + k];
  } else {
    const double fx = g.flip_x ? -1. : 1., fy = g.flip_y ? -1. : 1.;
    const double x = fx * (double)xf, y = fy * (double)yf, z = (double)zf;
    // rot(a): the product sum of a BLAS kernel that accumulates over k with fused multiply-adds (rule S)
    const float Px = (float)__builtin_fma(y, -g.s, g.c * x), Py = (float)__builtin_fma(y, g.c, g.s * x), Pz = zf;
    o[0] = Px; o[1] = Py; o[2] = Pz;
    for (int k = 0; k < 3; ++k) {
      const double ax = x + fx * w[1 + 3 * k], ay = y + fy * w[2 + 3 * k], az = z + w[3 + 3 * k];
      const double ex = __builtin_fma(ay, -g.s, g.c * ax), ey = __builtin_fma(ay, g.c, g.s * ax);
      ol[3 * k + 0] = (float)(ex - (double)Px);
      ol[3 * k + 1] = (float)(ey - (double)Py);
      ol[3 * k + 2] = (float)(az - (double)Pz);
    }
  }
  vote_mask[r] = (long long)w[0];
  instance[r] = (float)ids[j];
}

}  // namespace

RFD_API int rfd_labels_instance_aabb(int N, int I, int stride, const float *vertices, const unsigned *ids,
                                     unsigned *keys, float *box, void *stream) {
  if (N < 0 || I < 0 || stride < 3) return rfd_invalid("rfd_labels_instance_aabb: N, I >= 0, stride >= 3");
  if (I > INT_MAX / 6) return rfd_invalid("rfd_labels_instance_aabb: 6 I must stay below 2^31");
  if (I == 0) return 0;
  if (!keys || !box || (N > 0 && (!vertices || !ids))) return rfd_invalid("rfd_labels_instance_aabb: a null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const unsigned cells = (unsigned)ceil_div(I * 6, THREADS);
  aabb_init_kernel<<<cells, THREADS, 0, st>>>(I * 6, keys);
  RFD_CHECK_LAUNCH();
  if (N > 0) {
    const unsigned grid = (unsigned)(((long long)N + THREADS * AABB_PER_THREAD - 1) / (THREADS * AABB_PER_THREAD));
    instance_aabb_kernel<<<grid, THREADS, 0, st>>>(N, I, stride, vertices, ids, keys);
    RFD_CHECK_LAUNCH();
  }
  aabb_finish_kernel<<<cells, THREADS, 0, st>>>(I * 6, keys, box);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_labels_cad_extents(int M, int R, int step, const double *points, const int *off, const int *run_owner,
                                   const int *run_start, const double *L, unsigned long long *keys, double *ext,
                                   void *stream) {
  if (M < 0 || R < 0 || step < 1) return rfd_invalid("rfd_labels_cad_extents: M, R >= 0, step >= 1");
  if (M > INT_MAX / 12) return rfd_invalid("rfd_labels_cad_extents: 12 M must stay below 2^31");
  if (M == 0) return 0;
  if (!keys || !ext || !off || !L || (R > 0 && (!points || !run_owner || !run_start)))
    return rfd_invalid("rfd_labels_cad_extents: a null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const unsigned cells = (unsigned)ceil_div(M * 12, THREADS);
  extents_init_kernel<<<cells, THREADS, 0, st>>>(M * 12, keys);
  RFD_CHECK_LAUNCH();
  if (R > 0) {
    cad_extents_kernel<<<(unsigned)R, THREADS, 0, st>>>(M, step, points, off, run_owner, run_start, L, keys);
    RFD_CHECK_LAUNCH();
  }
  extents_finish_kernel<<<cells, THREADS, 0, st>>>(M * 12, keys, ext);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_labels_match_instances(int M, int I, const double *cad, const double *inst, double *best_iou,
                                       int *best_id, double *second_iou, void *stream) {
  if (M < 0 || I < 0) return rfd_invalid("rfd_labels_match_instances: M, I >= 0");
  if (M == 0) return 0;
  if (!cad || !best_iou || !best_id || !second_iou || (I > 0 && !inst))
    return rfd_invalid("rfd_labels_match_instances: a null pointer");
  match_kernel<<<(unsigned)M, 64, 0, (hipStream_t)stream>>>(I, cad, inst, best_iou, best_id, second_iou);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_labels_point_votes(int N, int M, int stride, const float *vertices, const double *boxes, double *votes,
                                   int *hits, void *stream) {
  if (N < 0 || M < 0 || stride < 3) return rfd_invalid("rfd_labels_point_votes: N, M >= 0, stride >= 3");
  if (N == 0) return 0;
  if (!vertices || !votes || !hits || (M > 0 && !boxes)) return rfd_invalid("rfd_labels_point_votes: a null pointer");
  const unsigned grid = (unsigned)(((long long)N + THREADS - 1) / THREADS);
  point_votes_kernel<<<grid, THREADS, 0, (hipStream_t)stream>>>(N, M, stride, vertices, boxes, votes, hits);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_labels_sample(int P, int N, int stride, int n_color, int use_height, int augment, int flip_x, int flip_y,
                              double c, double s, float floor_height, const double *mean, const float *vertices,
                              const double *votes, const unsigned *ids, const long long *choices, float *points,
                              float *vote_label, long long *vote_mask, float *instance, void *stream) {
  if (P < 0 || N < 0 || (n_color != 0 && n_color != 3) || stride < 3 + n_color)
    return rfd_invalid("rfd_labels_sample: P, N >= 0, n_color 0 or 3, stride >= 3 + n_color");
  if (P == 0) return 0;
  if (!choices || !points || !vote_label || !vote_mask || !instance || (n_color && !mean) ||
      (N > 0 && (!vertices || !votes || !ids)))
    return rfd_invalid("rfd_labels_sample: a null pointer");
  SampleArgs g;
  g.P = P; g.N = N; g.stride = stride; g.n_color = n_color; g.use_height = use_height; g.augment = augment;
  g.flip_x = flip_x; g.flip_y = flip_y; g.c = c; g.s = s; g.floor_height = floor_height;
  for (int k = 0; k < 3; ++k) g.mean[k] = n_color ? mean[k] : 0.;
  const unsigned grid = (unsigned)(((long long)P + THREADS - 1) / THREADS);
  sample_kernel<<<grid, THREADS, 0, (hipStream_t)stream>>>(g, vertices, votes, ids, choices, points, vote_label,
                                                         vote_mask, instance);
  RFD_CHECK_LAUNCH();
  return 0;
}
