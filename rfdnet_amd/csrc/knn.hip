// knn.hip -- exact k nearest neighbours among the points of a ragged batch of point sets and the per-segment sums of the
// point-cloud metrics (include/rfd_knn.h; rules N1 - N7 are spelled out there and restated in tests/knn_f64.py).  The
// library is built with -ffp-contract=off, so every expression below is evaluated as written; the f64 square root is the
// correctly rounded one.
//
// The query is one thread per point: the k best keys (squared distance, local row) are a sorted list of KMAX slots, KMAX a
// template parameter (1, 4, 8, 16, 32; the launcher takes the least one that holds k).  A candidate is tested against a
// copy of slot k - 1 first and only a winner runs the insertion, a compare-and-shift over all KMAX slots that is fully
// unrolled: no slot is ever named by a run-time subscript, so the list stays in registers (profiles/knn_codegen.txt: no
// scratch in any instance).  The host orders the queries by (object, cell) so that the lanes of a wave walk the same
// lists.  The cell lists are one CSR for the batch, built in two passes with integer atomics; the fill pass also writes
// the coordinates in list order, so that a cell's candidates are contiguous.  The sums are one wave per segment: lane j
// holds partial j, the tree runs through LDS.  No floating-point atomics, nothing waits for another workgroup, and every
// loop is bounded by the frame (at most R^3 cells), by a cell's list or by a segment.
#include <limits.h>
#include "common.h"
#include "../../include/rfd_knn.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_RES = 64;
constexpr int MAX_TAU = 8;
constexpr int MAX_K = 32;
constexpr int WAVE = 64;

// the three helpers below are mesh_dist.hip's own, copied: that file's results must not move with this one
__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// rule N2: clamp((int)floor((x - lo) * inv_h), 0, R - 1) without ever converting a value that an int cannot hold
__device__ __forceinline__ int cell_of(double x, double lo, double inv_h, int R) {
  const double t = (x - lo) * inv_h;
  if (!(t >= 0.)) return 0;
  if (t >= (double)R) return R - 1;
  return (int)t;
}

// the largest k with off[k] <= i, for 0 <= i < off[K]
__device__ __forceinline__ int segment_of(const int *__restrict__ off, int K, int i) {
  int a = 0, b = K - 1;
  while (a < b) {
    const int mid = a + (b - a + 1) / 2;
    if (off[mid] <= i) a = mid;
    else b = mid - 1;
  }
  return a;
}

__global__ __launch_bounds__(THREADS) void valid_kernel(int N, int K, const double *__restrict__ points,
                                                        const int *__restrict__ pend, unsigned char *__restrict__ valid,
                                                        int *__restrict__ pobj) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= N) return;
  const double *p = points + 3 * (size_t)i;
  valid[i] = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) ? 1 : 0;
  pobj[i] = segment_of(pend, K, i);
}

__global__ __launch_bounds__(THREADS) void point_cells_kernel(int N, int K, const double *__restrict__ points,
                                                              const unsigned char *__restrict__ valid,
                                                              const int *__restrict__ pobj, const double *__restrict__ lo,
                                                              const double *__restrict__ inv_h,
                                                              const int *__restrict__ res, const int *__restrict__ cbase,
                                                              int *__restrict__ cell) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= N) return;
  const int k = pobj[i];
  if (!valid[i] || k < 0 || k >= K) {
    cell[i] = -1;
    return;
  }
  const int R = min(max(res[k], 1), MAX_RES);
  const double *p = points + 3 * (size_t)i;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = cell_of(p[a], lo[3 * k + a], inv_h[3 * k + a], R);
  cell[i] = cbase[k] + (c[0] * R + c[1]) * R + c[2];
}

__global__ __launch_bounds__(THREADS) void cells_kernel(int N, const int *__restrict__ cell, int n_cells,
                                                        int *__restrict__ cursor, int *__restrict__ list, int M,
                                                        const double *__restrict__ points, double *__restrict__ sorted) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= N) return;
  const int c = cell[i];
  if (c < 0 || c >= n_cells) return;                    // not valid, or not a cell point_cells_kernel wrote
  const int slot = atomicAdd(cursor + c, 1);
  if (!list || slot < 0 || slot >= M) return;           // the counting pass; never outside the list
  list[slot] = i;
  if (sorted) {
#pragma unroll
    for (int a = 0; a < 3; ++a) sorted[3 * (size_t)slot + a] = points[3 * (size_t)i + a];
  }
}

// rule N5: key (a, i) < key (b, j)
__device__ __forceinline__ bool key_less(double a, int i, double b, int j) { return a < b || (a == b && i < j); }

// The k best keys of one query, ascending, in KMAX slots of which the first k count; `wd`, `wi` copy slot k - 1.  Every
// loop over the slots is unrolled with a compile-time subscript.
template <int KMAX>
struct Best {
  double d[KMAX];
  int i[KMAX];
  double wd;
  int wi;

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) d[j] = __builtin_inf(), i[j] = -1;
    wd = __builtin_inf(), wi = -1;
  }

  // (dd, row) is known to be less than slot k - 1: slot j takes the old slot j - 1 where the candidate goes before that
  // one, else the candidate where it goes before the old slot j, else stays.  From the top down, so every slot read is
  // still the old one.  What is pushed past slot k - 1 is never read again.
  __device__ __forceinline__ void insert(double dd, int row, int k) {
#pragma unroll
    for (int j = KMAX - 1; j >= 1; --j) {
      const bool before_prev = key_less(dd, row, d[j - 1], i[j - 1]);
      const bool before_this = key_less(dd, row, d[j], i[j]);
      d[j] = before_prev ? d[j - 1] : (before_this ? dd : d[j]);
      i[j] = before_prev ? i[j - 1] : (before_this ? row : i[j]);
    }
    if (key_less(dd, row, d[0], i[0])) d[0] = dd, i[0] = row;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j == k - 1) wd = d[j], wi = i[j];
  }
};

template <int KMAX>
__global__ __launch_bounds__(THREADS) void query_kernel(
    int n, const double *__restrict__ queries, const int *__restrict__ qobj, int k, double limit2,
    const unsigned char *__restrict__ mask, int K, int N, const double *__restrict__ points,
    const int *__restrict__ pend, const double *__restrict__ lo, const double *__restrict__ hi,
    const double *__restrict__ inv_h, const double *__restrict__ hh, const double *__restrict__ slack,
    const int *__restrict__ res, const int *__restrict__ cbase, const int *__restrict__ offsets,
    const int *__restrict__ list, int M, const double *__restrict__ sorted, double *__restrict__ d2out,
    int *__restrict__ idxout) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]};
  const int ko = qobj[i];
  Best<KMAX> best;
  best.clear();
  const bool answered = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && ko >= 0 && ko < K;
  if (answered) {
    const int R = min(max(res[ko], 1), MAX_RES), base = cbase[ko];
    const int p0 = max(pend[ko], 0), p1 = min(pend[ko + 1], N);          // never outside the N rows
    const double sl = slack[ko];
    double pp[3], l[3], h[3];
    int c[3], Ra[3];
    double out2;
    {
      double o[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        l[a] = lo[3 * ko + a], h[a] = hh[3 * ko + a];
        const double ih = inv_h[3 * ko + a];
        pp[a] = fmin(fmax(p[a], l[a]), hi[3 * ko + a]);
        c[a] = cell_of(pp[a], l[a], ih, R);
        Ra[a] = ih == 0. ? 1 : R;
        if (c[a] > Ra[a] - 1) c[a] = Ra[a] - 1;
        o[a] = fmax(fabs(p[a] - pp[a]) - sl, 0.);
      }
      out2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
    }
    for (int r = 0; r < R; ++r) {
      const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, Ra[0] - 1);
      const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, Ra[1] - 1);
      const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, Ra[2] - 1);
      for (int x = x0; x <= x1; ++x) {
        const bool xr = x - c[0] == r || c[0] - x == r;
        for (int y = y0; y <= y1; ++y) {
          const int row0 = base + (x * R + y) * R;
          // on the shell's x or y faces every z of the range; inside, its two z faces only (r >= 1 there)
          const bool full = xr || y - c[1] == r || c[1] - y == r;
          const int zs = full ? z0 : (c[2] - r >= 0 ? c[2] - r : c[2] + r), step = full ? 1 : 2 * r;
          for (int z = zs; z <= z1; z += step) {
            const int s0 = max(offsets[row0 + z], 0), s1 = min(offsets[row0 + z + 1], M);      // never outside the list
            for (int s = s0; s < s1; ++s) {
              const int row = list[s];
              if (row < p0 || row >= p1) continue;                       // a row outside its set is skipped
              if (mask && mask[row]) continue;
              const double *t = sorted ? sorted + 3 * (size_t)s : points + 3 * (size_t)row;
              const double rx = p[0] - t[0], ry = p[1] - t[1], rz = p[2] - t[2];
              const double dd = (rx * rx + ry * ry) + rz * rz;
              const int local = row - p0;
              if (dd < limit2 && key_less(dd, local, best.wd, best.wi)) best.insert(dd, local, k);
            }
          }
        }
      }
      double g = __builtin_inf();
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (c[a] - r - 1 >= 0) g = fmin(g, pp[a] - (l[a] + (double)(c[a] - r) * h[a]));
        if (c[a] + r + 1 <= Ra[a] - 1) g = fmin(g, (l[a] + (double)(c[a] + r + 1) * h[a]) - pp[a]);
      }
      if (g == __builtin_inf()) break;                                   // no side has cells left
      g = fmax(g - sl, 0.);
      const double bound = (out2 + g * g) * (1. - 0x1p-40);
      if (fmin(best.wd, limit2) < bound) break;
    }
  }
  double *dout = d2out + (size_t)i * k;
  int *iout = idxout + (size_t)i * k;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {
      dout[j] = answered ? best.d[j] : __builtin_nan("");
      iout[j] = answered ? best.i[j] : -1;
    }
  }
}

__global__ __launch_bounds__(WAVE) void sums_kernel(int S, int n, int stride, const int *__restrict__ seg,
                                                    const double *__restrict__ d2, const int *__restrict__ row,
                                                    const int *__restrict__ qobj, int K, int N,
                                                    const int *__restrict__ pend, const double *__restrict__ n_s,
                                                    const double *__restrict__ n_t, int T, const double *__restrict__ tau,
                                                    double *__restrict__ sums, int *__restrict__ counts) {
  __shared__ double part[3][WAVE];
  __shared__ int cnt[1 + MAX_TAU][WAVE];
  const int s = blockIdx.x, j = threadIdx.x;
  const int e0 = min(max(seg[s], 0), n), e1 = min(max(seg[s + 1], e0), n);      // never outside the n entries
  const bool normals = n_s && n_t;
  double th[MAX_TAU];
  int within[MAX_TAU];
#pragma unroll
  for (int t = 0; t < MAX_TAU; ++t) th[t] = t < T ? tau[t] : 0., within[t] = 0;
  double sd = 0., sd2 = 0., sn = 0.;
  int left_out = 0;
  for (int e = e0 + j; e < e1; e += WAVE) {
    const double v = d2[(size_t)e * stride];
    const double d = sqrt(v);
    const int local = row[(size_t)e * stride], ko = qobj[e];
    int target = -1;
    if (ko >= 0 && ko < K && local >= 0) {
      const int p0 = max(pend[ko], 0), p1 = min(pend[ko + 1], N);
      if (local < p1 - p0) target = p0 + local;                          // never outside the N rows
    }
    if (!isfinite(d) || target < 0) {
      ++left_out;
      continue;
    }
    sd += d, sd2 += v;
    if (normals) {
      const double *a = n_s + 3 * (size_t)e, *b = n_t + 3 * (size_t)target;
      sn += fabs(dot3(a[0], a[1], a[2], b[0], b[1], b[2]));
    }
#pragma unroll
    for (int t = 0; t < MAX_TAU; ++t)
      if (t < T && d <= th[t]) ++within[t];
  }
  part[0][j] = sd, part[1][j] = sd2, part[2][j] = sn;
  cnt[0][j] = left_out;
#pragma unroll
  for (int t = 0; t < MAX_TAU; ++t) cnt[1 + t][j] = within[t];
  __syncthreads();
  for (int w = WAVE / 2; w >= 1; w /= 2) {
    if (j < w) {
#pragma unroll
      for (int q = 0; q < 3; ++q) part[q][j] += part[q][j + w];
#pragma unroll
      for (int q = 0; q < 1 + MAX_TAU; ++q) cnt[q][j] += cnt[q][j + w];
    }
    __syncthreads();
  }
  if (j < 3) sums[3 * (size_t)s + j] = part[j][0];
  if (j < 1 + T) counts[(size_t)(1 + T) * s + j] = cnt[j][0];
}

}  // namespace

RFD_API int rfd_knn_points(int N, int K, const double *points, const int *pend, const double *lo, const double *inv_h,
                           const int *res, const int *cbase, unsigned char *valid, int *pobj, int *cell, void *stream) {
  if (N < 0 || K < 0) return rfd_invalid("rfd_knn_points: N, K >= 0");
  if (N > INT_MAX / 3) return rfd_invalid("rfd_knn_points: 3 N must stay below 2^31");
  if (N == 0) return 0;
  if (K < 1) return rfd_invalid("rfd_knn_points: points without a set");
  if (!points || !pend || !valid || !pobj) return rfd_invalid("rfd_knn_points: a null pointer");
  const unsigned blocks = (unsigned)ceil_div(N, THREADS);
  if (!lo) {
    valid_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(N, K, points, pend, valid, pobj);
  } else {
    if (!inv_h || !res || !cbase || !cell) return rfd_invalid("rfd_knn_points: a null pointer");
    point_cells_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(N, K, points, valid, pobj, lo, inv_h, res, cbase,
                                                                    cell);
  }
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_knn_cells(int N, const int *cell, int n_cells, int *cursor, int *list, int M, const double *points,
                          double *sorted, void *stream) {
  if (N < 0 || n_cells < 0 || M < 0) return rfd_invalid("rfd_knn_cells: N, n_cells, M >= 0");
  if (N > INT_MAX / 3) return rfd_invalid("rfd_knn_cells: 3 N must stay below 2^31");
  if (N == 0) return 0;
  if (!cell || !cursor || (sorted && (!list || !points))) return rfd_invalid("rfd_knn_cells: a null pointer");
  cells_kernel<<<(unsigned)ceil_div(N, THREADS), THREADS, 0, (hipStream_t)stream>>>(N, cell, n_cells, cursor, list, M,
                                                                                    points, sorted);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_knn_query(int n, const double *queries, const int *qobj, int k, double limit2,
                          const unsigned char *mask, int K, int N, const double *points, const int *pend,
                          const double *lo, const double *hi, const double *inv_h, const double *h, const double *slack,
                          const int *res, const int *cbase, const int *offsets, const int *list, int M,
                          const double *sorted, double *d2, int *idx, void *stream) {
  if (n < 0 || K < 0 || N < 0 || M < 0) return rfd_invalid("rfd_knn_query: n, K, N, M >= 0");
  if (k < 1 || k > MAX_K) return rfd_invalid("rfd_knn_query: 1 <= k <= 32");
  if (n > INT_MAX / 3 || n > INT_MAX / k) return rfd_invalid("rfd_knn_query: 3 n and n k must stay below 2^31");
  if (limit2 != limit2) return rfd_invalid("rfd_knn_query: limit2 is a NaN");
  if (n == 0) return 0;
  if (!queries || !qobj || !d2 || !idx ||
      (K > 0 && (!pend || !lo || !hi || !inv_h || !h || !slack || !res || !cbase || !offsets)) ||
      (M > 0 && (!list || (!points && !sorted))))
    return rfd_invalid("rfd_knn_query: a null pointer");
  const unsigned blocks = (unsigned)ceil_div(n, THREADS);
#define RFD_KNN_LAUNCH(KMAX)                                                                                          \
  query_kernel<KMAX><<<blocks, THREADS, 0, (hipStream_t)stream>>>(n, queries, qobj, k, limit2, mask, K, N, points, pend, \
                                                                   lo, hi, inv_h, h, slack, res, cbase, offsets, list, M, \
                                                                   sorted, d2, idx)
  if (k <= 1) RFD_KNN_LAUNCH(1);
  else if (k <= 4) RFD_KNN_LAUNCH(4);
  else if (k <= 8) RFD_KNN_LAUNCH(8);
  else if (k <= 16) RFD_KNN_LAUNCH(16);
  else RFD_KNN_LAUNCH(32);
#undef RFD_KNN_LAUNCH
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_knn_sums(int S, int n, int stride, const int *seg, const double *d2, const int *row, const int *qobj,
                         int K, int N, const int *pend, const double *n_s, const double *n_t, int T, const double *tau,
                         double *sums, int *counts, void *stream) {
  if (S < 0 || n < 0 || K < 0 || N < 0 || T < 0 || T > MAX_TAU || stride < 1)
    return rfd_invalid("rfd_knn_sums: S, n, K, N >= 0, 0 <= T <= 8, stride >= 1");
  if (n > INT_MAX / 3 || n > INT_MAX / stride) return rfd_invalid("rfd_knn_sums: 3 n and n stride must stay below 2^31");
  if (S == 0) return 0;
  if (!seg || !sums || !counts || (T > 0 && !tau) || (n > 0 && (!d2 || !row || !qobj)) || (K > 0 && !pend))
    return rfd_invalid("rfd_knn_sums: a null pointer");
  sums_kernel<<<(unsigned)S, WAVE, 0, (hipStream_t)stream>>>(S, n, stride, seg, d2, row, qobj, K, N, pend, n_s, n_t, T, tau,
                                                             sums, counts);
  RFD_CHECK_LAUNCH();
  return 0;
}
