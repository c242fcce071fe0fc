// objgrid.hip -- the voxel grids of ALL objects of a scene in one ragged batch (include/rfd_objgrid.h; rules B1 - B7 in
// include/rfd_mesh_eval.h):
// surface words, bin lists, interior words, union and counts.  Four kernels, each launched once per scene whatever the
// number of objects; every object has its own dimension D <= 256 and its own words at its own offset.  The library is
// built with -ffp-contract=off, so every expression below is evaluated as written.
//
// The interior kernel is one WAVE per column (i, j) of an object, and it uses its 64 lanes twice over:
//   - along the column's triangle list: lane l takes triangle base + l and runs C2 / C4 / C5 for (px', py') once, so the
//     2-D test costs ceil(list / 64) rounds per column and no lane repeats another's arithmetic;
//   - along z: for every hit (the ballot of the round, walked bit by bit; depth and |n2| are broadcast from the lane that
//     found it) lane l compares the lattice points z = 64 w + l, w < W, and keeps the two parities of each in two 4-bit
//     registers.  The ballot of (P0 & P1) over the wave IS the 64-bit word of I: whole words are stored, no atomics.
// One thread per column with the parities in 2 x 4 u64 registers would do the same arithmetic, but with the small
// triangles of a reconstructed mesh (a triangle covers less than a column) every lane of a wave hits in a different
// round, and the D compares of one lane would run with the other 63 idle.  Only parities are read, so the order in which
// a column meets its triangles -- the order the integer atomics of the fill pass left -- changes nothing.
//
// The table rows and face_obj are checked by every kernel that reads them: a row outside 2 <= D <= 256 or whose words
// do not lie inside [0, n_words) is an object without a grid, a face of no such object is skipped.  No floating-point
// atomics, nothing waits for another workgroup, every loop is bounded.
#include "common.h"
#include "../../include/rfd_objgrid.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TRI_PER_BLOCK = 64;
constexpr int SLABS = 8;                   // workgroups that share one triangle's box of voxels
constexpr int MAX_D = 256;
constexpr int MAX_OBJECTS = 65535;         // gridDim.y
constexpr int HASH_RES = 512;              // rule B3: C1 at res = 512
constexpr int BIN_SHIFT = 4, BINS = HASH_RES >> BIN_SHIFT;      // 32 x 32 bins of 16 x 16 cells per object
constexpr int FINISH_BLOCKS = 64;
constexpr int INTERIOR_MAX_BLOCKS = 4096;

// (int)x clamped to [0, last] (rule C3 / V2), without ever converting a value that an int cannot hold
template <typename T>
__device__ __forceinline__ int cell_of(T x, int last) {
  if (!(x >= (T)0)) return 0;
  if (x >= (T)(last + 1)) return last;
  return (int)x;
}

// -> D of table row `obj` and its word offset, or 0: no grid (the row is out of range in some way)
__device__ __forceinline__ int load_row(int obj, int N, const int *dim, const long long *off, long long n_words,
                                        long long &at) {
  if (obj < 0 || obj >= N) return 0;
  const int D = dim[obj];
  if (D < 2 || D > MAX_D) return 0;
  at = off[obj];
  const long long need = (long long)D * D * ((D + 63) >> 6);
  if (at < 0 || at > n_words - need) return 0;
  return D;
}

// ---- rule V3.  A copy of mesh_sample.hip's separated / apart / tri_box_overlap (the original; keep the two alike):
// sharing them through a header is allowed only if mesh_sample.hip's generated code stays what it was.
__device__ __forceinline__ bool separated(float pa, float pb, float fa, float fb) {
  float mn, mx;
  if (pa < pb) mn = pa, mx = pb;
  else mn = pb, mx = pa;
  const float rad = fa * 0.5f + fb * 0.5f;
  return mn > rad || mx < -rad;
}

__device__ __forceinline__ bool apart(float a, float b, float c) {
  float mn = a, mx = a;
  if (b < mn) mn = b;
  if (b > mx) mx = b;
  if (c < mn) mn = c;
  if (c > mx) mx = c;
  return mn > 0.5f || mx < -0.5f;
}

__device__ __forceinline__ bool tri_box_overlap(const float *t, float cx, float cy, float cz) {
  const float v0x = t[0] - cx, v0y = t[1] - cy, v0z = t[2] - cz;
  const float v1x = t[3] - cx, v1y = t[4] - cy, v1z = t[5] - cz;
  const float v2x = t[6] - cx, v2y = t[7] - cy, v2z = t[8] - cz;
  const float e0x = v1x - v0x, e0y = v1y - v0y, e0z = v1z - v0z;
  const float e1x = v2x - v1x, e1y = v2y - v1y, e1z = v2z - v1z;
  const float e2x = v0x - v2x, e2y = v0y - v2y, e2z = v0z - v2z;
  float fex = fabsf(e0x), fey = fabsf(e0y), fez = fabsf(e0z);
  if (separated(e0z * v0y - e0y * v0z, e0z * v2y - e0y * v2z, fez, fey)) return false;      // X01
  if (separated(-e0z * v0x + e0x * v0z, -e0z * v2x + e0x * v2z, fez, fex)) return false;    // Y02
  if (separated(e0y * v1x - e0x * v1y, e0y * v2x - e0x * v2y, fey, fex)) return false;      // Z12
  fex = fabsf(e1x), fey = fabsf(e1y), fez = fabsf(e1z);
  if (separated(e1z * v0y - e1y * v0z, e1z * v2y - e1y * v2z, fez, fey)) return false;      // X01
  if (separated(-e1z * v0x + e1x * v0z, -e1z * v2x + e1x * v2z, fez, fex)) return false;    // Y02
  if (separated(e1y * v0x - e1x * v0y, e1y * v1x - e1x * v1y, fey, fex)) return false;      // Z0
  fex = fabsf(e2x), fey = fabsf(e2y), fez = fabsf(e2z);
  if (separated(e2z * v0y - e2y * v0z, e2z * v1y - e2y * v1z, fez, fey)) return false;      // X2
  if (separated(-e2z * v0x + e2x * v0z, -e2z * v1x + e2x * v1z, fez, fex)) return false;    // Y1
  if (separated(e2y * v1x - e2x * v1y, e2y * v2x - e2x * v2y, fey, fex)) return false;      // Z12
  if (apart(v0x, v1x, v2x) || apart(v0y, v1y, v2y) || apart(v0z, v1z, v2z)) return false;
  const float n0 = e0y * e1z - e0z * e1y, n1 = e0z * e1x - e0x * e1z, n2 = e0x * e1y - e0y * e1x;
  const float d = -((n0 * v0x + n1 * v0y) + n2 * v0z);
  const float m0 = n0 > 0.f ? -0.5f : 0.5f, m1 = n1 > 0.f ? -0.5f : 0.5f, m2 = n2 > 0.f ? -0.5f : 0.5f;
  if (((n0 * m0 + n1 * m1) + n2 * m2) + d > 0.f) return false;
  return ((n0 * -m0 + n1 * -m1) + n2 * -m2) + d >= 0.f;
}

// Rule B2.  mesh_sample.hip's voxelize_kernel with R and the words looked up per triangle: 64 triangles staged in LDS,
// the box of one triangle dealt over the workgroup and over gridDim.y; a set voxel is one integer atomicOr.
__global__ __launch_bounds__(THREADS) void surface_kernel(int F, const float *__restrict__ tri,
                                                          const int *__restrict__ face_obj, int N,
                                                          const int *__restrict__ dim, const long long *__restrict__ off,
                                                          long long n_words, unsigned long long *__restrict__ words) {
  __shared__ float stri[TRI_PER_BLOCK][9];
  __shared__ int sbox[TRI_PER_BLOCK][6];
  __shared__ int sdim[TRI_PER_BLOCK];
  __shared__ long long soff[TRI_PER_BLOCK];
  const int f0 = blockIdx.x * TRI_PER_BLOCK;
  const int nt = min(TRI_PER_BLOCK, F - f0);
  for (int k = threadIdx.x; k < nt * 9; k += THREADS) (&stri[0][0])[k] = tri[9 * (size_t)f0 + k];
  if ((int)threadIdx.x < nt) {
    long long at = 0;
    sdim[threadIdx.x] = load_row(face_obj[f0 + threadIdx.x], N, dim, off, n_words, at);
    soff[threadIdx.x] = at;
  }
  __syncthreads();
  if ((int)threadIdx.x < nt * 3) {      // rule V2, one axis of one triangle
    const int t = threadIdx.x / 3, a = threadIdx.x % 3;
    const int R = max(sdim[t], 1);
    const float p = stri[t][a], q = stri[t][3 + a], r = stri[t][6 + a];
    float mn = p, mx = p;
    if (q < mn) mn = q;
    if (r < mn) mn = r;
    if (q > mx) mx = q;
    if (r > mx) mx = r;
    sbox[t][2 * a] = cell_of(mn, R - 1), sbox[t][2 * a + 1] = cell_of(mx, R - 1);
  }
  __syncthreads();
  const int first = blockIdx.y * THREADS + threadIdx.x, step = gridDim.y * THREADS;
  for (int t = 0; t < nt; ++t) {
    const int D = sdim[t];
    if (D == 0) continue;                                               // no grid: the triangle is not looked at
    const int W = (D + 63) >> 6;
    unsigned long long *w = words + soff[t];
    const int i0 = sbox[t][0], j0 = sbox[t][2], k0 = sbox[t][4];
    const int nj = sbox[t][3] - j0 + 1, nk = sbox[t][5] - k0 + 1;
    const int n = (sbox[t][1] - i0 + 1) * nj * nk;                      // <= 256^3 < 2^31
    for (int c = first; c < n; c += step) {
      const int i = i0 + c / (nj * nk), j = j0 + (c / nk) % nj, k = k0 + c % nk;      // all in [0, D)
      if (tri_box_overlap(stri[t], (float)(i + 0.5), (float)(j + 0.5), (float)(k + 0.5)))
        atomicOr(w + ((size_t)i * D + j) * W + (k >> 6), 1ull << (k & 63));
    }
  }
}

// the constants of object `obj` (rule B3) -> false: no interior (no grid, or a scale that is not positive)
__device__ __forceinline__ bool load_constants(int obj, const double *consts, double *s, double *t) {
#pragma unroll
  for (int a = 0; a < 3; ++a) s[a] = consts[6 * (size_t)obj + a], t[a] = consts[6 * (size_t)obj + 3 + a];
  return s[0] > 0. && s[1] > 0. && s[2] > 0.;
}

// Rule B6, both passes (list == NULL: count).  One thread per triangle rescales x and y (C2), takes the C3 cell box and
// shifts it to bins; then all threads of the workgroup work through one triangle's bins at a time (at most 32 x 32).
__global__ __launch_bounds__(THREADS) void bins_kernel(int F, const double *__restrict__ tri,
                                                       const int *__restrict__ face_obj, int N,
                                                       const int *__restrict__ dim, const double *__restrict__ consts,
                                                       int *__restrict__ cursor, int *__restrict__ list, int n_pairs) {
  __shared__ int sbox[TRI_PER_BLOCK][5];
  const int f0 = blockIdx.x * TRI_PER_BLOCK;
  const int nt = min(TRI_PER_BLOCK, F - f0);
  if ((int)threadIdx.x < nt) {
    const int f = f0 + threadIdx.x, obj = face_obj[f];
    int *b = sbox[threadIdx.x];
    b[4] = -1;
    double s[3], t[3];
    if (obj >= 0 && obj < N && dim[obj] >= 2 && dim[obj] <= MAX_D && load_constants(obj, consts, s, t)) {
      const double *p = tri + 9 * (size_t)f;
      double x[3], y[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = s[0] * p[3 * c] + t[0], y[c] = s[1] * p[3 * c + 1] + t[1];
      const double x0 = fmin(fmin(x[0], x[1]), x[2]), x1 = fmax(fmax(x[0], x[1]), x[2]);
      const double y0 = fmin(fmin(y[0], y[1]), y[2]), y1 = fmax(fmax(y[0], y[1]), y[2]);
      b[0] = cell_of(x0, HASH_RES - 1) >> BIN_SHIFT, b[1] = cell_of(x1, HASH_RES - 1) >> BIN_SHIFT;
      b[2] = cell_of(y0, HASH_RES - 1) >> BIN_SHIFT, b[3] = cell_of(y1, HASH_RES - 1) >> BIN_SHIFT;
      b[4] = obj;
    }
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int obj = sbox[t][4];
    if (obj < 0) continue;
    const int x0 = sbox[t][0], y0 = sbox[t][2];
    const int ny = sbox[t][3] - y0 + 1;
    const int n = (sbox[t][1] - x0 + 1) * ny;                            // <= 1024
    for (int c = threadIdx.x; c < n; c += THREADS) {
      const int bin = (obj * BINS + x0 + c / ny) * BINS + (y0 + c % ny);
      const int slot = atomicAdd(cursor + bin, 1);
      if (list && slot >= 0 && slot < n_pairs) list[slot] = f0 + t;
    }
  }
}

// Rules B4 - B5: blockIdx.y is the object, a wave takes columns blockIdx.x * WAVES + wave, + gridDim.x * WAVES, ...
__global__ __launch_bounds__(THREADS) void interior_kernel(int F, const double *__restrict__ tri, int N,
                                                           const int *__restrict__ dim,
                                                           const long long *__restrict__ off, long long n_words,
                                                           const double *__restrict__ consts,
                                                           const int *__restrict__ offsets,
                                                           const int *__restrict__ list, int n_pairs,
                                                           unsigned long long *__restrict__ inter) {
  const int obj = blockIdx.y;
  long long at = 0;
  const int D = load_row(obj, N, dim, off, n_words, at);
  double s[3], t[3];
  if (D == 0 || !load_constants(obj, consts, s, t)) return;             // uniform over the workgroup
  const int W = (D + 63) >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double r = (double)HASH_RES, dD = (double)D;
  double pz[4];
  bool cz[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {                                          // rule B4 along z: this lane's lattice points
    const int z = 64 * w + lane;
    pz[w] = s[2] * (((double)z + 0.5) / dD - 0.5) + t[2];
    cz[w] = z < D && pz[w] >= 0. && pz[w] <= r;
  }
  for (int col = blockIdx.x * WAVES + wave; col < D * D; col += gridDim.x * WAVES) {
    const int i = col / D, j = col - i * D;
    const double px = s[0] * (((double)i + 0.5) / dD - 0.5) + t[0];
    const double py = s[1] * (((double)j + 0.5) / dD - 0.5) + t[1];
    if (!(px >= 0. && px < r && py >= 0. && py < r)) continue;          // no candidate: its words stay zero
    const int bin = (obj * BINS + ((int)px >> BIN_SHIFT)) * BINS + ((int)py >> BIN_SHIFT);
    const int begin = offsets[bin], end = offsets[bin + 1];
    unsigned p0 = 0, p1 = 0;                                             // bit w: the parities of z = 64 w + lane
    if (begin >= 0 && end <= n_pairs) {
      for (int base = begin; base < end; base += 64) {
        bool hit = false;
        double depth = 0., an = 0.;
        const int k = base + lane;
        const int f = k < end ? list[k] : -1;
        if (f >= 0 && f < F) {
          const double *p = tri + 9 * (size_t)f;
          const double t1x = s[0] * p[0] + t[0], t1y = s[1] * p[1] + t[1];                      // C2
          const double t2x = s[0] * p[3] + t[0], t2y = s[1] * p[4] + t[1];
          const double t3x = s[0] * p[6] + t[0], t3y = s[1] * p[7] + t[1];
          const double A00 = t1x - t3x, A10 = t1y - t3y, A01 = t2x - t3x, A11 = t2y - t3y;      // C4
          const double det = A00 * A11 - A01 * A10;
          if (det != 0.) {
            const double sg = det > 0. ? 1. : -1., ad = fabs(det);
            const double y0 = px - t3x, y1 = py - t3y;
            const double u = (A11 * y0 - A01 * y1) * sg;
            const double v = (-A10 * y0 + A00 * y1) * sg;
            const double w = u + v;
            if (0. < u && u < ad && 0. < v && v < ad && 0. < w && w < ad) {
              const double t1z = s[2] * p[2] + t[2], t2z = s[2] * p[5] + t[2], t3z = s[2] * p[8] + t[2];
              const double v1x = t3x - t1x, v1y = t3y - t1y, v1z = t3z - t1z;                   // C5
              const double v2x = t2x - t1x, v2y = t2y - t1y, v2z = t2z - t1z;
              const double nn0 = v1y * v2z - v1z * v2y, nn1 = v1z * v2x - v1x * v2z, nn2 = v1x * v2y - v1y * v2x;
              if (nn2 != 0.) {
                const double alpha = nn0 * (t1x - px) + nn1 * (t1y - py);
                an = fabs(nn2);
                depth = t1z * an + alpha * (nn2 > 0. ? 1. : -1.);
                hit = true;
              }
            }
          }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {                                                   // uniform over the wave
          const int src = __ffsll((long long)hits) - 1;
          hits &= hits - 1;
          const double d = __shfl(depth, src, 64), a = __shfl(an, src, 64);
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            if (cz[w]) {
              const double rhs = pz[w] * a;
              if (d >= rhs) p0 ^= 1u << w;
              else if (d < rhs) p1 ^= 1u << w;
            }
          }
        }
      }
    }
    const unsigned both = p0 & p1;
    for (int w = 0; w < W; ++w) {
      const unsigned long long word = __ballot((both >> w) & 1u);
      if (lane == 0) inter[at + (size_t)col * W + w] = word;
    }
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                            // lane 0 holds the sum
}

// Rule B7: blockIdx.y is the object, its words are dealt over gridDim.x workgroups
__global__ __launch_bounds__(THREADS) void finish_kernel(int N, const int *__restrict__ dim,
                                                         const long long *__restrict__ off, long long n_words,
                                                         unsigned long long *__restrict__ words,
                                                         const unsigned long long *__restrict__ inter,
                                                         int *__restrict__ cnt) {
  __shared__ int s_u[WAVES], s_s[WAVES];
  const int obj = blockIdx.y;
  long long at = 0;
  const int D = load_row(obj, N, dim, off, n_words, at);
  if (D == 0) return;                                                    // uniform over the workgroup
  const int total = D * D * ((D + 63) >> 6);                             // <= 2^18
  int nU = 0, nS = 0;
  for (int w = blockIdx.x * THREADS + threadIdx.x; w < total; w += gridDim.x * THREADS) {
    const unsigned long long sw = words[at + w], uw = sw | inter[at + w];
    words[at + w] = uw;
    nU += __popcll(uw);
    nS += __popcll(sw);
  }
  nU = wave_sum(nU), nS = wave_sum(nS);
  if ((threadIdx.x & 63) == 0) s_u[threadIdx.x >> 6] = nU, s_s[threadIdx.x >> 6] = nS;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) a += s_u[i], b += s_s[i];
    if (a) atomicAdd(cnt + 2 * (size_t)obj, a);
    if (b) atomicAdd(cnt + 2 * (size_t)obj + 1, b);
  }
}

// the host's copy of the table: -> NULL, or what is wrong with it.  max_dim: the largest D.
const char *check_table(int N, const int *dim_host, const long long *off_host, long long n_words, int *max_dim) {
  if (N < 0 || N > MAX_OBJECTS || n_words < 0) return "need 0 <= N <= 65535 and n_words >= 0";
  if (N > 0 && (!dim_host || !off_host)) return "a null pointer";
  *max_dim = 0;
  for (int k = 0; k < N; ++k) {
    const int D = dim_host[k];
    if (D == 0) continue;
    if (D < 2 || D > MAX_D) return "a dim outside {0} and [2, 256]";
    const long long need = (long long)D * D * ((D + 63) / 64);
    if (off_host[k] < 0 || off_host[k] > n_words - need) return "an object's words do not lie inside the buffer";
    if (D > *max_dim) *max_dim = D;
  }
  return nullptr;
}

int refuse(const char *fn, const char *what) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, what);
  return rfd_invalid(msg);                             // the message is copied
}

}  // namespace

RFD_API int rfd_objgrid_surface(int F, const float *tri, const int *face_obj, int N, const int *dim_host,
                                const long long *off_host, const int *dim, const long long *off, long long n_words,
                                unsigned long long *words, void *stream) {
  int max_dim;
  if (F < 0) return refuse("rfd_objgrid_surface", "F >= 0");
  if (const char *bad = check_table(N, dim_host, off_host, n_words, &max_dim)) return refuse("rfd_objgrid_surface", bad);
  if (F == 0 || N == 0 || max_dim == 0) return 0;
  if (!tri || !face_obj || !dim || !off || !words) return refuse("rfd_objgrid_surface", "a null pointer");
  surface_kernel<<<dim3((unsigned)ceil_div(F, TRI_PER_BLOCK), SLABS), THREADS, 0, (hipStream_t)stream>>>(
      F, tri, face_obj, N, dim, off, n_words, words);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_objgrid_bins(int F, const double *tri, const int *face_obj, int N, const int *dim_host,
                             const int *dim, const double *consts, int *cursor, int *list, int n_pairs,
                             void *stream) {
  if (F < 0 || n_pairs < 0) return refuse("rfd_objgrid_bins", "F, n_pairs >= 0");
  if (N < 0 || N > MAX_OBJECTS) return refuse("rfd_objgrid_bins", "need 0 <= N <= 65535");
  if (N > 0 && !dim_host) return refuse("rfd_objgrid_bins", "a null pointer");
  bool any = false;
  for (int k = 0; k < N; ++k) {
    if (dim_host[k] != 0 && (dim_host[k] < 2 || dim_host[k] > MAX_D))
      return refuse("rfd_objgrid_bins", "a dim outside {0} and [2, 256]");
    any = any || dim_host[k] != 0;
  }
  if (F == 0 || !any) return 0;
  if (!tri || !face_obj || !dim || !consts || !cursor) return refuse("rfd_objgrid_bins", "a null pointer");
  bins_kernel<<<(unsigned)ceil_div(F, TRI_PER_BLOCK), THREADS, 0, (hipStream_t)stream>>>(F, tri, face_obj, N, dim, consts,
                                                                                        cursor, list, n_pairs);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_objgrid_interior(int F, const double *tri, int N, const int *dim_host, const long long *off_host,
                                 const int *dim, const long long *off, long long n_words, const double *consts,
                                 const int *offsets, const int *list, int n_pairs, unsigned long long *inter,
                                 void *stream) {
  int max_dim;
  if (F < 0 || n_pairs < 0) return refuse("rfd_objgrid_interior", "F, n_pairs >= 0");
  if (const char *bad = check_table(N, dim_host, off_host, n_words, &max_dim)) return refuse("rfd_objgrid_interior", bad);
  if (F == 0 || n_pairs == 0 || max_dim == 0) return 0;
  if (!tri || !dim || !off || !consts || !offsets || !list || !inter)
    return refuse("rfd_objgrid_interior", "a null pointer");
  const int blocks = min(ceil_div(max_dim * max_dim, WAVES), INTERIOR_MAX_BLOCKS);
  interior_kernel<<<dim3((unsigned)blocks, (unsigned)N), THREADS, 0, (hipStream_t)stream>>>(
      F, tri, N, dim, off, n_words, consts, offsets, list, n_pairs, inter);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_objgrid_finish(int N, const int *dim_host, const long long *off_host, const int *dim,
                               const long long *off, long long n_words, unsigned long long *words,
                               const unsigned long long *inter, int *cnt, void *stream) {
  int max_dim;
  if (const char *bad = check_table(N, dim_host, off_host, n_words, &max_dim)) return refuse("rfd_objgrid_finish", bad);
  if (max_dim == 0) return 0;
  if (!dim || !off || !words || !inter || !cnt) return refuse("rfd_objgrid_finish", "a null pointer");
  finish_kernel<<<dim3(FINISH_BLOCKS, (unsigned)N), THREADS, 0, (hipStream_t)stream>>>(N, dim, off, n_words, words, inter,
                                                                                    cnt);
  RFD_CHECK_LAUNCH();
  return 0;
}
