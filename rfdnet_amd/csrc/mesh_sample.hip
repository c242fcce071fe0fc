// mesh_sample.hip -- point-in-mesh, surface voxels and surface samples of a triangle mesh (include/rfd_sample.h; the
// rules are spelled out there and restated in tests/mesh_sample_ref.py).  The library is built with -ffp-contract=off, so
// every expression below is evaluated as written; f64 division and square root are the correctly rounded ones.
//
// The containment query is one thread per point: the point's cell list is walked with the two counters in registers.
// The cell lists are a CSR built in two passes with integer atomics (count, prefix sum by the caller, fill).  The passes
// over a triangle's box of cells (the lists, the voxeliser) never give a whole box to one lane: a workgroup takes 64
// triangles, stages what it needs of them in LDS, and all its threads work through one triangle's box at a time, the
// box further dealt over gridDim.y workgroups.  No floating-point atomics, nothing waits, every loop is bounded.
#include "common.h"
#include "../../include/rfd_sample.h"

namespace {

constexpr int THREADS = 256;
constexpr int TRI_PER_BLOCK = 64;
constexpr int SLABS = 8;                   // workgroups that share one triangle's box
constexpr int MAX_HASH_RES = 32768;        // res^2 < 2^31
constexpr int MAX_VOXEL_RES = 1024;        // R^3 < 2^31

// (int)x clamped to [0, last] (rule C3 / V2), without ever converting a value that an int cannot hold
template <typename T>
__device__ __forceinline__ int cell_of(T x, int last) {
  if (!(x >= (T)0)) return 0;
  if (x >= (T)(last + 1)) return last;
  return (int)x;
}

__global__ __launch_bounds__(THREADS) void rescale_kernel(int F, const double *__restrict__ tri, double sx, double sy,
                                                          double sz, double tx, double ty, double tz, int res,
                                                          double *__restrict__ out, int *__restrict__ box) {
  const int f = blockIdx.x * THREADS + threadIdx.x;
  if (f >= F) return;
  const double *t = tri + 9 * (size_t)f;
  double *o = out + 9 * (size_t)f;
  double x[3], y[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x[c] = sx * t[3 * c] + tx;
    y[c] = sy * t[3 * c + 1] + ty;
    o[3 * c] = x[c], o[3 * c + 1] = y[c], o[3 * c + 2] = sz * t[3 * c + 2] + tz;
  }
  const double x0 = fmin(fmin(x[0], x[1]), x[2]), x1 = fmax(fmax(x[0], x[1]), x[2]);
  const double y0 = fmin(fmin(y[0], y[1]), y[2]), y1 = fmax(fmax(y[0], y[1]), y[2]);
  int *b = box + 4 * (size_t)f;
  b[0] = cell_of(x0, res - 1), b[1] = cell_of(x1, res - 1), b[2] = cell_of(y0, res - 1), b[3] = cell_of(y1, res - 1);
}

__global__ __launch_bounds__(THREADS) void cells_kernel(int F, const int *__restrict__ box, int res,
                                                        int *__restrict__ cursor, int *__restrict__ list) {
  __shared__ int sbox[TRI_PER_BLOCK][4];
  const int f0 = blockIdx.x * TRI_PER_BLOCK;
  const int nt = min(TRI_PER_BLOCK, F - f0);
  if ((int)threadIdx.x < nt * 4) (&sbox[0][0])[threadIdx.x] = box[4 * (size_t)f0 + threadIdx.x];
  __syncthreads();
  const int first = blockIdx.y * THREADS + threadIdx.x, step = gridDim.y * THREADS;
  for (int t = 0; t < nt; ++t) {
    const int x0 = sbox[t][0], y0 = sbox[t][2];
    const int nx = sbox[t][1] - x0 + 1, ny = sbox[t][3] - y0 + 1;      // 1 <= nx, ny <= res: nx ny < 2^31
    const int n = nx * ny;
    for (int c = first; c < n; c += step) {
      const int cell = (x0 + c / ny) * res + (y0 + c % ny);
      const int slot = atomicAdd(cursor + cell, 1);
      if (list) list[slot] = f0 + t;
    }
  }
}

__global__ __launch_bounds__(THREADS) void contains_kernel(int n, const double *__restrict__ points, double sx, double sy,
                                                           double sz, double tx, double ty, double tz, int res,
                                                           const double *__restrict__ tris,
                                                           const int *__restrict__ offsets, const int *__restrict__ list,
                                                           unsigned char *__restrict__ contains, int *__restrict__ out0,
                                                           int *__restrict__ out1) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const double px = sx * points[3 * (size_t)i] + tx, py = sy * points[3 * (size_t)i + 1] + ty,
               pz = sz * points[3 * (size_t)i + 2] + tz;
  const double r = (double)res;
  int n0 = 0, n1 = 0;
  if (px >= 0. && px < r && py >= 0. && py < r && pz >= 0. && pz <= r) {      // rule C3; false for a NaN
    const int cell = (int)px * res + (int)py;
    const int end = offsets[cell + 1];
    for (int k = offsets[cell]; k < end; ++k) {
      const double *t = tris + 9 * (size_t)list[k];
      const double t1x = t[0], t1y = t[1], t2x = t[3], t2y = t[4], t3x = t[6], t3y = t[7];
      const double A00 = t1x - t3x, A10 = t1y - t3y, A01 = t2x - t3x, A11 = t2y - t3y;
      const double det = A00 * A11 - A01 * A10;
      if (det == 0.) continue;
      const double s = det > 0. ? 1. : -1., ad = fabs(det);
      const double y0 = px - t3x, y1 = py - t3y;
      const double u = (A11 * y0 - A01 * y1) * s;
      const double v = (-A10 * y0 + A00 * y1) * s;
      const double w = u + v;
      if (!(0. < u && u < ad && 0. < v && v < ad && 0. < w && w < ad)) continue;
      const double t1z = t[2], t2z = t[5], t3z = t[8];
      const double v1x = t3x - t1x, v1y = t3y - t1y, v1z = t3z - t1z;
      const double v2x = t2x - t1x, v2y = t2y - t1y, v2z = t2z - t1z;
      const double nn0 = v1y * v2z - v1z * v2y, nn1 = v1z * v2x - v1x * v2z, nn2 = v1x * v2y - v1y * v2x;
      if (nn2 == 0.) continue;
      const double alpha = nn0 * (t1x - px) + nn1 * (t1y - py);
      const double an = fabs(nn2), sn = nn2 > 0. ? 1. : -1.;
      const double depth = t1z * an + alpha * sn, rhs = pz * an;
      if (depth >= rhs) ++n0;
      else if (depth < rhs) ++n1;
    }
  }
  contains[i] = (unsigned char)((n0 & 1) & (n1 & 1));
  if (out0) out0[i] = n0;
  if (out1) out1[i] = n1;
}

// one of the nine axis tests of rule V3: true = separated
__device__ __forceinline__ bool separated(float pa, float pb, float fa, float fb) {
  float mn, mx;
  if (pa < pb) mn = pa, mx = pb;
  else mn = pb, mx = pa;
  const float rad = fa * 0.5f + fb * 0.5f;
  return mn > rad || mx < -rad;
}

__device__ __forceinline__ bool apart(float a, float b, float c) {      // FINDMINMAX and the test against the half size
  float mn = a, mx = a;
  if (b < mn) mn = b;
  if (b > mx) mx = b;
  if (c < mn) mn = c;
  if (c > mx) mx = c;
  return mn > 0.5f || mx < -0.5f;
}

// rule V3: tri (9 floats) against the voxel with centre (cx, cy, cz)
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

__global__ __launch_bounds__(THREADS) void voxelize_kernel(int F, const float *__restrict__ tri, int R,
                                                           unsigned char *__restrict__ grid) {
  __shared__ float stri[TRI_PER_BLOCK][9];
  __shared__ int sbox[TRI_PER_BLOCK][6];
  const int f0 = blockIdx.x * TRI_PER_BLOCK;
  const int nt = min(TRI_PER_BLOCK, F - f0);
  for (int k = threadIdx.x; k < nt * 9; k += THREADS) (&stri[0][0])[k] = tri[9 * (size_t)f0 + k];
  __syncthreads();
  if ((int)threadIdx.x < nt * 3) {      // rule V2, one axis of one triangle
    const int t = threadIdx.x / 3, a = threadIdx.x % 3;
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
    const int i0 = sbox[t][0], j0 = sbox[t][2], k0 = sbox[t][4];
    const int nj = sbox[t][3] - j0 + 1, nk = sbox[t][5] - k0 + 1;
    const int n = (sbox[t][1] - i0 + 1) * nj * nk;                      // <= R^3 < 2^31
    for (int c = first; c < n; c += step) {
      const int i = i0 + c / (nj * nk), j = j0 + (c / nk) % nj, k = k0 + c % nk;
      if (tri_box_overlap(stri[t], (float)(i + 0.5), (float)(j + 0.5), (float)(k + 0.5)))
        grid[((size_t)i * R + j) * R + k] = 1;                          // rule V4: every writer writes the same byte
    }
  }
}

__device__ __forceinline__ void face_cross(const double *t, double &cx, double &cy, double &cz) {
  const double ax = t[3] - t[0], ay = t[4] - t[1], az = t[5] - t[2];
  const double bx = t[6] - t[0], by = t[7] - t[1], bz = t[8] - t[2];
  cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
}

__global__ __launch_bounds__(THREADS) void face_areas_kernel(int F, const double *__restrict__ tri,
                                                             double *__restrict__ area) {
  const int f = blockIdx.x * THREADS + threadIdx.x;
  if (f >= F) return;
  double cx, cy, cz;
  face_cross(tri + 9 * (size_t)f, cx, cy, cz);
  area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ __launch_bounds__(THREADS) void surface_kernel(int count, int F, const double *__restrict__ tri,
                                                          const double *__restrict__ cum, const double *__restrict__ u,
                                                          double *__restrict__ points, int *__restrict__ face,
                                                          double *__restrict__ normals) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  const double target = u[3 * (size_t)i] * cum[F - 1];
  int lo = 0, hi = F - 1;                  // the first f with cum[f] >= target, F - 1 if there is none (a NaN too)
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cum[mid] >= target) hi = mid;
    else lo = mid + 1;
  }
  const double *t = tri + 9 * (size_t)lo;
  double a = u[3 * (size_t)i + 1], b = u[3 * (size_t)i + 2];
  if (a + b > 1.) a = fabs(a - 1.), b = fabs(b - 1.);
#pragma unroll
  for (int c = 0; c < 3; ++c) points[3 * (size_t)i + c] = t[c] + ((t[3 + c] - t[c]) * a + (t[6 + c] - t[c]) * b);
  face[i] = lo;
  if (normals) {
    double cx, cy, cz;
    face_cross(t, cx, cy, cz);
    const double len = sqrt((cx * cx + cy * cy) + cz * cz);
    const bool flat = len == 0.;
    normals[3 * (size_t)i] = flat ? 0. : cx / len;
    normals[3 * (size_t)i + 1] = flat ? 0. : cy / len;
    normals[3 * (size_t)i + 2] = flat ? 0. : cz / len;
  }
}

}  // namespace

RFD_API int rfd_sample_rescale(int F, const double *tri, double sx, double sy, double sz, double tx, double ty, double tz,
                               int res, double *rescaled, int *box, void *stream) {
  if (F < 0 || res < 2 || res > MAX_HASH_RES) return rfd_invalid("rfd_sample_rescale: F >= 0, 2 <= res <= 32768");
  if (F == 0) return 0;
  if (!tri || !rescaled || !box) return rfd_invalid("rfd_sample_rescale: a null pointer");
  rescale_kernel<<<(unsigned)ceil_div(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, tri, sx, sy, sz, tx, ty, tz,
                                                                                     res, rescaled, box);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_sample_cells(int F, const int *box, int res, int *cursor, int *list, void *stream) {
  if (F < 0 || res < 2 || res > MAX_HASH_RES) return rfd_invalid("rfd_sample_cells: F >= 0, 2 <= res <= 32768");
  if (F == 0) return 0;
  if (!box || !cursor) return rfd_invalid("rfd_sample_cells: a null pointer");
  cells_kernel<<<dim3((unsigned)ceil_div(F, TRI_PER_BLOCK), SLABS), THREADS, 0, (hipStream_t)stream>>>(F, box, res,
                                                                                                        cursor, list);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_sample_contains(int n, const double *points, double sx, double sy, double sz, double tx, double ty,
                                double tz, int res, int F, const double *rescaled, const int *offsets, const int *list,
                                unsigned char *contains, int *n0, int *n1, void *stream) {
  if (n < 0 || F < 0 || res < 2 || res > MAX_HASH_RES)
    return rfd_invalid("rfd_sample_contains: n, F >= 0, 2 <= res <= 32768");
  if (n > INT_MAX / 3) return rfd_invalid("rfd_sample_contains: 3 n must stay below 2^31");
  if (n == 0) return 0;
  if (!points || !contains || !offsets || (F > 0 && (!rescaled || !list)))
    return rfd_invalid("rfd_sample_contains: a null pointer");
  contains_kernel<<<(unsigned)ceil_div(n, THREADS), THREADS, 0, (hipStream_t)stream>>>(
      n, points, sx, sy, sz, tx, ty, tz, res, rescaled, offsets, list, contains, n0, n1);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_sample_voxelize(int F, const float *tri, int R, unsigned char *grid, void *stream) {
  if (F < 0 || R < 1 || R > MAX_VOXEL_RES) return rfd_invalid("rfd_sample_voxelize: F >= 0, 1 <= R <= 1024");
  if (F == 0) return 0;
  if (!tri || !grid) return rfd_invalid("rfd_sample_voxelize: a null pointer");
  voxelize_kernel<<<dim3((unsigned)ceil_div(F, TRI_PER_BLOCK), SLABS), THREADS, 0, (hipStream_t)stream>>>(F, tri, R,
                                                                                                           grid);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_sample_face_areas(int F, const double *tri, double *area, void *stream) {
  if (F < 0) return rfd_invalid("rfd_sample_face_areas: F >= 0");
  if (F == 0) return 0;
  if (!tri || !area) return rfd_invalid("rfd_sample_face_areas: a null pointer");
  face_areas_kernel<<<(unsigned)ceil_div(F, THREADS), THREADS, 0, (hipStream_t)stream>>>(F, tri, area);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_sample_surface(int count, int F, const double *tri, const double *cum, const double *u, double *points,
                               int *face, double *normals, void *stream) {
  if (count < 0 || F < 0) return rfd_invalid("rfd_sample_surface: count, F >= 0");
  if (count > INT_MAX / 3) return rfd_invalid("rfd_sample_surface: 3 count must stay below 2^31");
  if (count == 0) return 0;
  if (F < 1) return rfd_invalid("rfd_sample_surface: samples of a mesh without faces");
  if (!tri || !cum || !u || !points || !face) return rfd_invalid("rfd_sample_surface: a null pointer");
  surface_kernel<<<(unsigned)ceil_div(count, THREADS), THREADS, 0, (hipStream_t)stream>>>(count, F, tri, cum, u, points,
                                                                                         face, normals);
  RFD_CHECK_LAUNCH();
  return 0;
}
