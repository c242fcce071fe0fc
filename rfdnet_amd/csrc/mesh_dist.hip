// mesh_dist.hip -- exact point-to-mesh distance over a ragged batch of meshes, the ragged surface samples and the
// per-segment sums of the surface metrics (include/rfd_mesh_dist.h; rules D1 - D8 are spelled out there and restated in
// tests/mesh_dist_f64.py).  The library is built with -ffp-contract=off, so every expression below is evaluated as
// written; f64 division and square root are the correctly rounded ones.
//
// The query is one thread per point: the best key (squared distance, face row), its closest point and the shell state
// live in registers, and the host orders the points by (object, cell) so that the lanes of a wave walk the same lists.
// The cell lists are one CSR for the batch, built in two passes with integer atomics, a workgroup working through 64
// triangles with all its threads on one triangle's box at a time (as mesh_sample.hip).  The sums are one wave per
// segment: lane j holds partial j, the tree runs through LDS.  No floating-point atomics, nothing waits for another
// workgroup, and every loop is bounded by the frame (at most R^3 cells and the object's lists) or by a segment.
#include <limits.h>
#include "common.h"
#include "../../include/rfd_mesh_dist.h"

namespace {

constexpr int THREADS = 256;
constexpr int TRI_PER_BLOCK = 64;
constexpr int SLABS = 8;                   // workgroups that share one triangle's box
constexpr int MAX_RES = 64;
constexpr int MAX_TAU = 8;
constexpr int WAVE = 64;

__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// rule D2: clamp((int)floor((x - lo) * inv_h), 0, R - 1) without ever converting a value that an int cannot hold
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

// the cross product of rule S1 / S4
__device__ __forceinline__ void face_cross(const double *t, double &cx, double &cy, double &cz) {
  const double ax = t[3] - t[0], ay = t[4] - t[1], az = t[5] - t[2];
  const double bx = t[6] - t[0], by = t[7] - t[1], bz = t[8] - t[2];
  cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
}

__global__ __launch_bounds__(THREADS) void faces_kernel(int F, int K, int V, const double *__restrict__ vertices,
                                                        const int *__restrict__ faces, const int *__restrict__ vend,
                                                        const int *__restrict__ tend, double *__restrict__ tri,
                                                        unsigned char *__restrict__ valid, int *__restrict__ fobj) {
  const int f = blockIdx.x * THREADS + threadIdx.x;
  if (f >= F) return;
  const int k = segment_of(tend, K, f);
  const int v0 = vend[k], nv = vend[k + 1] - v0;
  double t[9];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int idx = faces[3 * (size_t)f + c];
    const bool in = idx >= 0 && idx < nv && v0 >= 0 && v0 + idx < V;      // never outside the V rows
    ok = ok && in;
    const double *p = vertices + 3 * (size_t)(in ? v0 + idx : 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[3 * c + a] = in ? p[a] : 0.;
      ok = ok && isfinite(t[3 * c + a]);
    }
  }
  if (ok) {
    double cx, cy, cz;
    face_cross(t, cx, cy, cz);
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    ok = isfinite(area) && area != 0.;
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) tri[9 * (size_t)f + a] = t[a];      // the corners as they are; zeros for an index out of range
  valid[f] = ok ? 1 : 0;
  fobj[f] = k;
}

__global__ __launch_bounds__(THREADS) void boxes_kernel(int F, int K, const double *__restrict__ tri,
                                                        const unsigned char *__restrict__ valid,
                                                        const int *__restrict__ fobj, const double *__restrict__ lo,
                                                        const double *__restrict__ inv_h, const int *__restrict__ res,
                                                        const int *__restrict__ cbase, int *__restrict__ box) {
  const int f = blockIdx.x * THREADS + threadIdx.x;
  if (f >= F) return;
  int *b = box + 8 * (size_t)f;
  const int k = fobj[f];
  if (!valid[f] || k < 0 || k >= K) {
    b[0] = 0, b[1] = -1, b[2] = 0, b[3] = -1, b[4] = 0, b[5] = -1, b[6] = 0, b[7] = 1;
    return;
  }
  const int R = min(max(res[k], 1), MAX_RES);
  const double *t = tri + 9 * (size_t)f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double l = lo[3 * k + a], ih = inv_h[3 * k + a];
    const int c0 = cell_of(t[a], l, ih, R), c1 = cell_of(t[3 + a], l, ih, R), c2 = cell_of(t[6 + a], l, ih, R);
    b[2 * a] = min(min(c0, c1), c2), b[2 * a + 1] = max(max(c0, c1), c2);
  }
  b[6] = cbase[k], b[7] = R;
}

__global__ __launch_bounds__(THREADS) void cells_kernel(int F, const int *__restrict__ box, int n_cells,
                                                        int *__restrict__ cursor, int *__restrict__ list) {
  __shared__ int sbox[TRI_PER_BLOCK][8];
  const int f0 = blockIdx.x * TRI_PER_BLOCK;
  const int nt = min(TRI_PER_BLOCK, F - f0);
  for (int k = threadIdx.x; k < nt * 8; k += THREADS) (&sbox[0][0])[k] = box[8 * (size_t)f0 + k];
  __syncthreads();
  const int first = blockIdx.y * THREADS + threadIdx.x, step = gridDim.y * THREADS;
  for (int t = 0; t < nt; ++t) {
    const int x0 = sbox[t][0], y0 = sbox[t][2], z0 = sbox[t][4], base = sbox[t][6], R = sbox[t][7];
    const int nx = sbox[t][1] - x0 + 1, ny = sbox[t][3] - y0 + 1, nz = sbox[t][5] - z0 + 1;
    // a box the frame cannot hold (not one that boxes_kernel wrote) is skipped: no slot outside the cursor array
    if (nx < 1 || ny < 1 || nz < 1 || x0 < 0 || y0 < 0 || z0 < 0 || R < 1 || R > MAX_RES || x0 + nx > R || y0 + ny > R ||
        z0 + nz > R || base < 0 || base > n_cells - R * R * R)
      continue;
    const int n = nx * ny * nz;                                        // <= 64^3
    for (int c = first; c < n; c += step) {
      const int cell = base + ((x0 + c / (ny * nz)) * R + (y0 + (c / nz) % ny)) * R + (z0 + c % nz);
      const int slot = atomicAdd(cursor + cell, 1);
      if (list) list[slot] = f0 + t;
    }
  }
}

struct Best {
  double d2, qx, qy, qz;
  int face;
};

// rules D4 and D5: triangle `row` against p
__device__ __forceinline__ void closest_of(const double *__restrict__ t, int row, double px, double py, double pz,
                                           Best &best) {
  const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  double qx, qy, qz;
  if (d1 <= 0. && d2 <= 0.) qx = ax, qy = ay, qz = az;
  else if (d3 >= 0. && d4 <= d3) qx = bx, qy = by, qz = bz;
  else if (d6 >= 0. && d5 <= d6) qx = cx, qy = cy, qz = cz;
  else if (vc <= 0. && d1 >= 0. && d3 <= 0.) {
    const double s = d1 / (d1 - d3);
    qx = ax + abx * s, qy = ay + aby * s, qz = az + abz * s;
  } else if (vb <= 0. && d2 >= 0. && d6 <= 0.) {
    const double s = d2 / (d2 - d6);
    qx = ax + acx * s, qy = ay + acy * s, qz = az + acz * s;
  } else if (va <= 0. && d4 - d3 >= 0. && d5 - d6 >= 0.) {
    const double s = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    qx = bx + (cx - bx) * s, qy = by + (cy - by) * s, qz = bz + (cz - bz) * s;
  } else {
    const double e = 1. / ((va + vb) + vc);
    const double v = vb * e, w = vc * e;
    qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
  }
  const double rx = px - qx, ry = py - qy, rz = pz - qz;
  const double dd = (rx * rx + ry * ry) + rz * rz;
  if (dd < best.d2 || (dd == best.d2 && row < best.face)) {      // false for a NaN; +inf never beats the start (-1)
    best.d2 = dd, best.face = row, best.qx = qx, best.qy = qy, best.qz = qz;
  }
}

__device__ __forceinline__ void visit_cell(int cell, int F, const int *__restrict__ offsets, const int *__restrict__ list,
                                           const double *__restrict__ tri, double px, double py, double pz, Best &best) {
  const int end = offsets[cell + 1];
  for (int s = offsets[cell]; s < end; ++s) {
    const int row = list[s];
    if (row < 0 || row >= F) continue;
    closest_of(tri + 9 * (size_t)row, row, px, py, pz, best);
  }
}

__global__ __launch_bounds__(THREADS) void query_kernel(
    int n, const double *__restrict__ points, const int *__restrict__ qobj, int K, int F, const double *__restrict__ lo,
    const double *__restrict__ hi, const double *__restrict__ inv_h, const double *__restrict__ hh,
    const double *__restrict__ slack, const int *__restrict__ res, const int *__restrict__ cbase,
    const int *__restrict__ offsets, const int *__restrict__ list, const double *__restrict__ tri,
    double *__restrict__ d2out, int *__restrict__ faceout, double *__restrict__ closest) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const double nan = __builtin_nan("");
  const double p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
  const int k = qobj[i];
  Best best;
  best.d2 = __builtin_inf(), best.face = -1, best.qx = best.qy = best.qz = nan;
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) || k < 0 || k >= K) {
    best.d2 = nan;
  } else {
    const int R = min(max(res[k], 1), MAX_RES), base = cbase[k];
    const double sl = slack[k];
    double pp[3], l[3], h[3];
    int c[3], Ra[3];
    double out2;
    {
      double o[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        l[a] = lo[3 * k + a], h[a] = hh[3 * k + a];
        const double ih = inv_h[3 * k + a];
        pp[a] = fmin(fmax(p[a], l[a]), hi[3 * k + a]);
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
          const int row = base + (x * R + y) * R;
          if (xr || y - c[1] == r || c[1] - y == r) {
            for (int z = z0; z <= z1; ++z) visit_cell(row + z, F, offsets, list, tri, p[0], p[1], p[2], best);
          } else {
            if (c[2] - r >= 0) visit_cell(row + c[2] - r, F, offsets, list, tri, p[0], p[1], p[2], best);
            if (c[2] + r <= Ra[2] - 1) visit_cell(row + c[2] + r, F, offsets, list, tri, p[0], p[1], p[2], best);
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
      if (best.d2 < bound) break;
    }
  }
  const bool none = best.face < 0;
  d2out[i] = best.d2;
  faceout[i] = best.face;
  if (closest) {
    closest[3 * (size_t)i] = none ? nan : best.qx;
    closest[3 * (size_t)i + 1] = none ? nan : best.qy;
    closest[3 * (size_t)i + 2] = none ? nan : best.qz;
  }
}

__global__ __launch_bounds__(THREADS) void sample_kernel(int K, int count, const double *__restrict__ tri,
                                                         const int *__restrict__ tend, const double *__restrict__ cum,
                                                         const double *__restrict__ u, double *__restrict__ points,
                                                         int *__restrict__ face, double *__restrict__ normals) {
  const int i = blockIdx.x * THREADS + threadIdx.x;                     // K count <= INT_MAX / 3
  if (i >= K * count) return;
  const int k = i / count;
  const int f0 = tend[k], Fk = tend[k + 1] - f0;
  double *pt = points + 3 * (size_t)i;
  if (Fk < 1) {
    const double nan = __builtin_nan("");
    pt[0] = pt[1] = pt[2] = nan;
    face[i] = -1;
    if (normals) normals[3 * (size_t)i] = normals[3 * (size_t)i + 1] = normals[3 * (size_t)i + 2] = 0.;
    return;
  }
  const double *cm = cum + f0;
  const double target = u[3 * (size_t)i] * cm[Fk - 1];
  int lo = 0, hi = Fk - 1;                 // the first f with cum[f] >= target, Fk - 1 if there is none (a NaN too)
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cm[mid] >= target) hi = mid;
    else lo = mid + 1;
  }
  const double *t = tri + 9 * (size_t)(f0 + lo);
  double a = u[3 * (size_t)i + 1], b = u[3 * (size_t)i + 2];
  if (a + b > 1.) a = fabs(a - 1.), b = fabs(b - 1.);
#pragma unroll
  for (int c = 0; c < 3; ++c) pt[c] = t[c] + ((t[3 + c] - t[c]) * a + (t[6 + c] - t[c]) * b);
  face[i] = f0 + lo;
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

__global__ __launch_bounds__(WAVE) void sums_kernel(int S, int n, int F, const int *__restrict__ seg,
                                                    const double *__restrict__ d2, const int *__restrict__ face,
                                                    const double *__restrict__ normals, const double *__restrict__ tri,
                                                    int T, const double *__restrict__ tau, double *__restrict__ sums,
                                                    int *__restrict__ counts) {
  __shared__ double part[3][WAVE];
  __shared__ int cnt[1 + MAX_TAU][WAVE];
  const int s = blockIdx.x, j = threadIdx.x;
  const int e0 = min(max(seg[s], 0), n), e1 = min(max(seg[s + 1], e0), n);      // never outside the n entries
  double th[MAX_TAU];
  int within[MAX_TAU];
#pragma unroll
  for (int t = 0; t < MAX_TAU; ++t) th[t] = t < T ? tau[t] : 0., within[t] = 0;
  double sd = 0., sd2 = 0., sn = 0.;
  int left_out = 0;
  for (int e = e0 + j; e < e1; e += WAVE) {
    const double v = d2[e];
    const double d = sqrt(v);
    const int row = face[e];
    if (!isfinite(d) || row < 0 || row >= F) {
      ++left_out;
      continue;
    }
    sd += d, sd2 += v;
    if (normals) {
      double cx, cy, cz;
      face_cross(tri + 9 * (size_t)row, cx, cy, cz);
      const double len = sqrt((cx * cx + cy * cy) + cz * cz);
      const bool flat = len == 0.;
      const double nx = flat ? 0. : cx / len, ny = flat ? 0. : cy / len, nz = flat ? 0. : cz / len;
      sn += fabs(dot3(normals[3 * (size_t)e], normals[3 * (size_t)e + 1], normals[3 * (size_t)e + 2], nx, ny, nz));
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

RFD_API int rfd_mdist_faces(int F, int K, int V, const double *vertices, const int *faces, const int *vend,
                            const int *tend, const double *lo, const double *inv_h, const int *res, const int *cbase,
                            double *tri, unsigned char *valid, int *fobj, int *box, void *stream) {
  if (F < 0 || K < 0 || V < 0) return rfd_invalid("rfd_mdist_faces: F, K, V >= 0");
  if (F > INT_MAX / 9 || V > INT_MAX / 3) return rfd_invalid("rfd_mdist_faces: 9 F and 3 V must stay below 2^31");
  if (F == 0) return 0;
  if (K < 1) return rfd_invalid("rfd_mdist_faces: faces without an object");
  if (!faces || !vend || !tend || !tri || !valid || !fobj || (V > 0 && !vertices))
    return rfd_invalid("rfd_mdist_faces: a null pointer");
  const unsigned blocks = (unsigned)ceil_div(F, THREADS);
  if (!lo) {
    faces_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(F, K, V, vertices, faces, vend, tend, tri, valid,
                                                              fobj);
  } else {
    if (!inv_h || !res || !cbase || !box) return rfd_invalid("rfd_mdist_faces: a null pointer");
    boxes_kernel<<<blocks, THREADS, 0, (hipStream_t)stream>>>(F, K, tri, valid, fobj, lo, inv_h, res, cbase, box);
  }
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mdist_cells(int F, const int *box, int n_cells, int *cursor, int *list, void *stream) {
  if (F < 0 || n_cells < 0) return rfd_invalid("rfd_mdist_cells: F, n_cells >= 0");
  if (F == 0) return 0;
  if (!box || !cursor) return rfd_invalid("rfd_mdist_cells: a null pointer");
  cells_kernel<<<dim3((unsigned)ceil_div(F, TRI_PER_BLOCK), SLABS), THREADS, 0, (hipStream_t)stream>>>(F, box, n_cells,
                                                                                                        cursor, list);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mdist_query(int n, const double *points, const int *qobj, int K, int F, const double *lo,
                            const double *hi, const double *inv_h, const double *h, const double *slack, const int *res,
                            const int *cbase, const int *offsets, const int *list, const double *tri, double *d2,
                            int *face, double *closest, void *stream) {
  if (n < 0 || K < 0 || F < 0) return rfd_invalid("rfd_mdist_query: n, K, F >= 0");
  if (n > INT_MAX / 3) return rfd_invalid("rfd_mdist_query: 3 n must stay below 2^31");
  if (n == 0) return 0;
  if (!points || !qobj || !d2 || !face ||
      (K > 0 && (!lo || !hi || !inv_h || !h || !slack || !res || !cbase || !offsets)) || (F > 0 && (!list || !tri)))
    return rfd_invalid("rfd_mdist_query: a null pointer");
  query_kernel<<<(unsigned)ceil_div(n, THREADS), THREADS, 0, (hipStream_t)stream>>>(
      n, points, qobj, K, F, lo, hi, inv_h, h, slack, res, cbase, offsets, list, tri, d2, face, closest);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mdist_sample(int K, int count, int F, const double *tri, const int *tend, const double *cum,
                             const double *u, double *points, int *face, double *normals, void *stream) {
  if (K < 0 || count < 0 || F < 0) return rfd_invalid("rfd_mdist_sample: K, count, F >= 0");
  if ((long long)K * count > INT_MAX / 3) return rfd_invalid("rfd_mdist_sample: 3 K count must stay below 2^31");
  if (K == 0 || count == 0) return 0;
  if (!tend || !u || !points || !face || (F > 0 && (!tri || !cum)))
    return rfd_invalid("rfd_mdist_sample: a null pointer");
  sample_kernel<<<(unsigned)ceil_div(K * count, THREADS), THREADS, 0, (hipStream_t)stream>>>(K, count, tri, tend, cum, u,
                                                                                             points, face, normals);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mdist_sums(int S, int n, int F, const int *seg, const double *d2, const int *face,
                           const double *normals, const double *tri, int T, const double *tau, double *sums,
                           int *counts, void *stream) {
  if (S < 0 || n < 0 || F < 0 || T < 0 || T > MAX_TAU) return rfd_invalid("rfd_mdist_sums: S, n, F >= 0, 0 <= T <= 8");
  if (n > INT_MAX / 3) return rfd_invalid("rfd_mdist_sums: 3 n must stay below 2^31");
  if (S == 0) return 0;
  if (!seg || !sums || !counts || (T > 0 && !tau) || (n > 0 && (!d2 || !face)) || (normals && F > 0 && !tri))
    return rfd_invalid("rfd_mdist_sums: a null pointer");
  sums_kernel<<<(unsigned)S, WAVE, 0, (hipStream_t)stream>>>(S, n, F, seg, d2, face, normals, tri, T, tau, sums, counts);
  RFD_CHECK_LAUNCH();
  return 0;
}
