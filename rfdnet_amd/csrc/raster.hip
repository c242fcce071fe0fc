// raster.hip -- the scene render's rasteriser (include/rfd_render.h): projection, depth-tested triangles and points,
// shading.  The arithmetic of every rule is spelled out in the header and restated in tests/render_f64.py; the library
// is built with -ffp-contract=off, so the f64 expressions below are evaluated as written.
//
// Depth test: one atomicMax per covered pixel on a 64-bit key = (bits of the f32 1/z, 0xffffffff - primitive).  1/z is
// positive, so its bits order like its value: the nearest surface wins, the lowest primitive index wins a tie, and
// the result does not depend on the order in which workgroups run.  Nothing waits for anything.
#include "common.h"
#include "../../include/rfd_render.h"

namespace {

constexpr int RASTER_THREADS = 256;
constexpr int SMALL_BOX = 64;              // pixels of a clamped bounding box that one thread walks alone
constexpr int MAX_IMAGE = 8192;
constexpr int MAX_POINT_PX = 63;
constexpr double SCREEN_LIMIT = 1048576.0; // 2^20 pixels (rule 2)
constexpr float POINT_GREY = 0.55f;

struct Camera { double m[12], fx, fy, cx, cy; };

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// rules 1 and 2: one thread per vertex, then per scan point
__global__ __launch_bounds__(RASTER_THREADS) void raster_project_kernel(
    int V, int N, int point_stride, const float *__restrict__ vertices, const float *__restrict__ points, Camera cam,
    double near, double *__restrict__ q_out, int *__restrict__ sxy, unsigned char *__restrict__ valid) {
  const long r = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  if (r >= (long)V + N) return;
  const float *p = r < V ? vertices + 3 * r : points + (r - V) * (long)point_stride;
  const float Xf = p[0], Yf = p[1], Zf = p[2];
  double q = 0.0;
  int ix = 0, iy = 0;
  bool ok = finite_f32(Xf) && finite_f32(Yf) && finite_f32(Zf);
  if (ok) {
    const double X = Xf, Y = Yf, Z = Zf;
    const double xv = ((cam.m[0] * X + cam.m[1] * Y) + cam.m[2] * Z) + cam.m[3];
    const double yv = ((cam.m[4] * X + cam.m[5] * Y) + cam.m[6] * Z) + cam.m[7];
    const double zv = ((cam.m[8] * X + cam.m[9] * Y) + cam.m[10] * Z) + cam.m[11];
    ok = zv >= near;
    if (ok) {
      const double qq = 1.0 / zv;
      const double sx = (cam.fx * xv) * qq + cam.cx;
      const double sy = (cam.fy * yv) * qq + cam.cy;
      ok = fabs(sx) <= SCREEN_LIMIT && fabs(sy) <= SCREEN_LIMIT;
      if (ok) {                                     // |256 s + 0.5| < 2^29: the conversion is in range
        q = qq;
        ix = (int)floor(256.0 * sx + 0.5);
        iy = (int)floor(256.0 * sy + 0.5);
      }
    }
  }
  q_out[r] = q;
  sxy[2 * r] = ix;
  sxy[2 * r + 1] = iy;
  valid[r] = ok ? 1 : 0;
}

// a triangle ready to be tested at pixel centres: snapped corners, the sign that makes its area positive, the
// inclusive edges of the top-left rule, the clamped pixel box
struct Tri {
  long x[3], y[3];
  double q[3], area;
  long sign;
  bool incl[3];
  int i0, j0, nx, ny;
};

__device__ __forceinline__ bool tri_setup(int f, int V, int W, int H, const int *__restrict__ faces,
                                          const double *__restrict__ q, const int *__restrict__ sxy,
                                          const unsigned char *__restrict__ valid, Tri &t) {
  int xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = faces[3 * (long)f + c];
    if (v < 0 || v >= V || !valid[v]) return false;
    const int x = sxy[2 * (long)v], y = sxy[2 * (long)v + 1];
    t.x[c] = x, t.y[c] = y, t.q[c] = q[v];
    xmin = min(xmin, x), xmax = max(xmax, x), ymin = min(ymin, y), ymax = max(ymax, y);
  }
  const long area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
  if (area == 0) return false;
  t.sign = area < 0 ? -1 : 1;
  t.area = (double)(t.sign * area);
#pragma unroll
  for (int e = 0; e < 3; ++e) {                     // edge e runs from corner e+1 to corner e+2
    const long dx = t.sign * (t.x[(e + 2) % 3] - t.x[(e + 1) % 3]), dy = t.sign * (t.y[(e + 2) % 3] - t.y[(e + 1) % 3]);
    t.incl[e] = dy < 0 || (dy == 0 && dx > 0);
  }
  // pixels whose centre 256 i + 128 lies in [min, max], cut to the image (>> on a negative int rounds down)
  const int i0 = max((xmin + 127) >> 8, 0), i1 = min((xmax - 128) >> 8, W - 1);
  const int j0 = max((ymin + 127) >> 8, 0), j1 = min((ymax - 128) >> 8, H - 1);
  if (i1 < i0 || j1 < j0) return false;
  t.i0 = i0, t.j0 = j0, t.nx = i1 - i0 + 1, t.ny = j1 - j0 + 1;
  return true;
}

__device__ __forceinline__ void tri_pixel(const Tri &t, int i, int j, int W, unsigned prim,
                                          unsigned long long *__restrict__ keys) {
  const long px = 256L * i + 128, py = 256L * j + 128;
  long E[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int a = (e + 1) % 3, b = (e + 2) % 3;
    E[e] = t.sign * ((t.x[b] - t.x[a]) * (py - t.y[a]) - (t.y[b] - t.y[a]) * (px - t.x[a]));
    if (E[e] < 0 || (E[e] == 0 && !t.incl[e])) return;
  }
  const double w0 = (double)E[0] / t.area, w1 = (double)E[1] / t.area, w2 = (double)E[2] / t.area;
  const float invz = (float)((w0 * t.q[0] + w1 * t.q[1]) + w2 * t.q[2]);
  const unsigned long long key = ((unsigned long long)__float_as_uint(invz) << 32) | (0xffffffffu - prim);
  atomicMax(keys + (size_t)j * W + i, key);
}

// rules 3 and 4: thread p < F owns triangle p, thread F <= p < F + N scan point p - F.  A triangle whose clamped box
// has more than SMALL_BOX pixels is left in the workgroup's list and walked by all its threads afterwards.
__global__ __launch_bounds__(RASTER_THREADS) void raster_triangles_kernel(
    int V, int F, int N, int W, int H, int point_px, const int *__restrict__ faces, const double *__restrict__ q,
    const int *__restrict__ sxy, const unsigned char *__restrict__ valid, unsigned long long *__restrict__ keys) {
  __shared__ int s_big[RASTER_THREADS];            // thread t's large triangle, or -1
  const int tid = threadIdx.x;
  const long p = (long)blockIdx.x * RASTER_THREADS + tid;
  s_big[tid] = -1;
  if (p < F) {
    Tri t;
    if (tri_setup((int)p, V, W, H, faces, q, sxy, valid, t)) {
      if ((long)t.nx * t.ny <= SMALL_BOX) {
        for (int j = 0; j < t.ny; ++j)
          for (int i = 0; i < t.nx; ++i) tri_pixel(t, t.i0 + i, t.j0 + j, W, (unsigned)p, keys);
      } else {
        s_big[tid] = (int)p;
      }
    }
  } else if (p < (long)F + N) {
    const long r = (long)V + (p - F);
    if (valid[r]) {
      const int ci = sxy[2 * r] >> 8, cj = sxy[2 * r + 1] >> 8, h = point_px / 2;     // |ci|, |cj| <= 2^20
      const float invz = (float)q[r];
      const unsigned long long key = ((unsigned long long)__float_as_uint(invz) << 32) | (0xffffffffu - (unsigned)p);
      const int i0 = max(ci - h, 0), i1 = min(ci + h, W - 1), j0 = max(cj - h, 0), j1 = min(cj + h, H - 1);
      for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) atomicMax(keys + (size_t)j * W + i, key);
    }
  }
  __syncthreads();
  for (int b = 0; b < RASTER_THREADS; ++b) {
    const int f = s_big[b];                         // the same for every thread: no divergence
    Tri t;
    if (f < 0 || !tri_setup(f, V, W, H, faces, q, sxy, valid, t)) continue;     // it passed once already
    const int n = t.nx * t.ny;                      // <= W H <= 2^26
    for (int k = tid; k < n; k += RASTER_THREADS) tri_pixel(t, t.i0 + k % t.nx, t.j0 + k / t.nx, W, (unsigned)f, keys);
  }
}

__device__ __forceinline__ unsigned char to_u8(float c) {
  const float v = floorf(255.f * c + 0.5f);
  return (unsigned char)(v >= 255.f ? 255.f : v >= 0.f ? v : 0.f);     // a NaN gives 0
}

// rule 5: one thread per pixel
__global__ __launch_bounds__(RASTER_THREADS) void raster_shade_kernel(
    int F, int K, int C, int W, int H, const float *__restrict__ vertices, const int *__restrict__ faces,
    const int *__restrict__ face_obj, const int *__restrict__ obj_class, const float *__restrict__ palette,
    float ex, float ey, float ez, const unsigned long long *__restrict__ keys, int *__restrict__ ids,
    float *__restrict__ depth, unsigned char *__restrict__ image) {
  const long pix = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  if (pix >= (long)W * H) return;
  const unsigned long long key = keys[pix];
  float r = 1.f, g = 1.f, b = 1.f, z = __uint_as_float(0x7f800000u);
  int id = -1;
  if (key != 0) {
    const unsigned prim = 0xffffffffu - (unsigned)(key & 0xffffffffu);
    id = (int)prim;
    z = (float)(1.0 / (double)__uint_as_float((unsigned)(key >> 32)));
    if (prim >= (unsigned)F) {
      r = g = b = POINT_GREY;
    } else {
      const int *fv = faces + 3 * (long)prim;
      const float *pa = vertices + 3 * (long)fv[0], *pb = vertices + 3 * (long)fv[1], *pc = vertices + 3 * (long)fv[2];
      const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2];
      const float wx = pc[0] - pa[0], wy = pc[1] - pa[1], wz = pc[2] - pa[2];
      const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
      const float vx = ex - ((pa[0] + pb[0]) + pc[0]) / 3.f, vy = ey - ((pa[1] + pb[1]) + pc[1]) / 3.f,
                  vz = ez - ((pa[2] + pb[2]) + pc[2]) / 3.f;
      const float dot = (nx * vx + ny * vy) + nz * vz;
      const float nn = (nx * nx + ny * ny) + nz * nz, vv = (vx * vx + vy * vy) + vz * vz;
      float s = 0.3f + 0.7f * (fabsf(dot) / (sqrtf(nn) * sqrtf(vv)));
      if (!(s == s)) s = 0.3f;
      const int o = min(max(face_obj[prim], 0), K - 1);
      const int c = min(max(obj_class[o], 0), C - 1);
      r = palette[3 * c] * s, g = palette[3 * c + 1] * s, b = palette[3 * c + 2] * s;
    }
  }
  ids[pix] = id;
  depth[pix] = z;
  image[3 * pix] = to_u8(r), image[3 * pix + 1] = to_u8(g), image[3 * pix + 2] = to_u8(b);
}

int check_counts(int V, int F, int N) {
  if (V < 0 || F < 0 || N < 0) return rfd_invalid("raster: a negative count");
  if ((long)V + N > INT_MAX || (long)F + N > INT_MAX) return rfd_invalid("raster: V + N and F + N must stay below 2^31");
  return 0;
}

int check_image(int W, int H) {
  if (W < 1 || H < 1 || W > MAX_IMAGE || H > MAX_IMAGE) return rfd_invalid("raster: 1 <= W, H <= 8192");
  return 0;
}

}  // namespace

RFD_API int rfd_raster_project(int V, int N, int point_stride, const float *vertices, const float *points,
                               const double *camera, double near, double *q, int *sxy, unsigned char *valid,
                               void *stream) {
  if (int rc = check_counts(V, 0, N)) return rc;
  if (!(near > 0.0)) return rfd_invalid("rfd_raster_project: near must be positive");
  if (N > 0 && point_stride < 3) return rfd_invalid("rfd_raster_project: a scan point has at least three floats");
  if (!camera) return rfd_invalid("rfd_raster_project: no camera");
  const long n = (long)V + N;
  if (n == 0) return 0;
  Camera cam;
  for (int i = 0; i < 12; ++i) cam.m[i] = camera[i];
  cam.fx = camera[12], cam.fy = camera[13], cam.cx = camera[14], cam.cy = camera[15];
  raster_project_kernel<<<(unsigned)((n + RASTER_THREADS - 1) / RASTER_THREADS), RASTER_THREADS, 0,
                          (hipStream_t)stream>>>(V, N, point_stride, vertices, points, cam, near, q, sxy, valid);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_raster_triangles(int V, int F, int N, int W, int H, int point_px, const int *faces, const double *q,
                                 const int *sxy, const unsigned char *valid, unsigned long long *keys, void *stream) {
  if (int rc = check_counts(V, F, N)) return rc;
  if (int rc = check_image(W, H)) return rc;
  if (point_px < 1 || point_px > MAX_POINT_PX || point_px % 2 == 0)
    return rfd_invalid("rfd_raster_triangles: point_px is odd, 1..63");
  RFD_CHECK(hipMemsetAsync(keys, 0, (size_t)W * H * sizeof(unsigned long long), (hipStream_t)stream));
  const long n = (long)F + N;
  if (n == 0) return 0;
  raster_triangles_kernel<<<(unsigned)((n + RASTER_THREADS - 1) / RASTER_THREADS), RASTER_THREADS, 0,
                            (hipStream_t)stream>>>(V, F, N, W, H, point_px, faces, q, sxy, valid, keys);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_raster_shade(int F, int K, int C, int W, int H, const float *vertices, const int *faces,
                             const int *face_obj, const int *obj_class, const float *palette, const double *eye,
                             const unsigned long long *keys, int *ids, float *depth, unsigned char *image,
                             void *stream) {
  if (int rc = check_counts(0, F, 0)) return rc;
  if (int rc = check_image(W, H)) return rc;
  if (F > 0 && (K < 1 || C < 1)) return rfd_invalid("rfd_raster_shade: faces need an object and a palette entry");
  if (!eye) return rfd_invalid("rfd_raster_shade: no eye");
  const long n = (long)W * H;
  raster_shade_kernel<<<(unsigned)((n + RASTER_THREADS - 1) / RASTER_THREADS), RASTER_THREADS, 0,
                        (hipStream_t)stream>>>(F, K, C, W, H, vertices, faces, face_obj, obj_class, palette,
                                               (float)eye[0], (float)eye[1], (float)eye[2], keys, ids, depth, image);
  RFD_CHECK_LAUNCH();
  return 0;
}
