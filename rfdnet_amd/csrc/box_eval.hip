// box_eval.hip -- detection evaluation on the device: oriented 3-D box IoU of every
// (detection, ground truth) pair and the greedy VOC matching (include/rfd_eval.h).
//
// Replaces the nested Python loops at the end of the reference's test sweep:
//   * box3d_iou (net_utils/box_util.py:90-115): per pair a Sutherland-Hodgman clip of the two
//     bird's-eye rectangles (:22-69), a scipy ConvexHull of the clipped polygon for its area
//     (:71-81), the height overlap and the volumes from three edge lengths (:83-88);
//   * eval_det_cls_wo_mesh (net_utils/eval_det.py:304-331): detections by descending score,
//     each takes the ground truth of its class it overlaps most; a true positive if that IoU
//     is above the threshold and the ground truth is still free.
// Both are small, latency-bound fp64 VALU kernels (K = 256 detections x G <= 64 ground truths per
// scene); the library is built with -ffp-contract=off, so the inside / outside decisions of the
// clip follow the reference's arithmetic exactly.
#include "common.h"

namespace {

constexpr int MAX_SCENES = 65535;   // gridDim.y
constexpr int IOU_THREADS = 64;
// A convex quadrilateral clipped by four half-planes has at most 8 vertices.  The buffers hold a
// few more: vertices are classified one by one in floating point, and a vertex that does not fit
// is dropped rather than written out of bounds.
constexpr int IOU_MAXV = 10;

struct P2 { double x, y; };

// box_util.py:83-88
__device__ __forceinline__ double box3d_vol(const double *c) {
  const double ax = c[0] - c[3], ay = c[1] - c[4], az = c[2] - c[5];
  const double bx = c[3] - c[6], by = c[4] - c[7], bz = c[5] - c[8];
  const double cx = c[0] - c[12], cy = c[1] - c[13], cz = c[2] - c[14];
  const double a = sqrt(ax * ax + ay * ay + az * az);
  const double b = sqrt(bx * bx + by * by + bz * bz);
  const double h = sqrt(cx * cx + cy * cy + cz * cz);
  return a * b * h;
}

// box_util.py:17-19 on the rectangle (corners 3,2,1,0; x and z)
__device__ __forceinline__ double rect_area(const P2 *r) {
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const P2 p = r[i], q = r[(i + 3) & 3];      // np.roll(., 1)[i] = [i - 1]
    s1 += p.x * q.y;
    s2 += p.y * q.x;
  }
  return 0.5 * fabs(s1 - s2);
}

// One thread per (detection, ground truth) pair.  The two polygon buffers of a thread live in LDS,
// [buffer][vertex][x|y][thread]: a runtime-indexed per-thread array would go to scratch memory, and
// this layout puts the 64 lanes of an access on consecutive words.
__global__ __launch_bounds__(IOU_THREADS) void box3d_iou_kernel(
    int K, int G, const double *__restrict__ pred, const double *__restrict__ gt,
    double *__restrict__ iou3d, double *__restrict__ iou2d) {
  __shared__ double s_poly[2][IOU_MAXV][2][IOU_THREADS];
  const int bi = blockIdx.y, t = threadIdx.x;
  const long pair = (long)blockIdx.x * IOU_THREADS + t;
  if (pair >= (long)K * G) return;
  const int k = (int)(pair / G), g = (int)(pair % G);
  const double *c1 = pred + ((size_t)bi * K + k) * 24;
  const double *c2 = gt + ((size_t)bi * G + g) * 24;

  P2 r1[4], r2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r1[i].x = c1[(3 - i) * 3 + 0]; r1[i].y = c1[(3 - i) * 3 + 2];
    r2[i].x = c2[(3 - i) * 3 + 0]; r2[i].y = c2[(3 - i) * 3 + 2];
  }
  const double area1 = rect_area(r1), area2 = rect_area(r2);

  // polygon_clip(rect1, rect2), box_util.py:22-69
  int cur = 0, n = 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) { s_poly[0][i][0][t] = r1[i].x; s_poly[0][i][1][t] = r1[i].y; }
  P2 cp1 = r2[3];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const P2 cp2 = r2[ci];
    if (n > 0) {
      const int nxt = cur ^ 1;
      int m = 0;
      P2 s = {s_poly[cur][n - 1][0][t], s_poly[cur][n - 1][1][t]};
      const double ex_ = cp2.x - cp1.x, ey_ = cp2.y - cp1.y;
      bool s_in = ex_ * (s.y - cp1.y) > ey_ * (s.x - cp1.x);
      for (int i = 0; i < n; ++i) {
        const P2 e = {s_poly[cur][i][0][t], s_poly[cur][i][1][t]};
        const bool e_in = ex_ * (e.y - cp1.y) > ey_ * (e.x - cp1.x);
        if (e_in != s_in) {                        // computeIntersection(), :40-46
          const double dcx = cp1.x - cp2.x, dcy = cp1.y - cp2.y;
          const double dpx = s.x - e.x, dpy = s.y - e.y;
          const double n1 = cp1.x * cp2.y - cp1.y * cp2.x;
          const double n2 = s.x * e.y - s.y * e.x;
          const double n3 = 1.0 / (dcx * dpy - dcy * dpx);
          if (m < IOU_MAXV) {
            s_poly[nxt][m][0][t] = (n1 * dpx - n2 * dcx) * n3;
            s_poly[nxt][m][1][t] = (n1 * dpy - n2 * dcy) * n3;
            ++m;
          }
        }
        if (e_in && m < IOU_MAXV) { s_poly[nxt][m][0][t] = e.x; s_poly[nxt][m][1][t] = e.y; ++m; }
        s = e; s_in = e_in;
      }
      cur = nxt; n = m;
    }
    cp1 = cp2;
  }

  // area of the clipped (convex) polygon: shoelace sum; fewer than 3 points or no area -> 0
  double inter_area = 0.0;
  if (n >= 3) {
    double acc = 0.0;
    P2 p = {s_poly[cur][n - 1][0][t], s_poly[cur][n - 1][1][t]};
    for (int i = 0; i < n; ++i) {
      const P2 q = {s_poly[cur][i][0][t], s_poly[cur][i][1][t]};
      acc += p.x * q.y - q.x * p.y;
      p = q;
    }
    inter_area = 0.5 * fabs(acc);
    if (!(inter_area > 0.0) || !(inter_area < 1.0e300)) inter_area = 0.0;   // NaN / inf from a degenerate edge
  }

  const double den2 = area1 + area2 - inter_area;
  const double ymax = fmin(c1[1], c2[1]);
  const double ymin = fmax(c1[4 * 3 + 1], c2[4 * 3 + 1]);
  const double inter_vol = inter_area * fmax(0.0, ymax - ymin);
  const double den3 = box3d_vol(c1) + box3d_vol(c2) - inter_vol;
  const size_t o = ((size_t)bi * K + k) * G + g;
  iou3d[o] = den3 > 0.0 ? inter_vol / den3 : 0.0;
  if (iou2d) iou2d[o] = den2 > 0.0 ? inter_area / den2 : 0.0;
}

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_MAX_K = 1024, MATCH_MAX_G = 256, MATCH_MAX_T = 4;

// One workgroup per (scene, class).  Phase 1, a thread per detection: its best ground truth of the
// class (independent of the other detections).  Phase 2, a thread per threshold: the walk down the
// score order with that threshold's `det` flags -- the only serial part, K steps on LDS.
__global__ __launch_bounds__(MATCH_THREADS) void ap_match_kernel(
    int C, int K, int G, int nT, const double *__restrict__ iou3d, const int *__restrict__ order,
    const unsigned char *__restrict__ det_valid, const int *__restrict__ gt_cls,
    const unsigned char *__restrict__ gt_valid, const double *__restrict__ thr,
    unsigned char *__restrict__ tp) {
  __shared__ double s_ov[MATCH_MAX_K];
  __shared__ short s_j[MATCH_MAX_K];            // -1: not a valid detection of this class (skipped)
  __shared__ unsigned char s_gt[MATCH_MAX_G];   // ground truth takes part for this class
  __shared__ unsigned char s_det[MATCH_MAX_T][MATCH_MAX_G];
  const int c = blockIdx.x, bi = blockIdx.y, b = gridDim.y, t = threadIdx.x;
  const size_t row = ((size_t)bi * C + c) * K;
  order += row; det_valid += row;
  iou3d += (size_t)bi * K * G;
  for (int g = t; g < G; g += MATCH_THREADS) {
    s_gt[g] = gt_valid[(size_t)bi * G + g] != 0 && gt_cls[(size_t)bi * G + g] == c;
    for (int ti = 0; ti < nT; ++ti) s_det[ti][g] = 0;
  }
  for (int ti = 0; ti < nT; ++ti)
    for (int k = t; k < K; k += MATCH_THREADS) tp[((size_t)ti * b + bi) * C * K + (size_t)c * K + k] = 0;
  __syncthreads();
  for (int r = t; r < K; r += MATCH_THREADS) {
    const int d = order[r];
    double ovmax = -INFINITY;
    int jmax = -1;
    const bool ok = d >= 0 && d < K && det_valid[d] != 0;
    if (ok) {
      jmax = -2;                                 // valid, no ground truth of the class
      const double *rowp = iou3d + (size_t)d * G;
      for (int g = 0; g < G; ++g) {
        if (!s_gt[g]) continue;
        const double v = rowp[g];
        if (v > ovmax) { ovmax = v; jmax = g; }
      }
    }
    s_ov[r] = ovmax;
    s_j[r] = (short)jmax;
  }
  __syncthreads();                               // also orders the zeroing of tp before the writes below
  if (t < nT) {
    const double th = thr[t];
    unsigned char *out = tp + ((size_t)t * b + bi) * C * K + (size_t)c * K;
    for (int r = 0; r < K; ++r) {
      const int j = s_j[r];
      if (j >= 0 && s_ov[r] > th && !s_det[t][j]) {
        s_det[t][j] = 1;
        out[order[r]] = 1;
      }
    }
  }
}

}  // namespace

RFD_API int rfd_box3d_iou(int b, int K, int G, const double *pred_corners, const double *gt_corners,
                          double *iou3d, double *iou2d, void *stream) {
  if (b <= 0 || K <= 0 || G <= 0) return 0;
  if (b > MAX_SCENES) {                          // b is the grid's y extent
    return rfd_invalid("rfd_box3d_iou: need b <= 65535");
  }
  const long pairs = (long)K * G;
  hipLaunchKernelGGL(box3d_iou_kernel, dim3((unsigned)((pairs + IOU_THREADS - 1) / IOU_THREADS), b),
                     dim3(IOU_THREADS), 0, (hipStream_t)stream, K, G, pred_corners, gt_corners, iou3d, iou2d);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_ap_match(int b, int C, int K, int G, int nT, const double *iou3d, const int *order,
                         const unsigned char *det_valid, const int *gt_cls, const unsigned char *gt_valid,
                         const double *thr, unsigned char *tp, void *stream) {
  if (K > MATCH_MAX_K || G > MATCH_MAX_G || nT < 1 || nT > MATCH_MAX_T || G < 0 || b > MAX_SCENES || C > MAX_SCENES) {
    return rfd_invalid("rfd_ap_match: need K <= 1024, G <= 256, 1 <= nT <= 4, b and C <= 65535");
  }
  if (b <= 0 || C <= 0 || K <= 0) return 0;
  hipLaunchKernelGGL(ap_match_kernel, dim3(C, b), dim3(MATCH_THREADS), 0, (hipStream_t)stream, C, K, G, nT,
                     iou3d, order, det_valid, gt_cls, gt_valid, thr, tp);
  RFD_CHECK_LAUNCH();
  return 0;
}
