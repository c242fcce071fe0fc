// fit_pose.hip -- the optimisation loop of fit_mesh_to_scan on the device (include/rfd_fit.h): per iteration one
// nearest-neighbour launch over the ragged (object, scan tile) list and one one-workgroup launch that finishes the loss
// and the gradient, keeps the best parameters and applies Adam.  The iteration boundary is the kernel boundary.
//
// Search: chamfer_nn_kernel's (chamfer.hip) -- a thread owns its scan points in registers, the object's mesh points stream
// through LDS in tiles of 1024 float4 and are transformed by the current pose while they are staged.  The loss depends
// on four parameters per object and the assignment is piecewise constant, so the gradient is four sums over the
// object's scan points: no per-point gradient buffers, no atomics.  Sums as in det_loss.hip: f64, thread t takes its points in
// order, then a tree in LDS.
#include "common.h"
#include "../../include/rfd_fit.h"
#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WG = 256;
constexpr int TILE_PTS = 1024;
constexpr int TERMS = 5;                 // loss, d/dcx, d/dcy, d/dcz, d/dtheta
constexpr int MAX_ITERATIONS = 100000;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the pose applied to one mesh point: fp32, products summed left to right (the library is built with -ffp-contract=off)
__device__ __forceinline__ f32x4 pose_point(const float *__restrict__ o, float c, float s, float cx, float cy, float cz) {
  const float ox = o[0], oy = o[1], oz = o[2];
  const float ns = -s;
  return f32x4{ox * c + oy * ns + cx, ox * s + oy * c + cy, oz + cz, 0.f};
}

template <int PPT>
__global__ __launch_bounds__(WG) void fit_nn_kernel(int P, int n_obj, int n_scan, const float *__restrict__ obj,
                                                    const int *__restrict__ obj_off, const float *__restrict__ scan,
                                                    const int *__restrict__ scan_off, const int *__restrict__ tile_obj,
                                                    const int *__restrict__ tile_start, const float *__restrict__ params,
                                                    double *__restrict__ partial) {
  __shared__ f32x4 s_pt[TILE_PTS];
  __shared__ double s_red[TERMS][WG];
  __shared__ float s_cs[2];
  const int t = threadIdx.x, tile = blockIdx.x;
  const int p = clampi(tile_obj[tile], 0, P - 1);
  const int o0 = clampi(obj_off[p], 0, n_obj), o1 = clampi(obj_off[p + 1], o0, n_obj);
  const int s0 = clampi(scan_off[p], 0, n_scan), s1 = clampi(scan_off[p + 1], s0, n_scan);
  const int start = clampi(tile_start[tile], s0, s1);
  const int m = o1 - o0;
  double acc[TERMS];
#pragma unroll
  for (int i = 0; i < TERMS; ++i) acc[i] = 0.0;
  if (m > 0 && start < s1) {               // uniform over the workgroup
    const float cx = params[4 * p], cy = params[4 * p + 1], cz = params[4 * p + 2];
    if (t == 0) {                          // once per workgroup: the f64 functions, rounded (rfd_fit.h)
      const double th = (double)params[4 * p + 3];
      s_cs[0] = (float)cos(th);
      s_cs[1] = (float)sin(th);
    }
    __syncthreads();
    const float c = s_cs[0], s = s_cs[1];
    const float *po = obj + (size_t)o0 * 3;
    const int j0 = start + t * PPT;
    float qx[PPT], qy[PPT], qz[PPT], best[PPT];
    int besti[PPT];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
      const int j = j0 + q < s1 ? j0 + q : s1 - 1;
      qx[q] = scan[(size_t)j * 3 + 0];
      qy[q] = scan[(size_t)j * 3 + 1];
      qz[q] = scan[(size_t)j * 3 + 2];
      best[q] = 0.f;
      besti[q] = 0;
    }
    for (int k0 = 0; k0 < m; k0 += TILE_PTS) {
      const int cnt = m - k0 < TILE_PTS ? m - k0 : TILE_PTS;
      __syncthreads();
      for (int k = t; k < cnt; k += WG) s_pt[k] = pose_point(po + (size_t)(k0 + k) * 3, c, s, cx, cy, cz);
      __syncthreads();
      for (int k = 0; k < cnt; ++k) {
        const f32x4 pt = s_pt[k];
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
          const float x2 = pt[0] - qx[q], y2 = pt[1] - qy[q], z2 = pt[2] - qz[q];
          const float d = x2 * x2 + y2 * y2 + z2 * z2;
          if ((k0 + k) == 0 || d < best[q]) {
            best[q] = d;
            besti[q] = k0 + k;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < PPT; ++q)
      if (j0 + q < s1) {
        const f32x4 nn = pose_point(po + (size_t)besti[q] * 3, c, s, cx, cy, cz);      // the bits that were staged
        const float rx = nn[0] - qx[q], ry = nn[1] - qy[q], rz = nn[2] - qz[q];
        const float ax = nn[0] - cx, ay = nn[1] - cy;
        acc[0] += (double)best[q];
        acc[1] += 2.0 * (double)rx;
        acc[2] += 2.0 * (double)ry;
        acc[3] += 2.0 * (double)rz;
        acc[4] += 2.0 * ((double)rx * -(double)ay + (double)ry * (double)ax);
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TERMS; ++i) s_red[i][t] = acc[i];
  __syncthreads();
  for (int d = WG / 2; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int i = 0; i < TERMS; ++i) s_red[i][t] += s_red[i][t + d];
    }
    __syncthreads();
  }
  if (t < TERMS) partial[(size_t)tile * TERMS + t] = s_red[t][0];
}

struct AdamStep {
  float w1, b2, w2, eps;       // 1 - beta1, beta2, 1 - beta2, eps as fp32
  float c2, neg_step;          // sqrt(1 - beta2^t) and -lr / (1 - beta1^t) of this step, rounded from double
};

__global__ __launch_bounds__(WG) void fit_update_kernel(int P, int n_tiles, int it, double loss_scale, AdamStep a,
                                                        const int *__restrict__ tile_obj,
                                                        const double *__restrict__ partial, double *__restrict__ obj_loss,
                                                        float *__restrict__ mom1, float *__restrict__ mom2,
                                                        float *__restrict__ params, float *__restrict__ best_params,
                                                        float *__restrict__ best_loss, int *__restrict__ best_iter,
                                                        float *__restrict__ hist_loss, float *__restrict__ hist_params) {
  __shared__ int s_better;
  const int t = threadIdx.x;
  // per object: its tiles' partial sums in ascending tile order
  for (int p = t; p < P; p += WG) {
    double sum[TERMS];
#pragma unroll
    for (int i = 0; i < TERMS; ++i) sum[i] = 0.0;
    for (int k = 0; k < n_tiles; ++k)
      if (clampi(tile_obj[k], 0, P - 1) == p) {
#pragma unroll
        for (int i = 0; i < TERMS; ++i) sum[i] += partial[(size_t)k * TERMS + i];
      }
    obj_loss[p] = sum[0];
    float g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = (float)(sum[1 + i] * loss_scale);
    if (hist_params != nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) hist_params[((size_t)it * P + p) * 4 + i] = params[4 * p + i];
    }
    // Adam's two moments now; the parameters move below, after the best ones were copied
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m1 = it == 0 ? 0.f : mom1[4 * p + i], m2 = it == 0 ? 0.f : mom2[4 * p + i];
      m1 = __builtin_fmaf(a.w1, g[i] - m1, m1);
      m2 = m2 * a.b2;
      m2 = __builtin_fmaf(a.w2 * g[i], g[i], m2);
      mom1[4 * p + i] = m1;
      mom2[4 * p + i] = m2;
    }
  }
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int p = 0; p < P; ++p) total += obj_loss[p];
    const float loss = (float)(total * loss_scale);
    const float before = it == 0 ? 1e6f : best_loss[0];
    const int better = loss < before;
    if (better) {
      best_loss[0] = loss;
      best_iter[0] = it;
    } else if (it == 0) {                  // nothing was below the start value: still defined
      best_loss[0] = before;
      best_iter[0] = -1;
    }
    if (hist_loss != nullptr) hist_loss[it] = loss;
    s_better = better;
  }
  __syncthreads();
  const int better = s_better;
  for (int p = t; p < P; p += WG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float cur = params[4 * p + i];
      if (better || it == 0) best_params[4 * p + i] = cur;
      const float m1 = mom1[4 * p + i], m2 = mom2[4 * p + i];
      const float den = sqrtf(m2) / a.c2 + a.eps;
      params[4 * p + i] = cur + (a.neg_step * m1) / den;
    }
  }
}

}  // namespace

RFD_API size_t rfd_fit_pose_workspace_bytes(int P, int n_tiles) {
  if (P <= 0 || n_tiles <= 0) return 0;
  return sizeof(double) * ((size_t)n_tiles * TERMS + (size_t)P) + sizeof(float) * 8 * (size_t)P;
}

RFD_API int rfd_fit_pose_run(int P, int n_obj, int n_scan, int n_tiles, int points_per_thread, int iterations, double lr,
                             double loss_scale, const float *obj, const int *obj_off, const float *scan,
                             const int *scan_off, const int *tile_obj, const int *tile_start, float *params,
                             float *best_params, float *best_loss, int *best_iter, float *hist_loss, float *hist_params,
                             void *workspace, void *stream) {
  if (P <= 0 || n_tiles <= 0) return 0;
  if (n_obj < 1 || n_scan < 1) return rfd_invalid("rfd_fit_pose_run: n_obj, n_scan >= 1");
  if (points_per_thread != 1 && points_per_thread != 4) return rfd_invalid("rfd_fit_pose_run: points_per_thread is 1 or 4");
  if (iterations < 1 || iterations > MAX_ITERATIONS) return rfd_invalid("rfd_fit_pose_run: 1 <= iterations <= 100000");
  if (!(lr > 0.0) || !isfinite(lr) || !isfinite(loss_scale)) return rfd_invalid("rfd_fit_pose_run: lr > 0, finite scales");
  if (!obj || !obj_off || !scan || !scan_off || !tile_obj || !tile_start || !params || !best_params || !best_loss ||
      !best_iter || !workspace)
    return rfd_invalid("rfd_fit_pose_run: a required array is missing");
  if ((hist_loss == nullptr) != (hist_params == nullptr))
    return rfd_invalid("rfd_fit_pose_run: hist_loss and hist_params go together");
  if (((uintptr_t)workspace & 7) != 0) return rfd_invalid("rfd_fit_pose_run: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double *partial = (double *)workspace;
  double *obj_loss = partial + (size_t)n_tiles * TERMS;
  float *mom1 = (float *)(obj_loss + P);
  float *mom2 = mom1 + (size_t)P * 4;
  const double beta1 = 0.9, beta2 = 0.999;
  AdamStep a;
  a.w1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.w2 = (float)(1.0 - beta2), a.eps = (float)1e-8;
  for (int it = 0; it < iterations; ++it) {
    // torch/optim/adam.py, single tensor: bias_correction = 1 - beta ** step, step_size = lr / bias_correction1,
    // bias_correction2 ** 0.5 -- Python floats, i.e. pow() in double
    const double bc1 = 1.0 - pow(beta1, (double)(it + 1)), bc2 = 1.0 - pow(beta2, (double)(it + 1));
    a.c2 = (float)pow(bc2, 0.5);
    a.neg_step = (float)(-(lr / bc1));
    if (points_per_thread == 1)
      hipLaunchKernelGGL(fit_nn_kernel<1>, dim3(n_tiles), dim3(WG), 0, s, P, n_obj, n_scan, obj, obj_off, scan, scan_off,
                         tile_obj, tile_start, params, partial);
    else
      hipLaunchKernelGGL(fit_nn_kernel<4>, dim3(n_tiles), dim3(WG), 0, s, P, n_obj, n_scan, obj, obj_off, scan, scan_off,
                         tile_obj, tile_start, params, partial);
    hipLaunchKernelGGL(fit_update_kernel, dim3(1), dim3(WG), 0, s, P, n_tiles, it, loss_scale, a, tile_obj, partial,
                       obj_loss, mom1, mom2, params, best_params, best_loss, best_iter, hist_loss, hist_params);
  }
  RFD_CHECK_LAUNCH();
  return 0;
}
