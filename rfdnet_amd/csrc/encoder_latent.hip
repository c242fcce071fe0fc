// encoder_latent.hip -- the completion loss of the test mode (include/rfd_latent.h): the latent encoder q(z | p, occ, c)
// (models/iscnet/modules/encoder_latent.py:49-73), z = rsample(), KL(q || N(0, 1)), the row sums of
// binary_cross_entropy_with_logits and the voxel IoU counts (occupancy_net.py:59-109, network.py:144-148).
//
//   net1 = fc_1(relu(fc_0(occ) + fc_pos(p) + fc_c(c)))                  (K, T, 128)
//   net2 = fc_2(relu([net1 | max_T net1])) = W2[:, :128] relu(net1) + (W2[:, 128:] relu(max_T net1) + b2)
//   net3 = fc_3(relu([net2 | max_T net2]))   likewise
//   mean, logstd = fc_mean(max_T net3), fc_logstd(max_T net3)
//
// The pooled half of each concatenation is a bias vector per proposal (built in the stage's prologue, f64 sum in a
// fixed order); a point's input is 16 bytes, so stage s recomputes stages 1 .. s-1 in registers and nothing of width
// (K, T, *) is ever stored.  The layers are sa_fused.hip's pipeline (f32_wave32.h): a wave owns 32 points, D[channel,
// point] = W[channel, k] x[k, point] with the exact-fp32 v_mfma_f32_32x32x2_f32, the accumulator layout of a layer is
// the B layout of the next one and the 128 x 128 weights are staged per layer in LDS -- here in two buffers, so the
// next layer's copy is issued in front of this layer's products.  The 132 KiB of LDS
// also keep a CU to one workgroup, i.e. one wave per SIMD: the VALU first layer consumes LDS reads in front of MFMA
// code, the shape that must not run beside a partner wave's MFMAs (tests/test_isa_audit.py).
// The max over a proposal's points: lane shuffles, then LDS, then one integer atomic per channel and workgroup on the
// (K, 128) row (atomic_max_float, common.h) -- exact, hence independent of order and grid.
#include "f32_wave32.h"
#include "../../include/rfd_latent.h"

namespace {

using namespace f32_wave32;

constexpr int LH = 128;                    // hidden width
constexpr int LW = LH * LH;                // floats of one packed layer (64 KiB)

// s_bias[c] = b[c] + sum_k wT[k][c] relu(pooled[k]): two halves of k in f64, added in a fixed order, rounded once.
// All 256 threads call it; s_m / s_part are scratch; ends with a barrier.
__device__ __forceinline__ void pooled_bias(const float *__restrict__ wT, const float *__restrict__ b,
                                            const float *__restrict__ pooled, float *s_m, double *s_part,
                                            float *s_bias, int t) {
  if (t < LH) {
    const float m = pooled[t];
    s_m[t] = m > 0.f ? m : 0.f;
  }
  __syncthreads();
  const int c = t & (LH - 1), k0 = (t >> 7) * (LH / 2);
  double s = 0.0;
  for (int k = k0; k < k0 + LH / 2; ++k) s = __builtin_fma((double)wT[k * LH + c], (double)s_m[k], s);
  s_part[t] = s;
  __syncthreads();
  if (t < LH) s_bias[t] = (float)(s_part[t] + s_part[t + LH] + (double)b[t]);
  __syncthreads();
}

template <int STAGE>
__global__ __launch_bounds__(256) void latent_stage_kernel(
    int K, int T, int tiles, const float *__restrict__ p, const float *__restrict__ occ, const float *__restrict__ l0,
    const float *__restrict__ bias0, const float *__restrict__ wa, const float *__restrict__ wbT,
    const float *__restrict__ b123, float *__restrict__ pool) {
  __shared__ __attribute__((aligned(16))) float s_w[2][LW];
  __shared__ __attribute__((aligned(16))) f32x4 s_l0[LH];
  __shared__ __attribute__((aligned(16))) float s_b0[LH];
  __shared__ __attribute__((aligned(16))) float s_bias[3][LH];
  __shared__ float s_m[LH], s_pool[LH];
  __shared__ double s_part[2 * LH];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int half = lane >> 5, nrow = lane & 31;
  const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
  const int row = (tile * 4 + wave) * 32 + nrow;            // may run past the end
  const bool live = row < T;

  stage(s_w[0], wa, LW, t);
  if (STAGE >= 2) stage(s_w[1], wa + LW, LW, t);
  if (t < LH) {
    s_l0[t] = reinterpret_cast<const f32x4 *>(l0)[t];
    s_b0[t] = bias0[(size_t)k * LH + t];
    s_bias[0][t] = b123[t];
    s_pool[t] = -__builtin_inff();
  }
  if (STAGE >= 2) pooled_bias(wbT, b123 + LH, pool + (size_t)k * LH, s_m, s_part, s_bias[1], t);
  if (STAGE >= 3) pooled_bias(wbT + LW, b123 + 2 * LH, pool + ((size_t)K + k) * LH, s_m, s_part, s_bias[2], t);
  __syncthreads();

  // ---- the first layer on the VALU: channel at position 2j + half of this lane's point
  float bin[LH / 2];
  {
    const size_t pi = (size_t)k * T + (live ? row : 0);
    const float px = p[pi * 3], py = p[pi * 3 + 1], pz = p[pi * 3 + 2], po = occ[pi];
#pragma unroll
    for (int j = 0; j < LH / 2; ++j) {
      const f32x4 w = s_l0[2 * j + half];
      float v = __builtin_fmaf(w[3], po, s_b0[2 * j + half]);
      v = __builtin_fmaf(w[0], px, v);
      v = __builtin_fmaf(w[1], py, v);
      v = __builtin_fmaf(w[2], pz, v);
      bin[j] = v > 0.f ? v : 0.f;
    }
  }
  f32x16 acc[4];
  layer<LH / 2, 4>(s_w[0], bin, acc, lane);
  add_bias<false>(acc, s_bias[0], half);
  if (STAGE >= 2) {
    __syncthreads();                                      // every wave is done with buffer 0
    if (STAGE >= 3) stage(s_w[0], wa + 2 * LW, LW, t);
    acc_to_b<true>(acc, bin);
    layer<LH / 2, 4>(s_w[1], bin, acc, lane);
    add_bias<false>(acc, s_bias[1], half);
  }
  if (STAGE >= 3) {
    __syncthreads();                                      // fc_3's fragments have landed
    acc_to_b<true>(acc, bin);
    layer<LH / 2, 4>(s_w[0], bin, acc, lane);
    add_bias<false>(acc, s_bias[2], half);
  }

  // ---- max over the live points: the 32 lanes of a half, then LDS, then the proposal's row
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = live ? acc[b][r] : -__builtin_inff();
      for (int d = 1; d < 32; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
      acc[b][r] = v;
    }
  if (nrow == 0) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) atomic_max_float(s_pool + 32 * b + 8 * (r >> 2) + 4 * half + (r & 3), acc[b][r]);
  }
  __syncthreads();
  if (t < LH) atomic_max_float(pool + ((size_t)(STAGE - 1) * K + k) * LH + t, s_pool[t]);
}

// bias0[k] = b0 + c[k] . wcT (two halves of c_dim in f64, fixed order); pool = -inf.  One workgroup per proposal.
__global__ __launch_bounds__(256) void latent_prep_kernel(int K, int c_dim, const float *__restrict__ c,
                                                          const float *__restrict__ wcT, const float *__restrict__ b0,
                                                          float *__restrict__ bias0, float *__restrict__ pool) {
  __shared__ double s_part[2 * LH];
  const int t = threadIdx.x, k = blockIdx.x;
  const int ch = t & (LH - 1), part = t >> 7;
  const int per = (c_dim + 1) / 2;
  const int lo = part * per, hi = lo + per < c_dim ? lo + per : c_dim;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s = __builtin_fma((double)wcT[(size_t)i * LH + ch], (double)c[(size_t)k * c_dim + i], s);
  s_part[t] = s;
  __syncthreads();
  if (t < LH) bias0[(size_t)k * LH + t] = (float)(s_part[t] + s_part[t + LH] + (double)b0[t]);
  for (int i = t; i < 3 * LH; i += 256) pool[((size_t)(i / LH) * K + k) * LH + (i % LH)] = -__builtin_inff();
}

// One workgroup per proposal: output o < z_dim is mean[o], o >= z_dim is logstd[o - z_dim].
__global__ __launch_bounds__(256) void latent_head_kernel(int z_dim, const float *__restrict__ pool3,
                                                          const float *__restrict__ whT, const float *__restrict__ bh,
                                                          const float *__restrict__ eps, float *__restrict__ mean,
                                                          float *__restrict__ logstd, float *__restrict__ z,
                                                          float *__restrict__ kl) {
  __shared__ float s_m[LH];
  __shared__ float s_out[1024];
  __shared__ double s_kl[256];
  const int t = threadIdx.x, k = blockIdx.x;
  if (t < LH) s_m[t] = pool3[(size_t)k * LH + t];
  __syncthreads();
  for (int o = t; o < 2 * z_dim; o += 256) {
    double s = (double)bh[o];
    for (int i = 0; i < LH; ++i) s = __builtin_fma((double)whT[(size_t)i * 2 * z_dim + o], (double)s_m[i], s);
    const float v = (float)s;
    s_out[o] = v;
    if (o < z_dim) mean[(size_t)k * z_dim + o] = v;
    else logstd[(size_t)k * z_dim + o - z_dim] = v;
  }
  __syncthreads();
  double term = 0.0;
  for (int j = t; j < z_dim; j += 256) {
    const float m = s_out[j], ls = s_out[z_dim + j];
    if (z != nullptr) {
      const float sd = expf(ls);
      const float es = eps[(size_t)k * z_dim + j] * sd;
      z[(size_t)k * z_dim + j] = m + es;
    }
    term += 0.5 * (exp(2.0 * (double)ls) + (double)m * (double)m - 1.0) - (double)ls;
  }
  s_kl[t] = term;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d) s_kl[t] += s_kl[t + d];
    __syncthreads();
  }
  if (t == 0 && kl != nullptr) kl[k] = (float)s_kl[0];
}

// One workgroup per row: thread t sums elements t, t + 256, ... in f64, then a fixed tree.
__global__ __launch_bounds__(256) void bce_rowsum_kernel(int T, const float *__restrict__ logits, int ld_logits,
                                                         const float *__restrict__ target, int ld_target,
                                                         float *__restrict__ out) {
  __shared__ double s_sum[256];
  const int t = threadIdx.x, k = blockIdx.x;
  const float *x = logits + (size_t)k * ld_logits, *y = target + (size_t)k * ld_target;
  double s = 0.0;
  for (int i = t; i < T; i += 256) {
    const float xi = x[i];
    const float xy = xi * y[i];
    const float pos = xi > 0.f ? xi : 0.f;
    const float sp = log1pf(expf(-fabsf(xi)));
    const float term = (pos - xy) + sp;
    s += (double)term;
  }
  s_sum[t] = s;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d) s_sum[t] += s_sum[t + d];
    __syncthreads();
  }
  if (t == 0) out[k] = (float)s_sum[0];
}

// One workgroup per proposal: a wave counts 64 voxels per step with two ballots.
__global__ __launch_bounds__(256) void voxel_iou_kernel(int V, const float *__restrict__ logits, int ld_logits,
                                                        float thr, const float *__restrict__ gt,
                                                        int *__restrict__ inter, int *__restrict__ uni) {
  __shared__ int s_cnt[8];
  const int t = threadIdx.x, k = blockIdx.x, wave = t >> 6;
  int ni = 0, nu = 0;                                          // wave-uniform
  for (int v0 = 0; v0 < V; v0 += 256) {
    const int v = v0 + t;
    const bool in = v < V;
    const bool pred = in && logits[(size_t)k * ld_logits + v] >= thr;
    const bool g = in && gt[(size_t)k * V + v] >= 0.5f;
    ni += __popcll(__ballot(pred && g));
    nu += __popcll(__ballot(pred || g));
  }
  if ((t & 63) == 0) {
    s_cnt[wave] = ni;
    s_cnt[4 + wave] = nu;
  }
  __syncthreads();
  if (t == 0) {
    inter[k] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    uni[k] = s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7];
  }
}

}  // namespace

RFD_API int rfd_latent_prep(int K, int c_dim, const float *c, const float *wcT, const float *b0, float *bias0,
                            float *pool, void *stream) {
  if (K <= 0) return 0;
  if (c_dim < 0 || (c_dim > 0 && (c == nullptr || wcT == nullptr))) return rfd_invalid("rfd_latent_prep: c_dim / c / wcT");
  hipLaunchKernelGGL(latent_prep_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, K, c_dim, c, wcT, b0, bias0, pool);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_latent_stage(int stage, int K, int T, const float *p, const float *occ, const float *l0,
                             const float *bias0, const float *wa, const float *wbT, const float *b123, float *pool,
                             void *stream) {
  if (K <= 0) return 0;
  if (T <= 0) return rfd_invalid("rfd_latent_stage: T >= 1 (the max over no points is undefined)");
  const int tiles = (T + 127) / 128;
  if ((long long)tiles * K > 0x7fffffffLL) return rfd_invalid("rfd_latent_stage: K * ceil(T / 128) must fit in 31 bits");
  if (((uintptr_t)l0 & 15) || ((uintptr_t)wa & 15)) return rfd_invalid("rfd_latent_stage: 16-byte aligned l0 / wa");
  const dim3 grid((unsigned)(tiles * K));
  hipStream_t s = (hipStream_t)stream;
#define RFD_LATENT_CASE(S)                                                                                        \
  if (stage == S) {                                                                                               \
    hipLaunchKernelGGL((latent_stage_kernel<S>), grid, dim3(256), 0, s, K, T, tiles, p, occ, l0, bias0, wa, wbT, \
                       b123, pool);                                                                               \
    RFD_CHECK_LAUNCH();                                                                                           \
    return 0;                                                                                                     \
  }
  RFD_LATENT_CASE(1)
  RFD_LATENT_CASE(2)
  RFD_LATENT_CASE(3)
#undef RFD_LATENT_CASE
  return rfd_invalid("rfd_latent_stage: stage must be 1, 2 or 3");
}

RFD_API int rfd_latent_head(int K, int z_dim, const float *pool3, const float *whT, const float *bh, const float *eps,
                            float *mean, float *logstd, float *z, float *kl, void *stream) {
  if (K <= 0) return 0;
  if (z_dim < 1 || z_dim > 512) return rfd_invalid("rfd_latent_head: 1 <= z_dim <= 512");
  if (z != nullptr && eps == nullptr) return rfd_invalid("rfd_latent_head: z needs eps");
  hipLaunchKernelGGL(latent_head_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, z_dim, pool3, whT, bh, eps, mean,
                     logstd, z, kl);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_bce_logits_rowsum(int K, int T, const float *logits, int ld_logits, const float *target, int ld_target,
                                  float *out, void *stream) {
  if (K <= 0) return 0;
  if (T < 0 || ld_logits < T || ld_target < T) return rfd_invalid("rfd_bce_logits_rowsum: row strides must cover T");
  hipLaunchKernelGGL(bce_rowsum_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, T, logits, ld_logits, target,
                     ld_target, out);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_voxel_iou(int K, int V, const float *logits, int ld_logits, float logit_threshold, const float *gt,
                          int *inter, int *uni, void *stream) {
  if (K <= 0) return 0;
  if (V < 0 || ld_logits < V) return rfd_invalid("rfd_voxel_iou: the row stride must cover V");
  hipLaunchKernelGGL(voxel_iou_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, V, logits, ld_logits,
                     logit_threshold, gt, inter, uni);
  RFD_CHECK_LAUNCH();
  return 0;
}
