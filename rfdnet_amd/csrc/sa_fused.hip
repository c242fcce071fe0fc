// sa_fused.hip -- one set-abstraction layer after the ball query, fused:
//   group -> centre-subtract / normalise -> concat -> 3 x [1x1 conv + BN(eval) + ReLU]
//   -> max over the nsample neighbours, never materialising the (C, M, nsample) tensor.
//
// Replaces PointnetSAModuleVotes.forward after its grouper's ball query
// (external/pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py:219-255, QueryAndGroup
// pointnet2_utils.py:333-344, build_shared_mlp :9-19) at inference.
//
// A wave owns 32 rows = (centre, neighbour) pairs.  D[channel, row] = W[channel, k] x[k, row]
// with the exact-fp32 v_mfma_f32_32x32x2_f32 (no split precision: 10 GFLOP per scene):
// A = weights (fragment-ordered, staged per layer in LDS), B = activations held in registers.
// The accumulator layout of a layer is the B layout of the next one (lane (row, h) holds
// channels 8q + 4h + e of each 32-channel block; the host packs the next layer's k-order as
// that delivery order), so bias + ReLU are applied in place and the activations never leave
// the lane.  The last layer is reduced over the rows of a centre with lane shuffles.
// BatchNorm (eval) is folded into W and the bias on the host.  The layer pipeline and the packed-weight layout:
// f32_wave32.h.
#include "f32_wave32.h"
#include "../../include/rfd_pointnet2.h"

namespace {

using namespace f32_wave32;

constexpr int SA_LDS_FLOATS = 36 * 1024;   // 144 KiB: the largest packed layer (128 x 264)

template <int KJ1, int C1, int C2, int C3>
__global__ __launch_bounds__(256) void sa_fused_kernel(
    int n, int m, int ns, int c_feat, float inv_radius, const float *__restrict__ xyz,
    const float *__restrict__ new_xyz, const float *__restrict__ features, const int *__restrict__ idx,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
    const float *__restrict__ b2, const float *__restrict__ w3, const float *__restrict__ b3,
    float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_w[SA_LDS_FLOATS];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int half = lane >> 5, nrow = lane & 31;
  const int bi = blockIdx.y;
  const int rows = m * ns;
  const int row = (blockIdx.x * 4 + wave) * 32 + nrow;          // (centre, neighbour), may run past the end
  const bool live = row < rows;
  const int centre = live ? row / ns : 0;

  // ---- layer-1 input, channel c = 2j + kh of this lane's row: (xyz[idx] - centre) [/ r], features
  float bin1[KJ1];
  {
    const int pi = live ? idx[((size_t)bi * m + centre) * ns + (row - centre * ns)] : 0;
    const float *px = xyz + ((size_t)bi * n + pi) * 3;
    const float *pc = new_xyz + ((size_t)bi * m + centre) * 3;
#pragma unroll
    for (int j = 0; j < KJ1; ++j) {
      const int c = 2 * j + half;
      float v = 0.f;
      if (c < 3) v = (px[c] - pc[c]) * inv_radius;
      else if (c - 3 < c_feat) v = features[((size_t)bi * c_feat + (c - 3)) * n + pi];
      bin1[j] = v;
    }
  }
  stage(s_w, w1, C1 * KJ1 * 2, t);
  __syncthreads();
  f32x16 a1[C1 / 32];
  layer<KJ1, C1 / 32>(s_w, bin1, a1, lane);
  add_bias<true, C1 / 32>(a1, b1, half);
  __syncthreads();

  stage(s_w, w2, C2 * C1, t);
  __syncthreads();
  float bin2[C1 / 2];                                   // spelled out, not acc_to_b<false>: see f32_wave32.h
#pragma unroll
  for (int j = 0; j < C1 / 2; ++j) bin2[j] = a1[j >> 4][j & 15];
  f32x16 a2[C2 / 32];
  layer<C1 / 2, C2 / 32>(s_w, bin2, a2, lane);
  add_bias<true, C2 / 32>(a2, b2, half);
  __syncthreads();

  stage(s_w, w3, C3 * C2, t);
  __syncthreads();
  float bin3[C2 / 2];
#pragma unroll
  for (int j = 0; j < C2 / 2; ++j) bin3[j] = a2[j >> 4][j & 15];
  f32x16 a3[C3 / 32];
  layer<C2 / 2, C3 / 32>(s_w, bin3, a3, lane);
  add_bias<true, C3 / 32>(a3, b3, half);
  __syncthreads();

  // ---- max over the neighbours of a centre: lanes nrow..nrow+ns-1 of the same half (post-ReLU
  // values are >= 0, so dead rows contribute 0 safely only if they are excluded: mask them)
  float *s_part = s_w;                                  // [wave][half][C3 / 2 channel slots] for ns = 64
  const int span = ns < 32 ? ns : 32;
#pragma unroll
  for (int b = 0; b < C3 / 32; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = live ? a3[b][r] : 0.f;
      for (int d = 1; d < span; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
      a3[b][r] = v;
    }
  if (ns == 64) {       // a centre spans two waves (2w, 2w+1): combine through LDS
    if (nrow == 0) {
#pragma unroll
      for (int b = 0; b < C3 / 32; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) s_part[(wave * 2 + half) * (C3 / 2) + 16 * b + r] = a3[b][r];
    }
    __syncthreads();
    if (nrow == 0 && !(wave & 1) && live) {
#pragma unroll
      for (int b = 0; b < C3 / 32; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = fmaxf(a3[b][r], s_part[((wave + 1) * 2 + half) * (C3 / 2) + 16 * b + r]);
          const int ch = 32 * b + 8 * (r >> 2) + 4 * half + (r & 3);
          out[((size_t)bi * C3 + ch) * m + centre] = v;
        }
    }
  } else if (live && (nrow % ns) == 0) {
#pragma unroll
    for (int b = 0; b < C3 / 32; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = 32 * b + 8 * (r >> 2) + 4 * half + (r & 3);
        out[((size_t)bi * C3 + ch) * m + centre] = a3[b][r];
      }
  }
}

}  // namespace

RFD_API int rfd_sa_fused(int b, int n, int m, int nsample, int c_feat, float radius, int normalize_xyz,
                         const float *xyz, const float *new_xyz, const float *features, const int *idx,
                         int c1, int c2, int c3, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *w3, const float *b3, float *out, void *stream) {
  if (b <= 0 || m <= 0) return 0;
  const int cin = 3 + c_feat;
  const int kj1 = ((cin + 7) / 8) * 4;        // k-steps of layer 1: channel pairs, padded to 4
  if (!(nsample == 16 || nsample == 32 || nsample == 64)) {
    return rfd_invalid("rfd_sa_fused: nsample must be 16, 32 or 64");
  }
  const float inv_r = normalize_xyz ? 1.0f / radius : 1.0f;
  const int rows = m * nsample;
  const dim3 grid((rows + 127) / 128, b);
  hipStream_t s = (hipStream_t)stream;
#define RFD_SA_CASE(KJ1, C1, C2, C3)                                                                    \
  if (kj1 == KJ1 && c1 == C1 && c2 == C2 && c3 == C3) {                                                 \
    hipLaunchKernelGGL((sa_fused_kernel<KJ1, C1, C2, C3>), grid, dim3(256), 0, s, n, m, nsample, c_feat, \
                       inv_r, xyz, new_xyz, features, idx, w1, b1, w2, b2, w3, b3, out);                 \
    RFD_CHECK_LAUNCH();                                                                                  \
    return 0;                                                                                            \
  }
  RFD_SA_CASE(4, 64, 64, 128)        // SA1: 3 + 1 inputs
  RFD_SA_CASE(68, 128, 128, 256)     // SA2: 3 + 128
  RFD_SA_CASE(132, 128, 128, 256)    // SA3, SA4: 3 + 256
  RFD_SA_CASE(132, 128, 128, 128)    // vote aggregation: 3 + 256
#undef RFD_SA_CASE
  return rfd_invalid("rfd_sa_fused: layer widths not instantiated");
}
