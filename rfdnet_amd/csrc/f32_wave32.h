// f32_wave32.h -- what the exact-fp32 matrix-core kernels share: sa_fused_kernel (sa_fused.hip) and latent_stage_kernel
// (encoder_latent.hip).  A wave owns 32 rows, D[channel, row] = W[channel, k] x[k, row] with v_mfma_f32_32x32x2_f32 (a k-ordered
// fmaf chain, no split precision): A = weights, fragment-ordered by the host and staged per layer in LDS, B = activations held
// in registers.  The accumulator layout of a layer is the B layout of the next one: lane (row, h) holds channels 8q + 4h + e of
// each 32-channel block in register 4q + e, so register r of block b is the next layer's B operand of k-step 16b + r and the
// activations never leave the lane.
//
// Packed layer layout (built by the host, rfdnet_amd/sa_fused.py::pack_layer): [C / 32][KJ / 4][64 lanes][4],
// element (b, j4, lane, e) = W'[32b + (lane & 31)][korder(4 j4 + e, lane >> 5)], W' = BN-folded weight.  The two k orders:
// of a first layer korder(j, kh) = 2j + kh (zero beyond the real input width), of a layer fed by accumulators
// korder(j, kh) = 32 (j >> 4) + 8 ((j & 15) >> 2) + 4 kh + (j & 3), the delivery order above.
//
// Here: the matrix instruction, one layer's product, the bias pass, the accumulator-to-operand copy and the copy of a packed
// layer to LDS.  NOT here: the kernels' prologues, pooling tails and launchers -- and sa_fused_kernel's own accumulator-to-operand
// loops, which stay spelled out there: through acc_to_b<false> its neighbour-max loop compiles to another compare-and-branch.
//
// Everything is __forceinline__, as in split_f16.h: each kernel compiles to the instruction stream it had with its own
// copy of this text.
#pragma once
#include "common.h"

namespace f32_wave32 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// One layer: acc[b] = sum_j W[32b.., korder(j, kh)] * bin[j]; packed W in LDS as
// [block b][j4 = j / 4][lane][4 floats].
template <int KJ, int NB>   // KJ = k-steps (pairs of input channels, multiple of 4), NB = 32-channel output blocks
__device__ __forceinline__ void layer(const float *s_w, const float (&bin)[KJ], f32x16 (&acc)[NB], int lane) {
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x16{0.f};
  const f32x4 *w = reinterpret_cast<const f32x4 *>(s_w) + lane;
#pragma unroll
  for (int j4 = 0; j4 < KJ / 4; ++j4) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x4 w4 = w[(b * (KJ / 4) + j4) * 64];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[b] = mfma32(w4[e], bin[4 * j4 + e], acc[b]);
    }
  }
}

// + bias [, ReLU] in place (bias in natural channel order, LDS or global memory)
template <bool RELU, int NB>
__device__ __forceinline__ void add_bias(f32x16 (&acc)[NB], const float *__restrict__ bias, int half) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 32 * b + 8 * q + 4 * half);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = acc[b][4 * q + e] + bv[e];
        acc[b][4 * q + e] = RELU ? (v > 0.f ? v : 0.f) : v;
      }
    }
}

// the next layer's B operand: [ReLU of] the accumulators, register r of block b = k-step 16b + r
template <bool RELU, int NB>
__device__ __forceinline__ void acc_to_b(const f32x16 (&acc)[NB], float (&bin)[16 * NB]) {
#pragma unroll
  for (int j = 0; j < 16 * NB; ++j) {
    const float v = acc[j >> 4][j & 15];
    bin[j] = RELU ? (v > 0.f ? v : 0.f) : v;
  }
}

// n_floats of a packed layer, global memory -> LDS; all 256 threads of the workgroup call it
__device__ __forceinline__ void stage(float *s_w, const float *__restrict__ g_w, int n_floats, int t) {
  const f32x4 *src = reinterpret_cast<const f32x4 *>(g_w);
  f32x4 *dst = reinterpret_cast<f32x4 *>(s_w);
  for (int i = t; i < n_floats / 4; i += 256) dst[i] = src[i];
}

}  // namespace f32_wave32
