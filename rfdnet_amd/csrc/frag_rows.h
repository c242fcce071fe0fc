// frag_rows.h -- the "frag rows" layout of split activations (include/rfd_occ.h documents it, gemm_f16x3.hip's
// "Fragment-ordered split activations" says why), in ONE place: relu(x) 2^sa split into f16 (hi, lo) and stored in the
// order the consumer's v_mfma_f32_32x32x16_f16 wants its B operand.
//
//   block (rb, kb) = rows 32 rb .. +31, channels 32 kb .. +31 = FRAG_BLOCK_BYTES:
//     [kstep 2][split hi / lo][lane 64][8 f16]        = four runs of FRAG_RUN_BYTES, frag_run(kstep, lo)
//     row     = 32 rb + (lane & 31)
//     channel = 32 kb + frag_channel(kstep, lane >> 5, j)
//
// A buffer is [M / 32][row-block stride]; a column window is a block offset.  Producers: rows_to_frag_kernel,
// frag_epilogue (gemm_f16x3.hip), pos_embed_frag_kernel (pos_embed.hip); consumers: gemm_rowsf_kernel (whose W stream,
// layout 3 of rfd_gemm_pack_w, uses frag_channel for its k order) and frag_to_rows_kernel.
#pragma once
#include "split_f16.h"

namespace frag_rows {

using namespace split_f16;

constexpr int FRAG_RUN_BYTES = 1024;                      // 64 lanes x 8 f16: one operand fragment of a wave
constexpr int FRAG_BLOCK_BYTES = 4 * FRAG_RUN_BYTES;
// byte offset of a run in its block: k step 0 / 1, hi (0) or lo (1) halves
constexpr int frag_run(int kstep, int lo) { return (2 * kstep + lo) * FRAG_RUN_BYTES; }

// channel (0..31, within the block) of element j of lane (row, half)'s fragment of a k step: the ACCUMULATOR order of
// v_mfma_f32_32x32x16 (register r = 8 kstep + j of a lane), so a producer converts its accumulators in registers
__device__ __host__ __forceinline__ int frag_channel(int kstep, int half, int j) {
  const int r = 8 * kstep + j;
  return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// this lane's 16 bytes of run 0 of block (rb, kb)
template <class T>
__device__ __forceinline__ T *frag_block(T *base, int rb, long rb_stride, int kb, int lane) {
  return base + (size_t)rb * rb_stride + (size_t)kb * FRAG_BLOCK_BYTES + lane * 16;
}

// (hi, lo) words of two scaled values, the remainder by plain subtraction (v_cvt_f32_f16 + v_sub_f32) where
// split_f16.h's split2 issues one mixed-precision fma: same values, another instruction stream -- the GEMM kernels and
// pos_embed.hip's frag kernel keep the one they were measured and audited with
__device__ __forceinline__ void split2_sub(float a0, float a1, unsigned &hw, unsigned &lw) {
  const half2v h2 = __builtin_bit_cast(half2v, __builtin_amdgcn_cvt_pkrtz(a0, a1));
  const float r0 = a0 - (float)h2[0], r1 = a1 - (float)h2[1];
  hw = __builtin_bit_cast(unsigned, h2);
  lw = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
}

// one k step of a lane (4 hi words, 4 lo words) -> its two runs; d = frag_block(...)
__device__ __forceinline__ void frag_store_kstep(unsigned char *d, int kstep, const unsigned *hw, const unsigned *lw) {
  *reinterpret_cast<u32x4 *>(d + frag_run(kstep, 0)) = u32x4{hw[0], hw[1], hw[2], hw[3]};
  *reinterpret_cast<u32x4 *>(d + frag_run(kstep, 1)) = u32x4{lw[0], lw[1], lw[2], lw[3]};
}
// a lane's whole block (words 0-3: k step 0, 4-7: k step 1) -> four fully coalesced runs
__device__ __forceinline__ void frag_store(unsigned char *d, const unsigned (&hw)[8], const unsigned (&lw)[8]) {
  frag_store_kstep(d, 0, hw, lw);
  frag_store_kstep(d, 1, hw + 4, lw + 4);
}

}  // namespace frag_rows
