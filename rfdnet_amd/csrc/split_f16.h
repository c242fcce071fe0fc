// split_f16.h -- the device primitives of the "split f16" matrix-core kernels (occ_decoder*.hip, occ_normals.hip,
// pointseg_chain.hip, gemm_f16x3.hip, pos_embed.hip), in ONE place.
//
// The scheme: a value, scaled by a power of two, is converted to f16 round-to-zero (hi); the remainder value - hi is
// exact in fp32 and is converted again (lo).  A product is three MFMAs (W_hi a_hi, W_hi a_lo, W_lo a_hi; fp32
// accumulation).  Round to zero saturates at 65504 instead of giving inf, so every kernel keeps a packed running maximum
// of its |hi| words and raises a bit of the device status word when a value has left the f16 range.
//
// Everything here is __forceinline__: a kernel that uses a helper compiles to the instruction stream it had with its
// own copy (tests/test_isa_audit.py pins occ_decoder8.hip's).  A source opens its anonymous namespace with
// `using namespace split_f16;`.  occ_wave16.h builds on this header: the k-step product and the weight-fragment ring of
// the one-wave decoder kernels (occ_decoder_tail.hip, occ_normals.hip).
#pragma once
#include <type_traits>

namespace split_f16 {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ f32x4 mfma16(half8 a, half8 b, f32x4 c) {         // v_mfma_f32_16x16x32_f16
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(half8 a, half8 b, f32x16 c) {       // v_mfma_f32_32x32x16_f16
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// ---- the range watch ------------------------------------------------------------------------------------------------
// running maximum of packed f16 pairs compared as u16: monotone for non-negative f16, so the sign bits must be clear
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// 0x7bff = 65504 = the largest finite f16: the round-to-zero conversion saturates there, so a |hi| word that large
// means a value left the f16 range -> `flag` of the status word (include/rfd_pointnet2.h: RFD_STATUS_DECODER_RANGE for
// decoder activations, RFD_STATUS_GEMM_RANGE for GEMM / chain operands)
__device__ __forceinline__ void flag_f16_range(unsigned amax16, unsigned *status, unsigned flag) {
  if ((amax16 & 0xffffu) >= 0x7bffu || (amax16 >> 16) >= 0x7bffu) atomicOr(status, flag);
}
// the same watch on a value a kernel STORES in fp32 for the next split-precision layer, which will scale it by
// `next_scale` (2^sa) before its own split: |v| 2^sa >= F16_MAX would saturate there silently
constexpr float F16_MAX = 65504.f;
__device__ __forceinline__ bool out_of_f16_range(float absmax, float next_scale) { return absmax * next_scale >= F16_MAX; }
__device__ __forceinline__ void flag_out_range(float absmax, float next_scale, unsigned *status, unsigned flag) {
  if (out_of_f16_range(absmax, next_scale)) atomicOr(status, flag);
}

// ---- the conversion -------------------------------------------------------------------------------------------------
// two scaled values -> packed f16 hi (round to zero) and lo words; amax16 sees |hi| (NONNEG: the values carry no sign
// bit, nothing to mask).  lo = a - (float)hi, exact: one v_fma_mix_f32 per value, reading the f16 halves in place.
template <bool WITH_LO, bool NONNEG>
__device__ __forceinline__ void split_pair(float a0, float a1, unsigned &hiw, unsigned &low, unsigned &amax16) {
  hiw = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a0, a1));
  amax16 = pk_max_u16(amax16, NONNEG ? hiw : hiw & 0x7fff7fffu);
  if (WITH_LO) {
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hiw), "v"(a0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hiw), "v"(a1));
    low = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
  } else {
    low = 0u;
  }
}
// two values of any sign
__device__ __forceinline__ void split2(float a0, float a1, unsigned &hiw, unsigned &low, unsigned &amax16) {
  split_pair<true, false>(a0, a1, hiw, low, amax16);
}
// relu(s x + t) of two values (!WITH_LO: the single-term mode, hi only)
template <bool WITH_LO>
__device__ __forceinline__ void act2(float x0, float x1, float s0, float s1, float t0, float t1, unsigned &hiw,
                                     unsigned &low, unsigned &amax16) {
  float a0 = __builtin_fmaf(s0, x0, t0), a1 = __builtin_fmaf(s1, x1, t1);
  a0 = a0 > 0.f ? a0 : 0.f;
  a1 = a1 > 0.f ? a1 : 0.f;
  split_pair<WITH_LO, true>(a0, a1, hiw, low, amax16);
}

// the hi or the lo f16 half of a scaled weight: the pack kernels split once, round to nearest
__host__ __device__ __forceinline__ _Float16 weight_half(float w, bool want_lo) {
  const _Float16 hi = (_Float16)w;
  const _Float16 lo = (_Float16)(w - (float)hi);
  return want_lo ? lo : hi;
}

// ---- operand streams of the 16x16x32 decoder kernels; the one-wave kernels' fragment ring is occ_wave16.h's -----------
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// the S / T values of one k-step's two channel tiles
struct ST {
  f32x4 s0, t0, s1, t1;
};
__device__ __forceinline__ void st_issue(ST &d, const float *S, const float *T, int ch) {
  d.s0 = *reinterpret_cast<const f32x4 *>(S + ch);
  d.t0 = *reinterpret_cast<const f32x4 *>(T + ch);
  d.s1 = *reinterpret_cast<const f32x4 *>(S + ch + 16);
  d.t1 = *reinterpret_cast<const f32x4 *>(T + ch + 16);
}

// the weight fragments of one k-step: (hi, lo) of two channel tiles
struct Frag4 {
  half8 h0, l0, h1, l1;
};

}  // namespace split_f16
