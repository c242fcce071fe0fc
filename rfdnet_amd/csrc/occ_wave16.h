// occ_wave16.h -- what the one-wave, 16-point decoder kernels share: occ_decode_tail_kernel (occ_decoder_tail.hip) and both
// halves of occ_normals_kernel (occ_normals.hip).  One wave, 16x16x32 MFMAs over f16 (hi, lo) splits, no LDS, no barrier: the
// weight fragments come straight from L2 through a ring of register sets, DEPTH k-steps ahead.
//
// Here: the matrix instructions of one k-step (mma3) and the fragment ring (FragRing).  NOT here, although the two kernels
// spell them alike: fc_p, the activation of a k-step, the block walk and fc_out.  Both kernels' instruction streams are
// frozen, and hipcc optimises a helper on its own before it inlines it: fc_p's address arithmetic then folds differently,
// the walk gets another register assignment, and occ_normals.hip's activation converts through split2 (sign mask) where the
// tail's values are known non-negative.  tests/test_gpu_decoder.py and tests/test_gpu_normals.py hold those texts together.
//
// Everything is __forceinline__, as in split_f16.h: each kernel compiles to the instruction stream it had with its own
// copy of this text.
#pragma once
#include "split_f16.h"
#include "../../include/rfd_occ.h"

namespace occ_wave16 {

using namespace split_f16;

constexpr int H = RFD_OCC_HIDDEN;
constexpr int NB = RFD_OCC_BLOCKS;
constexpr int HALF_FRAGS = 32;                 // fragments (1 KiB each) per half of a packed stream

// ---- one k-step's product on two channel tiles: three terms (X3) or the hi term alone
template <bool X3>
__device__ __forceinline__ void mma3(f32x4 &a0, f32x4 &a1, const Frag4 &f, const half8 &xh, const half8 &xl) {
  a0 = mfma16(f.h0, xh, a0);
  a1 = mfma16(f.h1, xh, a1);
  if (X3) {
    a0 = mfma16(f.h0, xl, a0);
    a1 = mfma16(f.h1, xl, a1);
    a0 = mfma16(f.l0, xh, a0);
    a1 = mfma16(f.l1, xh, a1);
  }
}

// ---- the weight stream, DEPTH k-steps ahead.  Every stage of the walk is eight k-steps of ONE half and DEPTH < 8, so step
// k of a stage fetches step k + DEPTH of the same half or step k + DEPTH - 8 of the next stage's half; the rotation (set =
// step mod SETS, 8 mod SETS = 0) carries over stage boundaries and loop iterations.  Fragment f of half h is
// (packed + lane)[(h * 32 + f) * 64]; `lane` is the part of that offset which the half pointers given to prime / fetch do not
// contain yet: the lane (wave-uniform half pointers, the offset added last: occ_normals.hip) or 0 (half pointers into the
// lane's own slots: occ_decoder_tail.hip).  Each kernel keeps the form its stream was frozen with.
template <int DEPTH, int SETS>
struct FragRing {
  static_assert(SETS > DEPTH && DEPTH < 8 && 8 % SETS == 0, "fragment-set rotation");
  Frag4 fs[SETS];
  int lane;

  // k-step ks of a half: fragments 4 ks .. 4 ks + 3, 4 KiB in one piece
  __device__ __forceinline__ void frag_issue(Frag4 &d, const half8 *half_base, int ks) {
    const half8 *w = half_base + ks * 256 + lane;
    d.h0 = w[0];
    d.l0 = w[64];
    d.h1 = w[128];
    d.l1 = w[192];
  }
  // the first DEPTH k-steps of the first half
  __device__ __forceinline__ void prime(const half8 *h0) {
    static_for<0, DEPTH>([&](auto kc) { frag_issue(fs[decltype(kc)::value], h0, decltype(kc)::value); });
  }
  // at step ks of the stage on `cur`, `next` being the half of the stage after it
  template <int ks>
  __device__ __forceinline__ void fetch(const half8 *cur, const half8 *next) {
    __builtin_amdgcn_sched_barrier(0);           // a k-step's fetch and its matrix instructions stay one unit: the loads of step
                                                 // k + DEPTH go out before step k's first MFMA, the only wait is for step k's set
    if constexpr (ks + DEPTH < 8) frag_issue(fs[(ks + DEPTH) % SETS], cur, ks + DEPTH);
    else frag_issue(fs[(ks + DEPTH) % SETS], next, ks + DEPTH - 8);
  }
};

}  // namespace occ_wave16
