// occ_normals.hip -- vertex normals from the occupancy field's gradient (Generator3D.estimate_normals, generator.py:200-224):
// g = d logit_k(p) / d p in reverse mode, normals = -g / |g|, for all K meshes of a scene in one launch.
//
// Shape: the tail decoder's (occ_decoder_tail.hip) -- ONE wave per workgroup, 16 vertices, no LDS, no barrier, weight
// fragments straight from L2 one k-step ahead, 16x16x32 MFMAs on (hi, lo) f16 splits (three products per k-step, fp32
// accumulation).  The conversion, the range watch and the S / T fetch are split_f16.h's, the k-step product and the
// weight-fragment ring occ_wave16.h's, shared with that file.
//
// Forward pass: the decoder exactly as the tail kernel evaluates it (same table, same packed stream, same
// RFD_STATUS_DECODER_RANGE on an activation beyond the f16 range), but nothing is kept of it except the ReLU masks of its
// 11 CBN layers.  In the D layout a lane holds 64 channels of each layer, so a mask is 64 bits; bit 8 s + j belongs to
// the channel in slot j of k-step s's B
// fragment (channel 32 s + 16 (j >> 2) + 4 kg + (j & 3)) -- the same slot the backward pass reads it from.  The ten block masks
// travel through a register queue (shifted once per block: static indices, no scratch).
//
// Backward pass (unscaled quantities; S = the CBN scale per channel, m = the ReLU mask):
//   g = w_out . m_f . S_f;  for blocks 4 .. 0:  g_a1 = W1^T g,  g_h = S1 m1 g_a1,  g_a0 = W0^T g_h,  g += S0 m0 g_a0;
//   grad p = W_p^T g.
// The two 256x256 products per block are the forward pass's two GEMMs with transposed weights in reverse block order, so the
// same loop structure runs on a second packed stream: rfd_occ_pack_weights_w8(fc0' = W1^T, fc1' = W0^T, blocks reversed).  Its
// chunk (j, mb) = "W1^T rows of slab mb, then W0^T columns of slab mb" -- the order the backward block consumes them in, and
// the lane-local feedback of the D layout into the next B operand holds for any matrix.
// Scales: the table's S rows are pre-scaled by powers of two (occ_fold.py); S0 = S0' 2^kw1, S1 = S1' 2^kw0_i, S_f = S_f' 2^KH,
// and the packed backward weights carry 2^kb0_j / 2^kb1.  Every correction is a power of two folded into one multiplier per
// layer (exact).  The back-propagated vector is kept as g' = g 2^-X with a per-point exponent X: after the final layer and
// after every block the point's max |g'| over its 256 channels (4 lanes) is brought into [1, 2) by a power of two (exact), so
// the f16 (hi, lo) parts neither overflow nor lose the lo part to underflow; 2^X comes back in fp32 at the end (X starts at KH
// and fc_p_w = W_p 2^KH: the two cancel).  An f16 split beyond the range anyway (a gradient that grows by > 2^15 inside one
// block) raises RFD_STATUS_DECODER_RANGE like an activation.
// Outputs: normals[v] = -g / |g| (fp32); where g is exactly zero that is 0/0 = NaN, as in the reference (torch autograd's
// ni / torch.norm(ni)).  grad (optional) = g.
//
// Vertices are the marching-cubes f64 buffer (rfd_mc_emit_affine), rounded to fp32 on load like torch.FloatTensor(vertices).
// Groups of 16 vertices never span two meshes: gprefix[k] = first group of mesh k (K + 1 entries); a wave finds its mesh by
// binary search, the last group of a mesh is masked.
#include "common.h"
#include "occ_wave16.h"

namespace {

using namespace occ_wave16;

typedef unsigned long long u64;

constexpr int ROWS = RFD_OCC_TABLE_ROWS;
constexpr int DEPTH = 1;                       // k-steps of fragments in flight ahead of the one in use (2 would spill)
constexpr int SETS = 2;

// per backward block j (= forward block NB - 1 - j): g_h multiplier 2^e1[j] on S1', g += multiplier 2^e0[j] on S0'
struct Exps {
  int e1[NB], e0[NB];
};

// relu(s x + t) of two values -> split, and their two ReLU mask bits (bit 0: x0, bit 1: x1)
__device__ __forceinline__ unsigned act2m(float x0, float x1, float s0, float s1, float t0, float t1, unsigned &hiw,
                                          unsigned &low, unsigned &amax16) {
  float a0 = __builtin_fmaf(s0, x0, t0), a1 = __builtin_fmaf(s1, x1, t1);
  const unsigned m = (a0 > 0.f ? 1u : 0u) | (a1 > 0.f ? 2u : 0u);
  a0 = a0 > 0.f ? a0 : 0.f;
  a1 = a1 > 0.f ? a1 : 0.f;
  split2(a0, a1, hiw, low, amax16);
  return m;
}

// forward: relu(S x + T) of one k-step's two tiles -> B fragment pair; returns the 8 mask bits (bit j = slot j)
__device__ __forceinline__ unsigned act_kstep(const f32x4 &x0, const f32x4 &x1, const ST &c, half8 &hi, half8 &lo,
                                              unsigned &amax16) {
  unsigned hw[4], lw[4];
  unsigned m = act2m(x0[0], x0[1], c.s0[0], c.s0[1], c.t0[0], c.t0[1], hw[0], lw[0], amax16);
  m |= act2m(x0[2], x0[3], c.s0[2], c.s0[3], c.t0[2], c.t0[3], hw[1], lw[1], amax16) << 2;
  m |= act2m(x1[0], x1[1], c.s1[0], c.s1[1], c.t1[0], c.t1[1], hw[2], lw[2], amax16) << 4;
  m |= act2m(x1[2], x1[3], c.s1[2], c.s1[3], c.t1[2], c.t1[3], hw[3], lw[3], amax16) << 6;
  hi = __builtin_bit_cast(half8, u32x4{hw[0], hw[1], hw[2], hw[3]});
  lo = __builtin_bit_cast(half8, u32x4{lw[0], lw[1], lw[2], lw[3]});
  return m;
}

// backward: (S f m) x of one k-step's two tiles -> B fragment pair (m = the 8 mask bits of the slab, f a power of two)
__device__ __forceinline__ void grad_kstep(const f32x4 &x0, const f32x4 &x1, const f32x4 &s0, const f32x4 &s1, float f,
                                           unsigned m, half8 &hi, half8 &lo, unsigned &amax16) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = j < 4 ? x0[j] : x1[j - 4];
    const float s = j < 4 ? s0[j] : s1[j - 4];
    v[j] = (m >> j) & 1u ? (s * f) * x : 0.f;
  }
  unsigned hw[4], lw[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) split2(v[2 * q], v[2 * q + 1], hw[q], lw[q], amax16);
  hi = __builtin_bit_cast(half8, u32x4{hw[0], hw[1], hw[2], hw[3]});
  lo = __builtin_bit_cast(half8, u32x4{lw[0], lw[1], lw[2], lw[3]});
}

// brings the point's max |g'| (its 4 lanes: n, n + 16, n + 32, n + 48) into [1, 2) by a power of two; returns the exponent
// taken out (g = g' 2^X: X grows by it).  All-zero g: unchanged, 0.
__device__ __forceinline__ int renormalise(f32x4 (&G)[16]) {
  float mx = 0.f;
#pragma unroll
  for (int tt = 0; tt < 16; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = __builtin_fmaxf(mx, __builtin_fabsf(G[tt][r]));
  mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16));
  mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32));
  if (!(mx > 0.f) || !(mx < __builtin_huge_valf())) return 0;    // zero (or non-finite: left for the output to show)
  const int e = ilogbf(mx);
#pragma unroll
  for (int tt = 0; tt < 16; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) G[tt][r] = ldexpf(G[tt][r], -e);
  return e;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void occ_normals_kernel(
    const double *__restrict__ verts, const int *__restrict__ vend, const int *__restrict__ gprefix, int K,
    const half8 *__restrict__ packed_f, const half8 *__restrict__ packed_b, const float *__restrict__ fc_p_w,
    const float *__restrict__ table, const float *__restrict__ fc_out_w, Exps ex, float *__restrict__ normals,
    float *__restrict__ grad, unsigned *status) {
  const int lane = threadIdx.x;
  const int gid = blockIdx.x;
  const int g4 = 4 * (lane >> 4), n = lane & 15;
  // the mesh of this group: gprefix[prop] <= gid < gprefix[prop + 1] (empty meshes have no groups)
  int lo_k = 0, hi_k = K;
  while (hi_k - lo_k > 1) {
    const int mid = (lo_k + hi_k) >> 1;
    if (gprefix[mid] <= gid) lo_k = mid;
    else hi_k = mid;
  }
  const int prop = lo_k;
  const int vbase = vend[prop] + (gid - gprefix[prop]) * 16, vlim = vend[prop + 1];     // wave-uniform
  float px = 0.f, py = 0.f, pz = 0.f;
  if (vbase + n < vlim) {
    const int v = vbase + n;
    px = (float)verts[(size_t)v * 3 + 0];
    py = (float)verts[(size_t)v * 3 + 1];
    pz = (float)verts[(size_t)v * 3 + 2];
  }
  const float *tab = table + (size_t)prop * ROWS * H;
  unsigned amax16 = 0u;

  FragRing<DEPTH, SETS> ring;
  ring.lane = lane;
  // (through a closure, as before the ring was shared: a direct call changes hipcc's register assignment)
  auto fetch = [&](auto kc, const half8 *cur, const half8 *next) { ring.template fetch<decltype(kc)::value>(cur, next); };

  // ---- fc_p (+ fc_z bias): H' = (Wp p + bp + zb) 2^KH
  f32x4 Hs[16];
#pragma unroll
  for (int tt = 0; tt < 16; ++tt) {
    const int ch = 16 * tt + g4;
    const f32x4 b = *reinterpret_cast<const f32x4 *>(tab + ch);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = b[r];
      x = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 0], px, x);
      x = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 1], py, x);
      x = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 2], pz, x);
      Hs[tt][r] = x;
    }
  }

  // mask queue: after the forward pass M0[i] / M1[i] = masks of bn_0 / bn_1 of block i
  u64 M0[NB], M1[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) M0[i] = M1[i] = 0ull;

  half8 ahi[8], alo[8];
  // =============================== forward (occ_decoder_tail.hip, F16X3) ===============================
  {
    const half8 *wl = packed_f;
    auto half_ptr = [&](int h) { return wl + (size_t)h * HALF_FRAGS * 64; };
    ring.prime(wl);
    for (int blk = 0; blk < NB; ++blk) {
      const float *S0 = tab + (1 + 4 * blk) * H, *T0 = S0 + H, *S1 = T0 + H, *T1 = S1 + H;
      u64 m0 = 0ull, m1 = 0ull;
      f32x4 acc_cur[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      {
        const half8 *cur = half_ptr(2 * blk * 8), *next = half_ptr(2 * blk * 8 + 2);
        ST st[2];
        st_issue(st[0], S0, T0, g4);
        static_for<0, 8>([&](auto kc) {
          constexpr int ks = decltype(kc)::value;
          fetch(kc, cur, next);
          if constexpr (ks < 7) st_issue(st[(ks + 1) & 1], S0, T0, 32 * (ks + 1) + g4);
          m0 |= (u64)act_kstep(Hs[2 * ks], Hs[2 * ks + 1], st[ks & 1], ahi[ks], alo[ks], amax16) << (8 * ks);
          mma3<true>(acc_cur[0], acc_cur[1], ring.fs[ks % SETS], ahi[ks], alo[ks]);
        });
      }
      for (int mb = 0; mb < 8; ++mb) {
        const int c = blk * 8 + mb;
        f32x4 acc_next[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        half8 bhi, blo;
        ST sb;
        st_issue(sb, S1, T1, 32 * mb + g4);
        m1 = (m1 >> 8) | ((u64)act_kstep(acc_cur[0], acc_cur[1], sb, bhi, blo, amax16) << 56);
        const half8 *hA = half_ptr(2 * c + 2), *hB = half_ptr(2 * c + 1);
        // the half after phase B; behind the last slab of the last block: the backward stream's first half
        const half8 *hN = mb < 6 ? half_ptr(2 * c + 4) : mb == 6 ? half_ptr(2 * c + 3) : blk + 1 < NB ? half_ptr(2 * c + 2)
                                                                                                        : packed_b;
        if (mb < 7) {
          static_for<0, 8>([&](auto kc) {
            constexpr int ks = decltype(kc)::value;
            fetch(kc, hA, hB);
            mma3<true>(acc_next[0], acc_next[1], ring.fs[ks % SETS], ahi[ks], alo[ks]);
          });
        }
        static_for<0, 8>([&](auto kc) {
          constexpr int tp = decltype(kc)::value;
          fetch(kc, hB, hN);
          mma3<true>(Hs[2 * tp], Hs[2 * tp + 1], ring.fs[tp % SETS], bhi, blo);
        });
        acc_cur[0] = acc_next[0];
        acc_cur[1] = acc_next[1];
      }
#pragma unroll
      for (int i = 0; i + 1 < NB; ++i) {
        M0[i] = M0[i + 1];
        M1[i] = M1[i + 1];
      }
      M0[NB - 1] = m0;
      M1[NB - 1] = m1;
    }
  }

  // ---- final layer: g' = w_out m_f S_f'; from here on g = g' 2^(KH + X), X = the exponents taken out since
  {
    const float *Sf = tab + 21 * H, *Tf = Sf + H;
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) {
      const int ch0 = 16 * tt + g4;
      const f32x4 s4 = *reinterpret_cast<const f32x4 *>(Sf + ch0);
      const f32x4 t4 = *reinterpret_cast<const f32x4 *>(Tf + ch0);
      const f32x4 w4 = *reinterpret_cast<const f32x4 *>(fc_out_w + ch0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = __builtin_fmaf(s4[e], Hs[tt][e], t4[e]);
        Hs[tt][e] = a > 0.f ? w4[e] * s4[e] : 0.f;
      }
    }
  }
  int X = renormalise(Hs);

  // =============================== backward: stream block j = forward block NB - 1 - j ===============================
  {
    const half8 *wl = packed_b;
    auto half_ptr = [&](int h) { return wl + (size_t)h * HALF_FRAGS * 64; };
    for (int j = 0; j < NB; ++j) {
      const int blk = NB - 1 - j;
      const float *S0 = tab + (1 + 4 * blk) * H, *S1 = S0 + 2 * H;
      const float f1 = ldexpf(1.f, ex.e1[j]), f0 = ldexpf(1.f, ex.e0[j]);
      const u64 m0 = M0[NB - 1], m1 = M1[NB - 1];
      // ---- block input: B fragments of g', fused with W1^T slab 0; Hs then accumulates g_a0
      f32x4 acc_cur[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      {
        const half8 *cur = half_ptr(2 * j * 8), *next = half_ptr(2 * j * 8 + 2);
        static_for<0, 8>([&](auto kc) {
          constexpr int ks = decltype(kc)::value;
          fetch(kc, cur, next);
          unsigned hw[4], lw[4];
          split2(Hs[2 * ks][0], Hs[2 * ks][1], hw[0], lw[0], amax16);
          split2(Hs[2 * ks][2], Hs[2 * ks][3], hw[1], lw[1], amax16);
          split2(Hs[2 * ks + 1][0], Hs[2 * ks + 1][1], hw[2], lw[2], amax16);
          split2(Hs[2 * ks + 1][2], Hs[2 * ks + 1][3], hw[3], lw[3], amax16);
          ahi[ks] = __builtin_bit_cast(half8, u32x4{hw[0], hw[1], hw[2], hw[3]});
          alo[ks] = __builtin_bit_cast(half8, u32x4{lw[0], lw[1], lw[2], lw[3]});
          Hs[2 * ks] = f32x4{0.f, 0.f, 0.f, 0.f};
          Hs[2 * ks + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
          mma3<true>(acc_cur[0], acc_cur[1], ring.fs[ks % SETS], ahi[ks], alo[ks]);
        });
      }
      for (int mb = 0; mb < 8; ++mb) {
        const int c = j * 8 + mb;
        f32x4 acc_next[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        half8 bhi, blo;
        // ---- g_h of slab mb = S1 m1 (W1^T g)
        const f32x4 s1a = *reinterpret_cast<const f32x4 *>(S1 + 32 * mb + g4);
        const f32x4 s1b = *reinterpret_cast<const f32x4 *>(S1 + 32 * mb + g4 + 16);
        grad_kstep(acc_cur[0], acc_cur[1], s1a, s1b, f1, (unsigned)(m1 >> (8 * mb)) & 0xffu, bhi, blo, amax16);
        const half8 *hA = half_ptr(2 * c + 2), *hB = half_ptr(2 * c + 1);
        const half8 *hN = mb < 6 ? half_ptr(2 * c + 4) : mb == 6 ? half_ptr(2 * c + 3) : j + 1 < NB ? half_ptr(2 * c + 2) : wl;
        if (mb < 7) {
          // ---- W1^T slab mb + 1
          static_for<0, 8>([&](auto kc) {
            constexpr int ks = decltype(kc)::value;
            fetch(kc, hA, hB);
            mma3<true>(acc_next[0], acc_next[1], ring.fs[ks % SETS], ahi[ks], alo[ks]);
          });
        }
        // ---- g_a0[t] += W0^T[16t.., slab mb] g_h
        static_for<0, 8>([&](auto kc) {
          constexpr int tp = decltype(kc)::value;
          fetch(kc, hB, hN);
          mma3<true>(Hs[2 * tp], Hs[2 * tp + 1], ring.fs[tp % SETS], bhi, blo);
        });
        acc_cur[0] = acc_next[0];
        acc_cur[1] = acc_next[1];
      }
      // ---- g' <- (hi + lo of g') + S0 m0 g_a0
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const f32x4 sa = *reinterpret_cast<const f32x4 *>(S0 + 32 * ks + g4);
        const f32x4 sc = *reinterpret_cast<const f32x4 *>(S0 + 32 * ks + g4 + 16);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int tt = 2 * ks + (q >> 2), r = q & 3;
          const float gin = (float)ahi[ks][q] + (float)alo[ks][q];
          const float s = (q < 4 ? sa[r] : sc[r]) * f0;
          Hs[tt][r] = (m0 >> (8 * ks + q)) & 1ull ? __builtin_fmaf(s, Hs[tt][r], gin) : gin;
        }
      }
      X += renormalise(Hs);
#pragma unroll
      for (int i = NB - 1; i > 0; --i) {
        M0[i] = M0[i - 1];
        M1[i] = M1[i - 1];
      }
    }
  }

  // ---- grad p = W_p^T g = (fc_p_w 2^-KH)^T g' 2^(KH + X) = fc_p_w^T g' 2^X
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  int g4e = g4;
  asm volatile("" : "+v"(g4e));                  // fc_p_w's lane address is formed here again, not kept from the prologue
#pragma unroll
  for (int tt = 0; tt < 16; ++tt) {
    const int ch = 16 * tt + g4e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d0 = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 0], Hs[tt][r], d0);
      d1 = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 1], Hs[tt][r], d1);
      d2 = __builtin_fmaf(fc_p_w[(ch + r) * 3 + 2], Hs[tt][r], d2);
    }
  }
  d0 += __shfl_xor(d0, 16);
  d1 += __shfl_xor(d1, 16);
  d2 += __shfl_xor(d2, 16);
  d0 += __shfl_xor(d0, 32);
  d1 += __shfl_xor(d1, 32);
  d2 += __shfl_xor(d2, 32);
  const int v = vbase + n;
  if (lane < 16 && v < vlim) {
    const float nrm = __builtin_sqrtf(__builtin_fmaf(d0, d0, __builtin_fmaf(d1, d1, d2 * d2)));
    normals[(size_t)v * 3 + 0] = -d0 / nrm;
    normals[(size_t)v * 3 + 1] = -d1 / nrm;
    normals[(size_t)v * 3 + 2] = -d2 / nrm;
    if (grad) {
      grad[(size_t)v * 3 + 0] = ldexpf(d0, X);
      grad[(size_t)v * 3 + 1] = ldexpf(d1, X);
      grad[(size_t)v * 3 + 2] = ldexpf(d2, X);
    }
  }
  flag_f16_range(amax16, status, RFD_STATUS_DECODER_RANGE);
}

}  // namespace

// kw (host): [0..4] = kw0 and [5] = kw1 of packed_fwd, [6..10] = the first-half exponents of packed_bwd's blocks, [11] = its
// second-half exponent (the kw0 / kw1 arguments its rfd_occ_pack_weights_w8 call was given)
RFD_API int rfd_occ_normals_w8(int n_groups, const double *verts, const int *vend, const int *gprefix, int K,
                               const void *packed_fwd, const void *packed_bwd, const int *kw, const float *fc_p_w,
                               const float *table, const float *fc_out_w, float *normals, float *grad, int mode,
                               void *stream) {
  if (mode != RFD_OCC_MODE_F16X3) return rfd_invalid("rfd_occ_normals_w8: only RFD_OCC_MODE_F16X3 is supported");
  if (n_groups < 0 || K <= 0 || !kw || !verts || !vend || !gprefix || !normals) {
    return rfd_invalid("rfd_occ_normals_w8: arguments");
  }
  if (n_groups == 0) return 0;
  RFD_WORKSPACE(ws);
  hipStream_t s = (hipStream_t)stream;
  Exps ex;
  for (int j = 0; j < NB; ++j) {
    ex.e1[j] = kw[NB - 1 - j] - kw[6 + j];
    ex.e0[j] = kw[5] - kw[11];
  }
  hipLaunchKernelGGL(occ_normals_kernel, dim3(n_groups), dim3(64), 0, s, verts, vend, gprefix, K, (const half8 *)packed_fwd,
                     (const half8 *)packed_bwd, fc_p_w, table, fc_out_w, ex, normals, grad, rfd_status_word(ws, s));
  RFD_CHECK_LAUNCH();
  return 0;
}
