// det_loss.hip -- the detection loss and PointSeg's mask loss of the test mode (include/rfd_loss.h).
// Latency-bound like box_eval.hip: a scene is 1024 seeds, 256 proposals and 64 label rows, so a workgroup per scene (per
// proposal for the mask loss) does all of it and a one-workgroup kernel finishes.  Per-element terms are fp32 in the
// reference's order; every sum is f64 in a fixed order (thread t takes elements t, t + 256, ..., then a tree in LDS).
#include "common.h"
#include "../../include/rfd_loss.h"

namespace {

constexpr int WG = 256;
constexpr float NEAR_THRESHOLD = 0.3f, FAR_THRESHOLD = 0.6f;
constexpr int GT_VOTE_FACTOR = 3;

// partial[b][...]
enum { P_VOTE = 0, P_VOTE_N, P_OBJ, P_MASK_N, P_POS_N, P_CENTER1, P_HCLS, P_HREG, P_SCLS, P_SREG, P_SEM, P_ACC,
       P_CENTER2, P_BOX_N };
static_assert(P_BOX_N < RFD_LOSS_PARTIALS, "partial row too short");

// sum of v over the workgroup, in a fixed order; every thread gets it
__device__ __forceinline__ double block_sum(double v, double *s_red) {
  const int t = threadIdx.x;
  __syncthreads();                       // the previous sum's readers are done
  s_red[t] = v;
  __syncthreads();
  for (int d = WG / 2; d > 0; d >>= 1) {
    if (t < d) s_red[t] += s_red[t + d];
    __syncthreads();
  }
  return s_red[0];
}

// net_utils/nn_distance.py:15-32, delta = 1
__device__ __forceinline__ float huber1(float e) {
  const float a = fabsf(e);
  const float q = fminf(a, 1.0f);
  const float lin = a - q;
  return 0.5f * (q * q) + 1.0f * lin;
}

// -log_softmax(x)[label] over n channels `sc` apart: x - max - log(sum exp(x - max)), negated
__device__ __forceinline__ float cross_entropy(const float *x, int sc, int n, int label) {
  float mx = x[0];
  for (int c = 1; c < n; ++c) mx = fmaxf(mx, x[(size_t)c * sc]);
  float se = 0.f;
  for (int c = 0; c < n; ++c) se += expf(x[(size_t)c * sc] - mx);
  const float lp = (x[(size_t)label * sc] - mx) - logf(se);
  return -lp;
}

__device__ __forceinline__ int clamp_label(long long v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : (int)v); }

__device__ __forceinline__ float sqdist3(const float *a, const float *b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(WG) void vote_loss_kernel(int N, int S, int vf, const float *__restrict__ seed_xyz,
                                                       const int *__restrict__ seed_inds,
                                                       const float *__restrict__ vote_xyz,
                                                       const float *__restrict__ vote_label,
                                                       const long long *__restrict__ vote_label_mask,
                                                       double *__restrict__ partial) {
  __shared__ double s_red[WG];
  const int t = threadIdx.x, b = blockIdx.x;
  double sum = 0.0, cnt = 0.0;
  for (int s = t; s < S; s += WG) {
    const size_t row = (size_t)b * S + s;
    int ind = seed_inds[row];
    ind = ind < 0 ? 0 : (ind >= N ? N - 1 : ind);
    const size_t pt = (size_t)b * N + ind;
    const float m = (float)vote_label_mask[pt];
    const float *sx = seed_xyz + row * 3, *gl = vote_label + pt * 9, *pv = vote_xyz + row * vf * 3;
    float best = INFINITY;
    for (int j = 0; j < GT_VOTE_FACTOR; ++j) {
      const float gx = gl[3 * j] + sx[0], gy = gl[3 * j + 1] + sx[1], gz = gl[3 * j + 2] + sx[2];
      for (int i = 0; i < vf; ++i) {
        const float d = (fabsf(pv[3 * i] - gx) + fabsf(pv[3 * i + 1] - gy)) + fabsf(pv[3 * i + 2] - gz);
        best = fminf(best, d);
      }
    }
    sum += (double)(best * m);
    cnt += (double)m;
  }
  sum = block_sum(sum, s_red);
  cnt = block_sum(cnt, s_red);
  if (t == 0) {
    partial[(size_t)b * RFD_LOSS_PARTIALS + P_VOTE] = sum;
    partial[(size_t)b * RFD_LOSS_PARTIALS + P_VOTE_N] = cnt;
  }
}

struct ScoreStrides { int v[18]; };

struct ProposalArgs {
  int K, G, NH, NS, NC, ld_center, given;
  const float *agg, *center, *obj, *hs, *hr, *ss, *sr, *sem;
  const float *center_label, *hres_label, *sres_label, *box_mask, *mean_size;
  const long long *hcls_label, *scls_label, *sem_label;
  long long *objectness_label, *object_assignment;
  float *objectness_mask;
  double *partial;
  ScoreStrides st;
};

__global__ __launch_bounds__(WG) void proposal_loss_kernel(const ProposalArgs a) {
  __shared__ double s_red[WG];
  const int t = threadIdx.x, b = blockIdx.x;
  const int K = a.K, G = a.G;
  const int *st = a.st.v;
  const float *gt = a.center_label + (size_t)b * G * a.ld_center;
  double acc[10];
  for (int i = 0; i < 10; ++i) acc[i] = 0.0;
  for (int k = t; k < K; k += WG) {
    const size_t row = (size_t)b * K + k;
    // nearest label row of the aggregated vote and of the predicted centre: strict <, so the lowest index wins a tie
    const float *pa = a.agg + row * 3, *pc = a.center + row * 3;
    float d_agg = INFINITY, d_ctr = INFINITY;
    int assign = 0;
    for (int g = 0; g < G; ++g) {
      const float *q = gt + (size_t)g * a.ld_center;
      const float da = sqdist3(pa, q), dc = sqdist3(pc, q);
      if (da < d_agg) {
        d_agg = da;
        assign = g;
      }
      d_ctr = fminf(d_ctr, dc);
    }
    int label;
    float mask;
    if (a.given) {
      label = a.objectness_label[row] != 0;
      assign = clamp_label(a.object_assignment[row], G);
      mask = 0.f;                                            // objectness terms are not this call's
    } else {
      const float e = sqrtf(d_agg + 1e-6f);
      label = e < NEAR_THRESHOLD;
      mask = (e < NEAR_THRESHOLD || e > FAR_THRESHOLD) ? 1.f : 0.f;
      a.objectness_label[row] = label;
      a.objectness_mask[row] = mask;
      a.object_assignment[row] = assign;
    }
    const float lab = (float)label;
    const size_t lrow = (size_t)b * G + assign;
    // objectness: weighted ([0.2, 0.8]) two-way cross-entropy, and the accuracy of the arg-max
    const float *xo = a.obj + (size_t)b * st[0] + (size_t)k * st[1];
    const float ce_obj = (label ? 0.8f : 0.2f) * cross_entropy(xo, st[2], 2, label);
    const int pred = xo[st[2]] > xo[0];
    acc[0] += (double)(ce_obj * mask);
    acc[1] += (double)mask;
    acc[2] += (double)lab;
    acc[3] += (double)(d_ctr * lab);
    // heading
    const int hc = clamp_label(a.hcls_label[lrow], a.NH);
    const float *xh = a.hs + (size_t)b * st[3] + (size_t)k * st[4];
    acc[4] += (double)(cross_entropy(xh, st[5], a.NH, hc) * lab);
    const float hres = a.hres_label[lrow] / (float)(3.14159265358979323846 / (double)a.NH);
    const float hp = a.hr[(size_t)b * st[6] + (size_t)k * st[7] + (size_t)hc * st[8]];
    acc[5] += (double)(huber1(hp - hres) * lab);
    // size
    const int sc = clamp_label(a.scls_label[lrow], a.NS);
    const float *xs = a.ss + (size_t)b * st[9] + (size_t)k * st[10];
    acc[6] += (double)(cross_entropy(xs, st[11], a.NS, sc) * lab);
    const float *xr = a.sr + (size_t)b * st[12] + (size_t)k * st[13];
    float hub = 0.f;
    for (int ax = 0; ax < 3; ++ax) {
      const float want = a.sres_label[lrow * 3 + ax] / a.mean_size[sc * 3 + ax];
      hub += huber1(xr[(size_t)(3 * sc + ax) * st[14]] - want);
    }
    acc[7] += (double)((hub / 3.0f) * lab);
    // semantic class
    const int cc = clamp_label(a.sem_label[lrow], a.NC);
    const float *xc = a.sem + (size_t)b * st[15] + (size_t)k * st[16];
    acc[8] += (double)(cross_entropy(xc, st[17], a.NC, cc) * lab);
    acc[9] += (double)((pred == label ? 1.f : 0.f) * mask);
  }
  // per label row: the nearest predicted centre, masked by box_label_mask
  double c2 = 0.0, nbox = 0.0;
  for (int g = t; g < G; g += WG) {
    const float *q = gt + (size_t)g * a.ld_center;
    float d = INFINITY;
    for (int k = 0; k < K; ++k) d = fminf(d, sqdist3(a.center + ((size_t)b * K + k) * 3, q));
    const float m = a.box_mask[(size_t)b * G + g];
    c2 += (double)(d * m);
    nbox += (double)m;
  }
  double *out = a.partial + (size_t)b * RFD_LOSS_PARTIALS;
  for (int i = 0; i < 10; ++i) {
    const double s = block_sum(acc[i], s_red);
    if (t == 0) out[P_OBJ + i] = s;
  }
  c2 = block_sum(c2, s_red);
  nbox = block_sum(nbox, s_red);
  if (t == 0) {
    out[P_CENTER2] = c2;
    out[P_BOX_N] = nbox;
  }
}

__global__ __launch_bounds__(64) void detection_finish_kernel(int B, int K, int have,
                                                              const double *__restrict__ partial,
                                                              float *__restrict__ out) {
  if (threadIdx.x != 0) return;
  double s[RFD_LOSS_PARTIALS];
  for (int i = 0; i < RFD_LOSS_PARTIALS; ++i) s[i] = 0.0;
  for (int b = 0; b < B; ++b) {
    if (have & 1)
      for (int i = P_VOTE; i <= P_VOTE_N; ++i) s[i] += partial[(size_t)b * RFD_LOSS_PARTIALS + i];
    if (have & 2)
      for (int i = P_OBJ; i <= P_BOX_N; ++i) s[i] += partial[(size_t)b * RFD_LOSS_PARTIALS + i];
  }
  const double pos = s[P_POS_N] + 1e-6;
  const double vote = s[P_VOTE] / (s[P_VOTE_N] + 1e-6);
  const double objectness = s[P_OBJ] / (s[P_MASK_N] + 1e-6);
  const double center = s[P_CENTER1] / pos + s[P_CENTER2] / (s[P_BOX_N] + 1e-6);
  const double hcls = s[P_HCLS] / pos, hreg = s[P_HREG] / pos, scls = s[P_SCLS] / pos, sreg = s[P_SREG] / pos;
  const double sem = s[P_SEM] / pos;
  const double box = center + 0.1 * hcls + hreg + 0.1 * scls + sreg;
  const double total = 10.0 * (vote + 0.5 * objectness + box + 0.1 * sem);
  // the three statistics: the reference's fp32 operations on the (exact) counts
  const float n = (float)((long long)B * K);
  const float pos_ratio = (float)s[P_POS_N] / n;
  const float neg_ratio = (float)s[P_MASK_N] / n - pos_ratio;
  const float obj_acc = (float)s[P_ACC] / ((float)s[P_MASK_N] + 1e-6f);
  out[0] = (float)total;
  out[1] = (float)vote;
  out[2] = (float)objectness;
  out[3] = (float)box;
  out[4] = (float)sem;
  out[5] = pos_ratio;
  out[6] = neg_ratio;
  out[7] = (float)center;
  out[8] = (float)hcls;
  out[9] = (float)hreg;
  out[10] = (float)scls;
  out[11] = (float)sreg;
  out[12] = obj_acc;
}

// One workgroup per proposal.  T (T^t - I): entry (i, j) = sum_l T[i][l] (T[j][l] - [j == l]); the difference is rounded
// to fp32 as the reference forms it, the products and the sums are f64.
__global__ __launch_bounds__(WG) void mask_loss_kernel(int P, const float *__restrict__ logp,
                                                       const float *__restrict__ grouped_label, int ld_label,
                                                       const long long *__restrict__ proposal_label,
                                                       const float *__restrict__ trans_feat,
                                                       double *__restrict__ partial) {
  __shared__ double s_red[WG];
  __shared__ float s_t[64][65];
  const int t = threadIdx.x, k = blockIdx.x;
  const float want = (float)proposal_label[k];
  const float *lp = logp + (size_t)k * P * 2, *gl = grouped_label + (size_t)k * ld_label;
  double nll = 0.0;
  for (int p = t; p < P; p += WG) {
    const int target = gl[p] == want;
    nll += (double)(-lp[2 * p + target]);
  }
  const float *T = trans_feat + (size_t)k * 4096;
  for (int e = t; e < 4096; e += WG) s_t[e >> 6][e & 63] = T[e];
  nll = block_sum(nll, s_red);                                           // (its barriers also publish s_t)
  double sq = 0.0;
  for (int e = t; e < 4096; e += WG) {
    const int i = e >> 6, j = e & 63;
    double m = 0.0;
    for (int l = 0; l < 64; ++l) {
      const float d = s_t[j][l] - (j == l ? 1.0f : 0.0f);
      m += (double)s_t[i][l] * (double)d;
    }
    sq += m * m;
  }
  sq = block_sum(sq, s_red);
  if (t == 0) {
    partial[2 * (size_t)k] = nll;
    partial[2 * (size_t)k + 1] = sqrt(sq);
  }
}

__global__ __launch_bounds__(WG) void mask_finish_kernel(int Kp, int P, float scale, const double *__restrict__ partial,
                                                         float *__restrict__ out) {
  __shared__ double s_red[WG];
  const int t = threadIdx.x;
  double nll = 0.0, reg = 0.0;
  for (int k = t; k < Kp; k += WG) {
    nll += partial[2 * (size_t)k];
    reg += partial[2 * (size_t)k + 1];
  }
  nll = block_sum(nll, s_red);
  reg = block_sum(reg, s_red);
  if (t == 0) out[0] = (float)(nll / ((double)Kp * (double)P) + (double)scale * (reg / (double)Kp));
}

}  // namespace

RFD_API int rfd_vote_loss_partial(int B, int N, int S, int vote_factor, const float *seed_xyz, const int *seed_inds,
                                  const float *vote_xyz, const float *vote_label, const long long *vote_label_mask,
                                  double *partial, void *stream) {
  if (B <= 0) return 0;
  if (N < 1 || S < 0) return rfd_invalid("rfd_vote_loss_partial: N >= 1, S >= 0");
  if (vote_factor < 1 || vote_factor > 3) return rfd_invalid("rfd_vote_loss_partial: 1 <= vote_factor <= 3");
  hipLaunchKernelGGL(vote_loss_kernel, dim3(B), dim3(WG), 0, (hipStream_t)stream, N, S, vote_factor, seed_xyz,
                     seed_inds, vote_xyz, vote_label, vote_label_mask, partial);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_proposal_loss_partial(int B, int K, int G, int NH, int NS, int NC, const float *aggregated_vote_xyz,
                                      const float *center, const float *objectness_scores,
                                      const float *heading_scores, const float *heading_residuals_normalized,
                                      const float *size_scores, const float *size_residuals_normalized,
                                      const float *sem_cls_scores, const int *st, const float *center_label,
                                      int ld_center, const long long *heading_class_label,
                                      const float *heading_residual_label, const long long *size_class_label,
                                      const float *size_residual_label, const long long *sem_cls_label,
                                      const float *box_label_mask, const float *mean_size,
                                      long long *objectness_label, float *objectness_mask,
                                      long long *object_assignment, int given, double *partial, void *stream) {
  if (B <= 0) return 0;
  if (K < 1 || G < 1 || NH < 1 || NS < 1 || NC < 1 || ld_center < 3)
    return rfd_invalid("rfd_proposal_loss_partial: K, G, NH, NS, NC >= 1, ld_center >= 3");
  if (st == nullptr) return rfd_invalid("rfd_proposal_loss_partial: the stride array is missing");
  for (int i = 0; i < 18; ++i)
    if (st[i] < 0) return rfd_invalid("rfd_proposal_loss_partial: negative stride");
  ProposalArgs a;
  a.K = K, a.G = G, a.NH = NH, a.NS = NS, a.NC = NC, a.ld_center = ld_center, a.given = given;
  a.agg = aggregated_vote_xyz, a.center = center, a.obj = objectness_scores, a.hs = heading_scores;
  a.hr = heading_residuals_normalized, a.ss = size_scores, a.sr = size_residuals_normalized, a.sem = sem_cls_scores;
  a.center_label = center_label, a.hres_label = heading_residual_label, a.sres_label = size_residual_label;
  a.box_mask = box_label_mask, a.mean_size = mean_size;
  a.hcls_label = heading_class_label, a.scls_label = size_class_label, a.sem_label = sem_cls_label;
  a.objectness_label = objectness_label, a.object_assignment = object_assignment, a.objectness_mask = objectness_mask;
  a.partial = partial;
  for (int i = 0; i < 18; ++i) a.st.v[i] = st[i];
  hipLaunchKernelGGL(proposal_loss_kernel, dim3(B), dim3(WG), 0, (hipStream_t)stream, a);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_detection_loss_finish(int B, int K, int have, const double *partial, float *out, void *stream) {
  if (B <= 0 || K <= 0) return rfd_invalid("rfd_detection_loss_finish: B, K >= 1");
  hipLaunchKernelGGL(detection_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, B, K, have, partial, out);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mask_loss_partial(int Kp, int P, const float *logp, const float *grouped_label, int ld_label,
                                  const long long *proposal_label, const float *trans_feat, double *partial,
                                  void *stream) {
  if (Kp <= 0) return 0;
  if (P < 1 || ld_label < P) return rfd_invalid("rfd_mask_loss_partial: P >= 1 and the label row stride must cover P");
  hipLaunchKernelGGL(mask_loss_kernel, dim3(Kp), dim3(WG), 0, (hipStream_t)stream, P, logp, grouped_label, ld_label,
                     proposal_label, trans_feat, partial);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_mask_loss_finish(int Kp, int P, float scale, const double *partial, float *out, void *stream) {
  if (Kp <= 0 || P < 1) return rfd_invalid("rfd_mask_loss_finish: Kp, P >= 1");
  hipLaunchKernelGGL(mask_finish_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, Kp, P, scale, partial, out);
  RFD_CHECK_LAUNCH();
  return 0;
}
