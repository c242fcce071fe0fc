/* rfd_loss.h -- the losses the test mode reports beside its metrics, on the device: the thirteen-key detection loss
 * (models/loss.py:41-271 on net_utils/nn_distance.py:15-61) and PointSeg's mask loss (pointseg.py:132-139, 168-177,
 * skip_propagation.py:100-113).  Values only: no gradient of any loss is built.
 *
 * Arithmetic contract (that of rfd_bce_logits_rowsum): every per-element term is fp32, its operations in the
 * reference's order (log-softmax is x - max - log(sum exp(x - max))); every sum over seeds, proposals, ground-truth
 * rows, points or scenes is carried in f64 in a fixed order and rounded once.  No floating-point atomics: two calls on
 * the same inputs are bitwise equal.  Nearest-row ties go to the lowest index, and the nearest row is looked for among
 * ALL label rows, the zero-padded ones included (a proposal next to the origin is assigned a padded row).
 * Every function takes a trailing stream and returns a hipError_t value (0 = success). */
#ifndef RFD_LOSS_H
#define RFD_LOSS_H
#ifdef __cplusplus
extern "C" {
#endif

#define RFD_LOSS_PARTIALS 16 /* doubles per scene in `partial` */
#define RFD_LOSS_KEYS 13     /* floats of the result vector */
/* result vector: total, vote_loss, objectness_loss, box_loss, sem_cls_loss, pos_ratio, neg_ratio, center_loss,
 * heading_cls_loss, heading_reg_loss, size_cls_loss, size_reg_loss, obj_acc */

/* compute_vote_loss: per scene, sum over the S seeds of (min over the 3 ground-truth votes of the min over the seed's
 * vote_factor predicted votes of the L1 distance) * mask, and sum of mask -> partial[b][0..1].
 *   seed_xyz (B,S,3) f32, seed_inds (B,S) int32 in [0,N), vote_xyz (B,S*vote_factor,3) f32,
 *   vote_label (B,N,9) f32, vote_label_mask (B,N) int64, partial (B,RFD_LOSS_PARTIALS) f64.  1 <= vote_factor <= 3. */
int rfd_vote_loss_partial(int B, int N, int S, int vote_factor, const float *seed_xyz, const int *seed_inds,
                          const float *vote_xyz, const float *vote_label, const long long *vote_label_mask,
                          double *partial, void *stream);

/* compute_objectness_loss + compute_box_and_sem_cls_loss + the objectness accuracy: one workgroup per scene, one
 * thread per proposal -> partial[b][2..13] and the three per-proposal arrays.
 *   aggregated_vote_xyz, center (B,K,3) f32 contiguous;  the six score tensors are read in place through their element
 *   strides (batch, proposal, channel), stride array st[18] in the order objectness_scores (2 channels), heading_scores
 *   (NH), heading_residuals_normalized (NH), size_scores (NS), size_residuals_normalized (3 NS, channel 3 s + axis),
 *   sem_cls_scores (NC);
 *   center_label (B,G,>=3) f32 with row stride ld_center; heading_class_label, size_class_label, sem_cls_label (B,G)
 *   int64 (values outside their range are clamped into it); heading_residual_label, box_label_mask (B,G) f32,
 *   size_residual_label (B,G,3) f32; mean_size (NS,3) f32.
 *   objectness_label (B,K) int64, objectness_mask (B,K) f32, object_assignment (B,K) int64: written; with given != 0
 *   objectness_label and object_assignment are READ instead (compute_box_and_sem_cls_loss's meta_data). */
int rfd_proposal_loss_partial(int B, int K, int G, int NH, int NS, int NC, const float *aggregated_vote_xyz,
                              const float *center, const float *objectness_scores, const float *heading_scores,
                              const float *heading_residuals_normalized, const float *size_scores,
                              const float *size_residuals_normalized, const float *sem_cls_scores, const int *st,
                              const float *center_label, int ld_center, const long long *heading_class_label,
                              const float *heading_residual_label, const long long *size_class_label,
                              const float *size_residual_label, const long long *sem_cls_label,
                              const float *box_label_mask, const float *mean_size, long long *objectness_label,
                              float *objectness_mask, long long *object_assignment, int given, double *partial,
                              void *stream);

/* The result vector from the per-scene partial sums (scenes added in order, in f64): every term is sum / (count + 1e-6),
 * box_loss = center + 0.1 heading_cls + heading_reg + 0.1 size_cls + size_reg, total = 10 (vote + 0.5 objectness +
 * box + 0.1 sem_cls), each rounded once; pos_ratio, neg_ratio and obj_acc are the reference's fp32 operations on the
 * exact counts.  have: bit 0 = rfd_vote_loss_partial ran, bit 1 = rfd_proposal_loss_partial ran (the other part's
 * terms are 0).   out (RFD_LOSS_KEYS) f32. */
int rfd_detection_loss_finish(int B, int K, int have, const double *partial, float *out, void *stream);

/* PointSeg's mask loss, one workgroup per proposal: partial[k] = (sum over the P points of -logp[point][target],
 * target = (grouped_label == proposal_label[k]);  || T (T^t - I) ||_F of the proposal's 64 x 64 trans_feat).
 *   logp (Kp,P,2) f32, grouped_label (Kp,P) f32 with row stride ld_label, proposal_label (Kp) int64,
 *   trans_feat (Kp,64,64) f32, partial (Kp,2) f64. */
int rfd_mask_loss_partial(int Kp, int P, const float *logp, const float *grouped_label, int ld_label,
                          const long long *proposal_label, const float *trans_feat, double *partial, void *stream);

/* out[0] = sum_k partial[k][0] / (Kp P) + scale * sum_k partial[k][1] / Kp, in f64, rounded once. */
int rfd_mask_loss_finish(int Kp, int P, float scale, const double *partial, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_LOSS_H */
