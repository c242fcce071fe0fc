/* rfd_latent.h -- the completion loss of the test mode on the device: the latent encoder q(z | p, occ, c)
 * (models/iscnet/modules/encoder_latent.py:49-73), its reparameterised sample and KL term, the row sums of
 * binary_cross_entropy_with_logits and the voxel IoU counts (occupancy_net.py:59-109, network.py:144-148).
 *
 * The encoder is  net1 = fc_1(relu(fc_0(occ) + fc_pos(p) + fc_c(c))),  net_{s+1} = fc_{s+1}(relu([net_s | max_T net_s])),
 * (mean, logstd) = fc_mean / fc_logstd (max_T net3).  The pooled half of a concatenation is one bias vector per
 * proposal, so the (K, T, 256) tensors are never formed; a point's input is 16 bytes, so every stage recomputes its
 * predecessors in registers and only the three pooled rows (K, 128) live in memory.  Exact fp32 throughout
 * (v_mfma_f32_32x32x2_f32 = a k-ordered fmaf chain); the per-proposal vectors (fc_c(c), the pooled biases, the head)
 * are summed in f64 in a fixed order and rounded once.  Every result is independent of K, of the grid shape and of
 * the order of a proposal's points (the pool is a max).
 * Every function takes a trailing stream and returns a hipError_t value (0 = success). */
#ifndef RFD_LATENT_H
#define RFD_LATENT_H
#ifdef __cplusplus
extern "C" {
#endif

/* The hidden width (128) is fixed.  "lane order": position 2 j + h holds channel
 * 32 (j >> 4) + 8 ((j & 15) >> 2) + 4 h + (j & 3), the k order in which a 32x32 accumulator is the next layer's B operand.
 *   c     (K, c_dim) f32 or NULL when c_dim == 0
 *   wcT   (c_dim, 128) f32: fc_c.weight transposed, columns in lane order
 *   b0    (128) f32: fc_0.bias + fc_pos.bias + fc_c.bias, lane order
 *   bias0 (K, 128) f32 out: b0 + fc_c.weight . c, lane order
 *   pool  (3, K, 128) f32 out: filled with -inf (the running maxima of the three stages) */
int rfd_latent_prep(int K, int c_dim, const float *c, const float *wcT, const float *b0, float *bias0, float *pool,
                    void *stream);

/* Stage `stage` (1, 2, 3): net_stage of every point, recomputed from the input, max over a proposal's T points into
 * pool[stage - 1] (float max by integer atomics; pool[stage - 1] must hold -inf, pool[0 .. stage - 2] the finished rows).
 *   p (K, T, 3), occ (K, T) f32;  l0 (128, 4) f32: (fc_pos.weight row, fc_0.weight) per channel, lane order
 *   wa  (3, 4, 16, 64, 4) f32: fc_1.weight, fc_2.weight[:, :128], fc_3.weight[:, :128] as MFMA A fragments
 *       (element (b, j4, lane, e) = W[32 b + (lane & 31)][lane-order position 2 (4 j4 + e) + (lane >> 5)])
 *   wbT (2, 128, 128) f32: fc_2.weight[:, 128:] and fc_3.weight[:, 128:], transposed (natural channel order)
 *   b123 (3, 128) f32: the biases of fc_1, fc_2, fc_3.   Rows beyond T never reach the pool; T >= 1 is arbitrary. */
int rfd_latent_stage(int stage, int K, int T, const float *p, const float *occ, const float *l0, const float *bias0,
                     const float *wa, const float *wbT, const float *b123, float *pool, void *stream);

/* mean = fc_mean(pool3), logstd = fc_logstd(pool3) (K, z_dim); with eps (K, z_dim): z = mean + eps * exp(logstd) (fp32,
 * each operation rounded); kl[k] = sum_j 0.5 (exp(2 logstd) + mean^2 - 1) - logstd, terms and sum in f64 from the fp32
 * mean / logstd, rounded once.   whT (128, 2 z_dim): [fc_mean.weight; fc_logstd.weight] transposed, bh (2 z_dim).
 * eps / z / kl may be NULL (z needs eps).  1 <= z_dim <= 512. */
int rfd_latent_head(int K, int z_dim, const float *pool3, const float *whT, const float *bh, const float *eps,
                    float *mean, float *logstd, float *z, float *kl, void *stream);

/* out[k] = sum_t max(x, 0) - x y + log1p(exp(-|x|)),  x = logits[k * ld_logits + t], y = target[k * ld_target + t]:
 * the term in fp32, the row summed in f64 in a fixed order (no atomics) and rounded once. */
int rfd_bce_logits_rowsum(int K, int T, const float *logits, int ld_logits, const float *target, int ld_target,
                          float *out, void *stream);

/* inter[k] / uni[k] = number of v with (logits[k * ld_logits + v] >= logit_threshold) and / or (gt[k * V + v] >= 0.5),
 * counted by ballot + popcount; int32. */
int rfd_voxel_iou(int K, int V, const float *logits, int ld_logits, float logit_threshold, const float *gt, int *inter,
                  int *uni, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_LATENT_H */
