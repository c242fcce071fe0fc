/* rfd_labels.h -- scan ground truth: what the reference's ScanNet preparation (utils/scannet/gen_scannet_w_orientation.py
 * over load_scannet_data.py's export) and its dataloader (models/iscnet/dataloader.py, ISCNet_ScanNet.__getitem__) compute
 * per scan, as five device stages.  The host side is rfdnet_amd/scan_labels.py, the numpy restatement
 * tests/scan_labels_f64.py, the reference's own output tests/golden/F_SCAN.npz.
 *
 * Conventions (those of rfd_sample.h): every entry returns 0 or a hipError_t (rfd_last_error_string), takes the stream
 * last, raises no flag in a stream's status word and reads no environment.  All counts are >= 0; a count of 0 returns 0
 * without a launch.  No float atomics anywhere: the two reductions end in integer atomic min / max on order-preserving
 * keys, so their results do not depend on the order in which workgroups arrive.
 *
 * Rule K, keys.  key32(x) of an f32 x: bits ^ 0x80000000 for a clear sign bit, ~bits for a set one; key64 the same on
 *   f64.  x + 0 first, so that -0 and +0 share a key.  Keys order like the values (NaN is not ordered: the caller keeps
 *   it out).  A minimum starts at all ones, a maximum at 0; neither is the key of a finite value.
 *
 * Rule A, instance boxes.  lo / hi of instance i = min / max per axis over the vertices with id i (ids 1 .. I; id 0 is
 *   background, an id above I is ignored).  An id without a vertex leaves its six values at 0.
 *
 * Rule E, CAD extents.  Per model m with matrix L (row major 3x3) and per vertex p:
 *   q_i = (L_i0 p_x + L_i1 p_y) + L_i2 p_z, left to right, no fused multiply-add.  ext[m] = min p (3), max p (3),
 *   min q (3), max q (3).
 *
 * Rule M, matching.  CAD box b = (cx, cy, cz, sx, sy, sz, yaw), instance box a = (cx, cy, cz, dx, dy, dz), all f64.
 *   The rectangle of b has the corners c -/+ v0 -/+ v1 in the order (-,-), (+,-), (+,+), (-,+) with
 *   v0 = (sx/2 cos yaw, sx/2 sin yaw), v1 = (-(sy/2) sin yaw, sy/2 cos yaw).  It is clipped (Sutherland-Hodgman) against
 *   x >= a.cx - dx/2, x <= a.cx + dx/2, y >= a.cy - dy/2, y <= a.cy + dy/2, in this order; where an edge p -> q
 *   crosses a bound, the new corner has the bound itself on the clipped axis and p + (q - p) t on the other, with
 *   t = (bound - p) / (q - p) taken on the clipped axis.  area = |shoelace| / 2 of what is left.
 *   h = max(0, min(b.cz + sz/2, a.cz + dz/2) - max(b.cz - sz/2, a.cz - dz/2)); inter = area h;
 *   vol_b = |shoelace of the unclipped rectangle| / 2 * ((b.cz + sz/2) - (b.cz - sz/2)); vol_a likewise = dx dy dz
 *   formed from the corners; iou = inter / (vol_b + vol_a - inter).
 *   best = 0, id = 0; for i = 0 .. I-1 in order: iou > best -> best = iou, id = i + 1.  second = the largest iou of
 *   the other instances (0 if there is none or none is positive).
 *
 * Rule P, votes.  Point p (f32, widened) is inside box b iff |u| <= sx/2, |v| <= sy/2, |p_z - cz| <= sz/2 with
 *   d = p - c, u = d_x cos yaw + d_y sin yaw, v = -d_x sin yaw + d_y cos yaw (rfd_points_in_boxes' test).  Boxes in
 *   order; the vote of a hit is c - p per axis, one f64 subtraction.  Hit number 1 of a point writes the vote to all
 *   three slots (columns 1:4, 4:7, 7:10), hit number 2 to columns 4:7, every later hit to columns 7:10.  Column 0 is
 *   1 for a point with a hit.  Rows without a hit are all zero.
 *
 * Rule S, sample.  Row r reads vertex j = choices[r].  Colour (n_color = 3): ((f64)rgb - mean) / 256, rounded to f32.
 *   Height: the f32 difference z - floor.  Without augmentation xyz and the nine vote columns are copied (votes
 *   rounded to f32).  With it, in f64: x = -x if flip_x, y = -y if flip_y, for the point and for every vote; for each
 *   vote w: e = rot(p + w); the point becomes P = f32(rot(p)); the vote becomes f32(e - (f64)P), with
 *   rot(a) = (fma(a_y, -s, c a_x), fma(a_y, c, s a_x), a_z): the first product rounded, the second fused into the sum.
 *   That is a row of numpy's dot through a BLAS kernel that accumulates over k with fused multiply-adds (the third term
 *   is a_z times 0), the arithmetic the reference's output was made with.  The height column
 *   is that of the unflipped, unrotated vertex.  mask = (i64) column 0 of the votes; instance = (f32) the vertex's id. */
#ifndef RFD_LABELS_H
#define RFD_LABELS_H
#ifdef __cplusplus
extern "C" {
#endif

/* vertices (N, stride) f32 with xyz first, ids (N) u32 -> box (I,6) f32: lo xyz, hi xyz (rule A).  keys (I,6) u32 is
 * workspace the call initialises itself.  Partial minima and maxima are formed per wave and per workgroup in LDS; a
 * workgroup issues one atomic per destination it touched.  Refused: stride < 3. */
int rfd_labels_instance_aabb(int N, int I, int stride, const float *vertices, const unsigned *ids, unsigned *keys,
                             float *box, void *stream);

/* points (sum_v,3) f64, L (M,9) f64 -> ext (M,12) f64 (rule E).  The models' vertex ranges are cut into R runs of at
 * most `step` vertices (ragged.runs): run r belongs to model run_owner[r], starts at row run_start[r] and ends at
 * min(start + step, off[owner + 1]); off (M + 1) is the exclusive prefix of the vertex counts.  One workgroup per run,
 * one 64-bit atomic per destination per workgroup.  keys (M,12) u64 is workspace the call initialises itself.  A model
 * without a vertex keeps the initial keys, which decode to NaN: the caller refuses such a model before the call. */
int rfd_labels_cad_extents(int M, int R, int step, const double *points, const int *off, const int *run_owner,
                           const int *run_start, const double *L, unsigned long long *keys, double *ext, void *stream);

/* cad (M,7) f64, inst (I,6) f64 -> best_iou (M) f64, best_id (M) i32, second_iou (M) f64 (rule M).  One wave per CAD
 * box, the instances dealt over its lanes. */
int rfd_labels_match_instances(int M, int I, const double *cad, const double *inst, double *best_iou, int *best_id,
                               double *second_iou, void *stream);

/* vertices (N, stride) f32, boxes (M,7) f64 -> votes (N,10) f64, hits (N) i32 (rule P).  One thread per vertex, the
 * boxes staged in LDS 64 at a time.  M = 0 clears both outputs.  Refused: stride < 3. */
int rfd_labels_point_votes(int N, int M, int stride, const float *vertices, const double *boxes, double *votes,
                           int *hits, void *stream);

/* The dataloader's per-point work (rule S): choices (P) i64 rows of vertices (N, stride) f32, votes (N,10) f64 and
 * ids (N) u32 -> points (P, 3 + n_color + use_height) f32, vote_label (P,9) f32, vote_mask (P) i64, instance (P) f32.
 * mean (3) f64 is read on the HOST (n_color = 3 only).  A choice outside [0, N) writes a row of zeros.  Refused:
 * n_color not 0 or 3, stride < 3 + n_color. */
int rfd_labels_sample(int P, int N, int stride, int n_color, int use_height, int augment, int flip_x, int flip_y,
                      double c, double s, float floor_height, const double *mean, const float *vertices,
                      const double *votes, const unsigned *ids, const long long *choices, float *points,
                      float *vote_label, long long *vote_mask, float *instance, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_LABELS_H */
