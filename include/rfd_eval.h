/* rfd_eval.h -- detection evaluation on the device: oriented-box IoU of every (detection, ground truth)
 * pair of a scene and the greedy true-positive matching of the VOC protocol.
 *
 * Device counterparts of the reference's CPU evaluation loops:
 *   net_utils/box_util.py:22-115   polygon_clip / convex_hull_intersection / box3d_vol / box3d_iou
 *   net_utils/eval_det.py:304-331  the matching loop of eval_det_cls_wo_mesh
 * One launch each per scene; nothing but `tp`, scores and class counts leaves the device.
 * Every function takes a trailing stream and returns a hipError_t value (0 = success). */
#ifndef RFD_EVAL_H
#define RFD_EVAL_H
#ifdef __cplusplus
extern "C" {
#endif

/* pred_corners (b,K,8,3), gt_corners (b,G,8,3): box corners in the order of get_3d_box
 * (box_util.py:183-198), upright camera frame (up = -y), contiguous f64.
 * iou3d (b,K,G) f64 out; iou2d (b,K,G) f64 out (bird's-eye-view IoU) or NULL.
 * One thread per pair, arithmetic in double in the reference's operation order: the two rectangles
 * from corners 3,2,1,0 (x and z), Sutherland-Hodgman clipping of rect1 by rect2 with the strict
 * `inside` test, height overlap from corners[0].y and corners[4].y, volumes from three edge lengths.
 * Differences from the reference:
 *   - the clipped polygon's area is its shoelace sum (the reference takes scipy's
 *     ConvexHull(...).volume of the already convex polygon; ~1e-14 apart);
 *   - where the reference raises QhullError (fewer than 3 clipped points, a clipped polygon of zero
 *     area, a box of zero volume) the result is 0, never NaN.
 * Boxes with exactly coincident edges (a box against an exact copy of itself, boxes that touch along a face) are
 * ill-posed for this clip: its intersection formula divides by a rounding residue there, and the reference's own
 * result is arbitrary (values above 1 occur).  The kernel follows the same arithmetic and returns the shoelace sum of
 * the same points -- finite, never NaN, but no more meaningful and not equal to the reference's hull area.
 * b <= 65535, else hipErrorInvalidValue (nothing is launched). */
int rfd_box3d_iou(int b, int K, int G, const double *pred_corners, const double *gt_corners,
                  double *iou3d, double *iou2d, void *stream);

/* Greedy matching per (scene, class, threshold).
 *   iou3d     (b,K,G) f64
 *   order     (b,C,K) i32   detection indices (0..K-1) of each class by DESCENDING score
 *   det_valid (b,C,K) u8    indexed by detection: takes part for this class
 *   gt_cls    (b,G)   i32,  gt_valid (b,G) u8
 *   thr       (nT)    f64 on the device, 1 <= nT <= 4
 *   tp        (nT,b,C,K) u8 out, indexed by detection; every element is written
 * For each valid detection in `order`: the first maximum IoU over the valid ground truths of its class
 * (strict >, lowest index wins); above the threshold and that ground truth unmatched -> true positive
 * and the ground truth is taken, otherwise false positive (tp = 0).
 * K <= 1024, G <= 256, nT <= 4, b <= 65535, C <= 65535, else hipErrorInvalidValue (nothing is launched). */
int rfd_ap_match(int b, int C, int K, int G, int nT, const double *iou3d, const int *order,
                 const unsigned char *det_valid, const int *gt_cls, const unsigned char *gt_valid,
                 const double *thr, unsigned char *tp, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_EVAL_H */
