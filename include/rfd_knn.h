/* rfd_knn.h -- exact k nearest neighbours among points: for every query point the k closest points of its object's point
 * set, for the K point sets of a ragged batch at once, and the fixed-shape sums the point-cloud metrics are made of.
 * rfdnet_amd/knn.py drives these entries; tests/knn_f64.py restates the rules in numpy float64 and the kernels follow its
 * order of operations.  It is rfd_mesh_dist.h with points in place of triangles and the k least keys in place of one.
 * No floating-point atomics, no workgroup waits for another: a result depends on neither the grid, nor the walk, nor the
 * batch, nor the order of execution.
 *
 * A batch is K point sets: set k owns the rows pend[k] .. pend[k+1]-1 of points (N,3) f64 (K + 1 ints, on the device).
 * A row reported to the caller is LOCAL to its set (row - pend[k]), which is what pykdtree calls an index.  Everything is
 * f64, one rounding per written operation (the library is built with -ffp-contract=off); the square root is the
 * correctly rounded one.  Every dot product is (x0 y0 + x1 y1) + x2 y2.
 *
 * Rule N1, valid points.  A data point takes part iff its three coordinates are finite.  Nothing is refused for its data.
 * Rule N2, frame.  Rule D2 of rfd_mesh_dist.h word for word, over the valid points of the set: lo[k], hi[k] (0, 0 without
 *   any) and R[k] cells per axis, 1 <= R <= 64.  The HOST computes, in f64 and per axis, inv_h = R / (hi - lo) and
 *   h = (hi - lo) / R, both 0 for an axis of zero extent (such an axis has ONE cell: R_a = 1 where inv_h_a == 0, else R),
 *   and slack = 2^-30 max over the axes of max(hi - lo, |lo|, |hi|).  A coordinate's cell is
 *   clamp((int)floor((x - lo) * inv_h), 0, R - 1), 0 where the product is a NaN.  The cells of set k are
 *   cbase[k] + (ix R + iy) R + iz; cbase[K] < 2^31.  The default R = clamp(ceil(cbrt(n_valid / 8)), 1, 64) is the host's
 *   choice (about 8 points per cell of a filled frame); no result depends on it.
 * Rule N3, cell lists.  A valid point belongs to the one cell of its coordinates.  One CSR for the whole batch (count,
 *   prefix sum by the caller, fill); the list holds GLOBAL rows.  The order inside a cell is whatever the integer atomics
 *   give; rule N5 makes it irrelevant.  The fill pass may also write the coordinates in list order (`sorted` (M,3)), so
 *   that a cell's candidates are contiguous; no result depends on whether the query reads them there or in `points`.
 * Rule N4, distance.  r = q - p per axis, d2 = (rx rx + ry ry) + rz rz.
 * Rule N5, the answer.  The k least keys (d2, local row), in ascending key order, of the candidates: the points of the
 *   query's set that are valid, not masked (mask (N) u8 or null: a non-zero value excludes that GLOBAL row for this call)
 *   and have d2 < limit2 (a double passed by value, +inf without a bound; strict, as pykdtree reports a distance
 *   >= bound^2 as missing).  Key (a, i) is less than (b, j) iff a < b, or a == b and i < j.  A candidate enters iff its
 *   key is less than the key in slot k - 1.  Slots that stay empty hold (+inf, -1).  A query with a non-finite
 *   coordinate, or with an object outside [0, K), gives (NaN, -1) in all k slots.  1 <= k <= 32.
 * Rule N6, walk.  Rule D6 of rfd_mesh_dist.h with best := min(d2 of slot k - 1, limit2): p' = min(max(p, lo), hi),
 *   c = the cell of p', shell r = 0, 1, ... the cells at Chebyshev distance r of c; per axis and side that still has
 *   cells the gap p' - (lo + (c - r) h) and (lo + (c + r + 1) h) - p', g the least of them, no side left: done; with
 *   o = |p - p'| per axis, every length shortened by slack and clamped at 0 before it is squared,
 *     bound = (((ox^2 + oy^2) + oz^2) + g^2) (1 - 2^-40);   the walk stops iff best < bound.
 *   The walk only filters: R = 1 is the brute force and every R gives its bits.  A list row outside its set is skipped,
 *   not trusted.
 * Rule N7, sums per segment.  Rule D8's shape: segment s holds the entries seg[s] .. seg[s+1]-1, each the slot-0 result
 *   (d2, row) of a query of object obj, optionally with the source normal n_s (n,3); n_t (N,3) holds the target points'
 *   normals and is read at the GLOBAL row pend[obj] + row.  d = sqrt(d2).  An entry whose d is not finite, whose row is
 *   -1 (or outside its set, or whose object is outside [0, K)) is left out and counted.  For the others: sum d, sum d2,
 *   sum |n_s . n_t| (0 when either array is null), and for each of T <= 8 thresholds the number of d <= tau_t.  The
 *   three f64 sums: partial j (0..63) takes the segment's entries j, j + 64, ... in order, starting from 0 (a left-out
 *   entry adds nothing); then partial j += partial j + 32 (j < 32), j + 16 (j < 16), ... , j + 1 (j = 0). */
#ifndef RFD_KNN_H
#define RFD_KNN_H
#ifdef __cplusplus
extern "C" {
#endif

/* Two passes over the N points, one thread per point.
 *   lo == NULL (rule N1):  valid (N) u8 and pobj (N) i32, the point's set, are WRITTEN.
 *   lo != NULL (rule N2):  valid and pobj are READ, and cell (N) i32 is written: the point's cell of the batch, -1 for a
 *   point that is not valid.
 * Refused: N, K < 0, 3 N beyond 2^31, K < 1 with N > 0, a null pointer. */
int rfd_knn_points(int N, int K, const double *points, const int *pend, const double *lo, const double *inv_h,
                   const int *res, const int *cbase, unsigned char *valid, int *pobj, int *cell, void *stream);

/* The two passes of the cell lists over cell (N) (rule N3).  list == NULL: cursor[cell] += 1 for every point with a cell
 * (the caller clears its n_cells entries).  Otherwise cursor holds every cell's first slot, every such point takes the
 * next slot of its cell, writes its GLOBAL row there and, unless `sorted` is null, its coordinates to sorted (M,3) f64 at
 * that slot.  A cell outside [0, n_cells) or a slot outside [0, M) is skipped.  Refused: N, n_cells, M < 0, a null
 * pointer. */
int rfd_knn_cells(int N, const int *cell, int n_cells, int *cursor, int *list, int M, const double *points,
                  double *sorted, void *stream);

/* queries (n,3) f64, qobj (n) i32 -> d2 (n,k) f64, idx (n,k) i32 (rules N4 - N6).  points (N,3), pend (K + 1): the batch;
 * mask (N) u8 or null; lo, hi, inv_h, h (K,3) f64, slack (K) f64, res (K) i32, cbase (K + 1) i32: rule N2; offsets
 * (cbase[K] + 1) i32 and list (M) i32: rule N3; sorted (M,3) f64 or null.  One thread per query, the k best keys and the
 * shell state in registers.  Refused: n, K, N, M < 0, k outside 1 .. 32, n k or 3 n beyond 2^31, a NaN limit2, a null
 * pointer. */
int rfd_knn_query(int n, const double *queries, const int *qobj, int k, double limit2, const unsigned char *mask, int K,
                  int N, const double *points, const int *pend, const double *lo, const double *hi, const double *inv_h,
                  const double *h, const double *slack, const int *res, const int *cbase, const int *offsets,
                  const int *list, int M, const double *sorted, double *d2, int *idx, void *stream);

/* Rule N7: seg (S + 1) i32 ascending offsets into the n entries; entry e reads d2[e stride] and row[e stride] (the slot
 * 0 of (n,stride) query results), qobj[e], n_s (n,3) f64 and n_t (N,3) f64 (either null: the third sum is 0); tau (T) f64
 * -> sums (S,3) f64: sum d, sum d2, sum |n_s . n_t|;  counts (S, 1 + T) i32: the entries left out, then the entries with
 * d <= tau_t.  One wave per segment.  Refused: S, n, K, N, T < 0, T > 8, stride < 1, n stride or 3 n beyond 2^31, a null
 * pointer. */
int rfd_knn_sums(int S, int n, int stride, const int *seg, const double *d2, const int *row, const int *qobj, int K,
                 int N, const int *pend, const double *n_s, const double *n_t, int T, const double *tau, double *sums,
                 int *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_KNN_H */
