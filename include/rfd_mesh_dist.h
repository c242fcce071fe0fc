/* rfd_mesh_dist.h -- exact point-to-mesh distance: for every query point the closest triangle of its object's mesh, for
 * the K meshes of a ragged batch at once, and what the surface metrics are made of (Chamfer distance, F-score, normal
 * consistency): ragged surface samples and fixed-shape sums per segment.  rfdnet_amd/mesh_distance.py drives these
 * entries; tests/mesh_dist_f64.py restates the rules in numpy float64 and the kernels follow its order of operations.
 * No floating-point atomics, no workgroup waits for another: a result depends on neither the grid, nor the walk, nor the
 * batch, nor the order of execution.
 *
 * A batch is described by offsets: vertices vend[k] .. vend[k+1]-1, faces tend[k] .. tend[k+1]-1 (K + 1 ints each, on
 * the device), face indices local to their mesh.  Vertices are (V,3) f64.  A "face row" is a face's row in the batch's
 * flat face array.  Everything is f64, one rounding per written operation (the library is built with
 * -ffp-contract=off); division and square root are the correctly rounded ones.  Every dot product is
 * (x0 y0 + x1 y1) + x2 y2.
 *
 * Rule D1, valid faces.  A face takes no part if an index lies outside its object's vertex rows, if a corner is not
 *   finite, or if its area (rule S1 of rfd_sample.h) is exactly 0 or not finite.  The stored triangles hold every
 *   corner as it is, zeros for a corner whose index is out of range.
 * Rule D2, frame.  Object k has lo[k], hi[k] over the corners of its valid faces (0, 0 without any) and R[k] cells per
 *   axis, 1 <= R <= 64.  The HOST computes, in f64 and per axis, inv_h = R / (hi - lo) and h = (hi - lo) / R, both 0 for
 *   an axis of zero extent (such an axis has ONE cell: R_a = 1 where inv_h_a == 0, else R), and
 *   slack = 2^-30 max over the axes of max(hi - lo, |lo|, |hi|); they reach the kernels as (K,3) arrays and a (K) array.
 *   A coordinate's cell is clamp((int)floor((x - lo) * inv_h), 0, R - 1), 0 where the product is a NaN.  The cells of
 *   object k are cbase[k] + (ix R + iy) R + iz; cbase[K] < 2^31.
 *   The default R = clamp(ceil(cbrt(F_valid / 8)), 1, 64) is the host's choice (about 8 faces per cell of a filled
 *   frame), not a tuned value.
 * Rule D3, cell lists.  A triangle belongs to every cell of the index box spanned by its three corners' cells.  One CSR
 *   for the whole batch (count, prefix sum by the caller, fill).  The order inside a cell is whatever the atomics give;
 *   rule D5 makes it irrelevant.
 * Rule D4, closest point of one triangle a, b, c to p (Ericson, Real-Time Collision Detection, 5.1.5).
 *   ab = b - a, ac = c - a;  d1 = ab.(p - a), d2 = ac.(p - a), d3 = ab.(p - b), d4 = ac.(p - b), d5 = ab.(p - c),
 *   d6 = ac.(p - c);  vc = d1 d4 - d3 d2,  vb = d5 d2 - d1 d6,  va = d3 d6 - d5 d4.  The first region that applies:
 *     vertex a:  d1 <= 0 and d2 <= 0:                        q = a
 *     vertex b:  d3 >= 0 and d4 <= d3:                       q = b
 *     vertex c:  d6 >= 0 and d5 <= d6:                       q = c
 *     edge ab:   vc <= 0, d1 >= 0, d3 <= 0:                  t = d1 / (d1 - d3),  q = a + ab t
 *     edge ac:   vb <= 0, d2 >= 0, d6 <= 0:                  t = d2 / (d2 - d6),  q = a + ac t
 *     edge bc:   va <= 0, d4 - d3 >= 0, d5 - d6 >= 0:        t = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  q = b + (c - b) t
 *     interior:  e = 1 / ((va + vb) + vc),  v = vb e,  w = vc e,  q = (a + ab v) + ac w.
 *   The squared distance is ((rx rx + ry ry) + rz rz) with r = p - q.
 * Rule D5, the answer.  Of all valid triangles of the object, the least key (squared distance, face row): a candidate
 *   replaces the best iff its squared distance is smaller, or equal with a lower row; a non-finite one never wins.  An
 *   object without valid faces gives +inf, face -1; a query with a non-finite coordinate (or an object outside
 *   [0, K)) gives NaN, face -1.  The closest point of face -1 is NaN.
 * Rule D6, walk and pruning.  p' = min(max(p, lo), hi) per axis, c = the cell of p'.  Shell r = 0, 1, ... holds the
 *   cells at Chebyshev distance r of c; after shell r everything unvisited lies, on some axis, in cells below c - r or
 *   above c + r.  Per axis and side that still has cells (c - r - 1 >= 0;  c + r + 1 <= R_a - 1) the gap is
 *   p' - (lo + (c - r) h)  and  (lo + (c + r + 1) h) - p';  g = the least of them; no side left: the walk is done.
 *   With o = |p - p'| per axis, every length shortened by slack and clamped at 0 before it is squared:
 *     bound = (((ox^2 + oy^2) + oz^2) + g^2) (1 - 2^-40);   the walk stops iff best < bound.
 *   (|p - x|^2 >= |p - p'|^2 + |p' - x|^2 for x inside the frame; the slack is far above the rounding of the cell
 *   assignment and of the planes, the factor far above that of a squared distance, both far below a cell.)  The walk
 *   only filters: R = 1 is the brute force and every R gives its bits.
 * Rule D7, ragged surface samples: rules S2 - S4 of rfd_sample.h per object.  Object k draws `count` points from its own
 *   face rows with its own inclusive area prefix cum[tend[k] .. tend[k+1]-1] (a face that is not valid counts with
 *   area 0; the prefix's summation order is not part of the contract) and u[k] (count,3).  The face is reported as a face row.  A zero-area face gets the zero normal;
 *   an object without faces gives NaN points, face -1, zero normals.
 * Rule D8, sums per segment.  Segment s holds the entries seg[s] .. seg[s+1]-1, each a squared distance d2 with its
 *   face row and, optionally, a normal n_s.  d = sqrt(d2).  An entry whose d is not finite (or whose face is -1) is
 *   left out and counted.  For the others:  sum d,  sum d2,  sum |n_s . n_f| with n_f the rule-S4 normal of the face,
 *   and for each of T <= 8 thresholds the number of d <= tau_t.  The three f64 sums have decimation's fixed shape:
 *   partial j (0..63) takes the segment's entries j, j + 64, ... in order, starting from 0 (a left-out entry adds
 *   nothing); then partial j += partial j + 32 (j < 32), j + 16 (j < 16), ... , j + 1 (j = 0). */
#ifndef RFD_MESH_DIST_H
#define RFD_MESH_DIST_H
#ifdef __cplusplus
extern "C" {
#endif

/* Two passes over the F faces, one thread per face.
 *   lo == NULL (rule D1):  tri (F,3,3) f64, valid (F) u8 and fobj (F) i32, the face's object, are WRITTEN.
 *   lo != NULL (rule D2):  tri, valid and fobj are READ, and box (F,8) i32 is written: the first and last cell per axis
 *   (x0 x1 y0 y1 z0 z1; x1 < x0 for a face that is not valid), cbase[k] and R[k].
 * Refused: F, K < 0, V < 0, 3 F or 3 V beyond 2^31, K < 1 with F > 0, a null pointer. */
int rfd_mdist_faces(int F, int K, int V, const double *vertices, const int *faces, const int *vend, const int *tend,
                    const double *lo, const double *inv_h, const int *res, const int *cbase, double *tri,
                    unsigned char *valid, int *fobj, int *box, void *stream);

/* The two passes of the cell lists over box (F,8), as rfd_sample_cells.  list == NULL: cursor[cell] += the number of
 * triangles of every cell (the caller clears its cbase[K] entries).  Otherwise cursor holds every cell's first slot and
 * every (cell, triangle) pair takes the next slot of its cell and writes the face row there.  n_cells = cbase[K]: a box
 * that leaves it is skipped. */
int rfd_mdist_cells(int F, const int *box, int n_cells, int *cursor, int *list, void *stream);

/* points (n,3) f64, qobj (n) i32 -> d2 (n) f64, face (n) i32 and, unless null, closest (n,3) f64 (rules D4 - D6).
 * lo, hi, inv_h, h (K,3) f64, slack (K) f64, res (K) i32, cbase (K + 1) i32: rule D2; offsets (cbase[K] + 1) i32 and
 * list: rule D3; tri (F,3,3): rule D1.  One thread per query, best key and shell state in registers.  Refused: n, K,
 * F < 0, 3 n beyond 2^31, a null pointer. */
int rfd_mdist_query(int n, const double *points, const int *qobj, int K, int F, const double *lo, const double *hi,
                    const double *inv_h, const double *h, const double *slack, const int *res, const int *cbase,
                    const int *offsets, const int *list, const double *tri, double *d2, int *face, double *closest,
                    void *stream);

/* Rule D7: u (K,count,3) f64, cum (F) f64 -> points (K,count,3) f64, face (K,count) i32 and, unless null, normals
 * (K,count,3) f64.  Refused: K, count, F < 0, 3 K count beyond 2^31, a null pointer. */
int rfd_mdist_sample(int K, int count, int F, const double *tri, const int *tend, const double *cum, const double *u,
                     double *points, int *face, double *normals, void *stream);

/* Rule D8: seg (S + 1) i32 ascending offsets into d2 (n) f64, face (n) i32 and normals (n,3) f64 (or null: the third
 * sum is 0); tau (T) f64 -> sums (S,3) f64: sum d, sum d2, sum |n_s . n_f|;  counts (S, 1 + T) i32: the entries left
 * out, then the entries with d <= tau_t.  One wave per segment.  Refused: S, n, F, T < 0, T > 8, a null pointer. */
int rfd_mdist_sums(int S, int n, int F, const int *seg, const double *d2, const int *face, const double *normals,
                   const double *tri, int T, const double *tau, double *sums, int *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_MESH_DIST_H */
