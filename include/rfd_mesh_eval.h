/* rfd_mesh_eval.h -- mesh IoU of every (prediction, ground truth) pair of a scene on per-object voxel grids: the
 * piece between the voxeliser (rfd_sample.h) and the matching (rfd_eval.h: rfd_ap_match) that mesh mAP needs.
 *
 * Device counterpart of the reference's
 *   net_utils/eval_det.py:27-83     compute_mesh_iou (one Python call per pair, over a process pool)
 *   net_utils/ap_helper.py:429-478  the per-object voxel grids it is fed
 * Every object has a grid of its own -- its own origin, cell size and dimension -- and the filled voxel centres of
 * one object are looked up in the other object's grid, both ways.
 *
 * Rules.  Everything is float64, evaluated left to right as written; the library is built with -ffp-contract=off.
 *   M1 frame.   lo, hi: per-axis min / max over the placed vertices of the object.  L = max(hi - lo),
 *               D = max((int)(L / voxel_size), 2) (voxel_size 0.047 by default, ap_helper.py:438-439), cell = L / D.
 *               The grid is the cube [lo, lo + L]^3, anchored at lo on every axis.  L not finite, L == 0 or no faces:
 *               the object has no grid (D = 0 in the table) and every IoU with it is 0.  D > 256 is refused on the host.
 *   M2 grids.   vertices mapped to the unit cube by (v - lo) / L - 0.5; S = the surface voxels, I = the voxels whose
 *               centre is inside the mesh (rfd_sample.h, rules V1 - V4 and C1 - C6, no jitter); U = S | I.
 *   M3 centre.  voxel (i,j,k) of object A has the world centre lo_A + (idx + 0.5) * cell_A, per axis.
 *   M4 lookup.  a world point p is filled in object B iff per axis q = (p - lo_B) / cell_B, t = floor(q) satisfy
 *               0 <= t < D_B, and bit t of U_B is set.  A NaN fails.
 *   M5 IoU.     n_A = |U_A|, a_AB = #{v in U_A : centre_A(v) filled in B}; n_B, a_BA likewise.  0 if |S_A| == 0,
 *               |S_B| == 0, a_AB == 0 or a_BA == 0; otherwise a1 = a_AB / n_A, a2 = a_BA / n_B and
 *               iou = (a1 * a2) / (a1 + a2 - a1 * a2)   (eval_det.py:27-83; its four branches are this one formula).
 * Deviations from the reference:
 *   - M2's S and I stand in for binvox's `exact` and `wireframe + dilated_carving` grids.  binvox is an external
 *     program; its carving is not reproducible here and is not attempted.
 *   - M4 is `floor`, not trimesh's `round` about the voxel centre.  The two differ only for a point exactly on a cell
 *     boundary (and there by which of the two cells takes it); with floor the lo face of a grid is inside and the
 *     lo + L face is outside.
 *
 * Layout.  U is stored as bit words: 64 bits along z (bit k & 63 of word k >> 6), W = ceil(D / 64) words per (i,j) row,
 * row i * D + j; an object's D * D * W words start at its word offset in a buffer shared by a set of objects.
 * Object table, one row per object: frame (4) f64 = lo[3], cell; dim i32 = D (0: no grid); off i64 = the word
 * offset; cnt (2) i32 = |U|, |S|.
 * Every function takes a trailing stream and returns a hipError_t value (0 = success). */
#ifndef RFD_MESH_EVAL_H
#define RFD_MESH_EVAL_H
#ifdef __cplusplus
extern "C" {
#endif

/* S, I (D,D,D) u8 (non-zero = filled) of ONE object -> its D * D * W words at words[off ..] and
 * cnt[0] += |U|, cnt[1] += |S| (cnt must be zero on entry: one integer add per workgroup, after a wave popcount).
 * 2 <= D <= 256, 0 <= off, off + D * D * W <= n_words, else hipErrorInvalidValue (nothing is launched). */
int rfd_objgrid_pack(int D, const unsigned char *S, const unsigned char *I, unsigned long long *words,
                     long long off, long long n_words, int *cnt, void *stream);

/* counts (P,G,2) i32 out: a_AB (A = prediction p, B = ground truth g) and a_BA; every element is written.
 * One workgroup per (pair, direction).  A pair with an object without grid, or whose two cubes do not overlap,
 * writes 0 and returns.  Otherwise the source's index box is clipped to what can fall into the target's cube
 * (conservatively, by a cell; M4 decides), each lane takes 64-bit source words and for every set bit evaluates M3
 * and M4; wave reduction, LDS reduction, one store.  Integers: the same on every run.
 * A table row is taken as "no grid" unless 2 <= D <= 256, its frame is finite with cell > 0 and its words lie
 * inside [0, n_words).  0 <= P <= 1024, 0 <= G <= 256 (rfd_ap_match's limits), else hipErrorInvalidValue
 * (nothing is launched); P == 0 or G == 0: success without a launch. */
int rfd_mesh_iou_counts(int P, int G,
                        const double *frame_p, const int *dim_p, const long long *off_p,
                        const unsigned long long *words_p, long long n_words_p,
                        const double *frame_g, const int *dim_g, const long long *off_g,
                        const unsigned long long *words_g, long long n_words_g,
                        int *counts, void *stream);

/* M5 for every pair, scattered: iou[rows_p[p] * G_out + rows_g[g]] = the IoU of (p, g); rows_p / rows_g (P) / (G)
 * i32 or NULL for the identity; a row outside [0, K_out) x [0, G_out) is skipped.  iou (K_out,G_out) f64 is NOT
 * cleared: every other element stays what it was.  cnt_p (P,2), cnt_g (G,2): |U|, |S| of the tables.
 * Limits as rfd_mesh_iou_counts, K_out and G_out >= 0. */
int rfd_mesh_iou_finalize(int P, int G, const int *counts, const int *cnt_p, const int *cnt_g,
                          const int *rows_p, const int *rows_g, int K_out, int G_out, double *iou, void *stream);

/* ---- The ragged batch: M1 - M2 for ALL N objects of a scene in a number of launches that does not depend on N
 * (csrc/objgrid.hip; restated in numpy in tests/objgrid_ref.py).  The result is what the per-object path
 * (mesh_sample's voxelisers, then rfd_objgrid_pack per object) gives: rules M1 - M2 above and C1 - C6 / V1 - V4 of
 * rfd_sample.h, applied per object.  New is how the lattice is walked and how triangles are filtered.  Float64 unless
 * stated, left to right as written, no fused multiply-add.
 *   B1 frames.   On the host, from one read-back: M1 per object gives lo, L, D, cell; the unit map is
 *                (v - lo) / L - 0.5 for all objects at once.  An object has a grid iff it has vertices and faces and M1
 *                yields a frame.  Triangles of an object without a grid are read by no kernel.
 *   B2 surface.  V1: the corners are ((u + 0.5) * D_k)[faces] in f64, rounded once to f32; D_k enters as a double.
 *                V2 - V4 with R = D_k of the triangle's object.  A set voxel (i, j, z) sets bit z & 63 of word
 *                off_k + (i * D + j) * W + (z >> 6) of the surface words S.
 *   B3 constants.  C1 at res = 512 per object, on the bounding box of the object's referenced corners in the unit cube:
 *                host, float64, from the same read-back, uploaded as a table (N,6) = scale[3], translate[3].  An object
 *                whose box lacks positive extent on some axis has I = 0; its row holds zeros, and a row whose scale is
 *                not positive on every axis has no interior.  A scale or translate that is not finite is refused on the
 *                host.
 *   B4 lattice.  The coordinate of index i on any axis is c_i = (i + 0.5) / D - 0.5 (one division, one subtraction) and
 *                its image is p' = s * c_i + t (C2).  Column (i, j) is a candidate iff 0 <= px' < 512 and 0 <= py' < 512;
 *                a z index is a candidate iff 0 <= pz' <= 512; both decided on the doubles before any conversion.
 *   B5 parity.   A triangle that passes C4 for (px', py') and has n2 != 0 yields depth (C5).  For every candidate z,
 *                rhs = pz'_z * |n2|: depth >= rhs toggles bit z of P0, depth < rhs toggles bit z of P1, a NaN toggles
 *                neither.  I = P0 & P1.  The order in which a column meets its triangles is free.
 *   B6 filter.   A column looks only at triangles whose C3 cell box contains the column's cell ((int)px', (int)py'), or
 *                at any superset of them (C3: the cells only filter).  Here: per object 32 x 32 bins, bin = cell >> 4 per
 *                axis; a triangle goes into the bins of its C3 box shifted the same way; the lists are a CSR over all
 *                N * 1024 bins (bin index (k * 32 + bx) * 32 + by) built in two passes of integer atomics, the prefix
 *                between them is the caller's.  No per-object res^2 array.
 *   B7 union.    U = S | I word by word; cnt[k] = (popcount U, popcount S) by integer adds.
 *
 * The table.  dim (N) i32 (0: no grid), off (N) i64, both ALSO as host arrays (dim_host, off_host): every launcher reads
 * the host copy and refuses -- hipErrorInvalidValue, nothing launched -- a negative count, N > 65535, a null pointer it
 * needs, a dim outside {0} and [2, 256], and off < 0 or off + D * D * W > n_words.  The kernels check the device rows and
 * face_obj again: a row out of range is an object without a grid, a face of no such object is skipped.  F == 0, N == 0
 * or no object with a grid: success without a launch.  The four entries are declared in rfd_objgrid.h. */

#ifdef __cplusplus
}
#endif
#endif /* RFD_MESH_EVAL_H */
