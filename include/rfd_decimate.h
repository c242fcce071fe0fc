/* rfd_decimate.h -- mesh decimation by vertex clustering with a quadric-placed representative per cell, for all K
 * meshes of a ragged batch at once (rfdnet_amd/iscnet/decimate.py drives these entries; tests/decimate_f64.py restates
 * the rules in numpy float64 / int64 and the kernels follow its order of operations).  No floating-point atomics, no
 * workgroup waits for another: the result does not depend on the grid, the batch or the order of execution.
 *
 * A batch is described by offsets: vertices vend[k] .. vend[k+1]-1, faces tend[k] .. tend[k+1]-1 (K + 1 ints each, on
 * the device), face indices local to their mesh.  Vertices are (V,3) f64, or f32 with v_is_f32 != 0 (widened: exact).
 * All arithmetic below is f64, one rounding per written operation (the library is built with -ffp-contract=off).
 *
 * Rule 1, cells.  Mesh k has an origin lo[k] (3 f64), a cell size h[k] > 0 and inv_h[k] = 1 / h[k] (made by the
 *   host).  On axis a the cell of a vertex is i_a = clamp(floor((x_a - lo_a) * inv_h), 0, cells - 1): a vertex outside
 *   the cube lands in an edge cell.  Its key is k cells^3 + (iz cells + iy) cells + ix; K cells^3 < 2^31.  A vertex with
 *   a non-finite coordinate belongs to no cell: its key is K cells^3.
 * Rule 2, candidates.  The occupied cells in ascending key order (the host groups the keys: stable sort, unique).
 * Rule 3, position.  Cell centre g_a = lo_a + (i_a + 0.5) * h.  The corners (face, c) whose vertex lies in the cell
 *   are visited in ascending 3 face + c (a face with an index outside its mesh has no corners).  Per corner, with
 *   p0, p1, p2 the face's vertices, u = p1 - p0, v = p2 - p0:
 *     n = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx),  L = sqrt((nx nx + ny ny) + nz nz);  L = 0 or not finite: the
 *     corner is skipped;  w = 0.5 L,  m_a = n_a / L,  d = -((mx (p0x - gx) + my (p0y - gy)) + mz (p0z - gz)),
 *     A_ab += (w m_a) m_b  (xx xy xz yy yz zz),  b_a += (-(w d)) m_a,  W += w,  s_a += w (p_c,a - g_a).
 *   The 13 sums have a fixed shape: partial j (0..15) takes the cell's corners j, j + 16, ... in order, starting from
 *   0; then partial j += partial j + 8 (j < 8), j + 4 (j < 4), j + 2 (j < 2), j + 1 (j = 0).
 *   Solve with l = regularise * W:  mean_a = s_a / W,  A_aa += l,  b_a += l mean_a,  then by cofactors
 *     c00 = Ayy Azz - Ayz Ayz,  c01 = Axz Ayz - Axy Azz,  c02 = Axy Ayz - Axz Ayy,  c11 = Axx Azz - Axz Axz,
 *     c12 = Axy Axz - Axx Ayz,  c22 = Axx Ayy - Axy Axy,  det = (Axx c00 + Axy c01) + Axz c02,
 *     y_x = ((c00 bx + c01 by) + c02 bz) / det,  y_y = ((c01 bx + c11 by) + c12 bz) / det,
 *     y_z = ((c02 bx + c12 by) + c22 bz) / det.
 *   W = 0 gives y = 0, and so does a y_a that is not finite (a determinant that under- or overflowed).  y_a is
 *   clamped to [-h/2, h/2]; the vertex is (float)(g_a + y_a).
 * Rule 4, faces.  A face maps to its corners' candidates.  It is dropped if an index lies outside its mesh, if a
 *   corner has no cell, or if two of its candidates are equal.  Survivors with the same candidate SET are reduced
 *   mod 2: an even count removes all, an odd count keeps the one with the lowest face index.  Order is kept.
 * Rule 5, compaction.  Candidates no kept face names are removed; indices are renumbered in order, local to the
 *   mesh again. */
#ifndef RFD_DECIMATE_H
#define RFD_DECIMATE_H
#ifdef __cplusplus
extern "C" {
#endif

/* Rule 1: key (V) i32.  lo (K,3) f64, inv_h (K) f64 on the device. */
int rfd_decimate_vertex_keys(int V, int K, int cells, int v_is_f32, const void *vertices, const int *vend,
                             const double *lo, const double *inv_h, int *key, void *stream);

/* Rule 4, first half.  vcell (V) i32: the candidate (0 .. C-1) of every vertex, -1 for none.
 *   fcell (F,3) i32: the candidate of every corner, -1 for a corner without a cell, all three -1 for a face with an
 *   index outside its mesh (what the corner lists of rule 3 are made of);  alive (F) u8: not dropped;  for an alive
 *   face with candidates a < b < c:  pair (F) i64 = a C + b,  top (F) i32 = c  (0 for a dropped one). */
int rfd_decimate_face_remap(int F, int K, int C, const int *faces, const int *tend, const int *vend, const int *vcell,
                            int *fcell, long long *pair, int *top, unsigned char *alive, void *stream);

/* Rule 4, second half, over the n alive faces sorted by (pair, top) with ascending face index inside a run
 *   (s_pair, s_top, s_face): the first face of every run of odd length gets keep[face] = 1 and its three candidates
 *   used[c] = 1.  keep (F) u8 and used (C) i32 are zero on entry. */
int rfd_decimate_parity(int n, int C, int F, const long long *s_pair, const int *s_top, const int *s_face,
                        const int *fcell, unsigned char *keep, int *used, void *stream);

/* Rule 3 for every candidate with dst[cell] >= 0:  out[dst[cell]] (3 f32).  cellkey (C) i32;  rowptr (C + 1) / col:
 *   the corners 3 face + c (face counted over the whole batch) of every candidate, ascending;  h, lo as in rule 1.
 *   Sixteen lanes per cell hold the sixteen partial sums. */
int rfd_decimate_cell_solve(int C, int K, int F, int cells, int v_is_f32, const void *vertices, const int *faces,
                            const int *vend, const int *cellkey, const int *rowptr, const int *col, const int *dst,
                            const double *lo, const double *h, double regularise, float *out, void *stream);

/* Rule 5 for the faces:  f2[fincl[f] - 1][c] = (vincl[fcell[f][c]] - 1) - vend2[k] for every kept face f of mesh k.
 *   fincl (F) / vincl (C) i32: the inclusive prefix sums of keep / used;  vend2 (K + 1) i32: the new vertex offsets. */
int rfd_decimate_compact_faces(int F, int K, const int *tend, const int *fcell, const unsigned char *keep,
                               const int *fincl, const int *vincl, const int *vend2, int *f2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_DECIMATE_H */
