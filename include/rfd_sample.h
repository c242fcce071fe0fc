/* rfd_sample.h -- occupancy samples from a closed mesh (the reference's utils/shapenet/2_sample_mesh.py): is a point
 * inside the mesh (external/libmesh: inside_mesh.py, triangle_hash.pyx), which voxels does the surface touch
 * (external/libvoxelize: voxelize.pyx, tribox2.h), and points drawn uniformly from the surface (trimesh's sample).  The
 * first two follow the reference's arithmetic operation by operation and give its bits (tests/golden/F_SMP.npz); the
 * third is this project's own contract.  All three are restated in numpy in tests/mesh_sample_ref.py.
 *
 * Containment.  Everything is float64, evaluated left to right as written, no fused multiply-add.
 *
 * Rule C1, rescale constants.  The triangles are vertices[faces] as f64.  bmin / bmax run over the 3F referenced corners
 *   only.  The HOST computes, in float64, scale = (res - 1) / (bmax - bmin) and translate = 0.5 - scale * bmin per axis;
 *   they reach the kernels as six doubles.
 * Rule C2, rescale.  Every triangle corner and every point is x' = scale * x + translate: one multiply, one add.
 * Rule C3, candidates.  A point is a candidate iff 0 <= x' <= res on all three axes and (int)x' < res and (int)y' < res
 *   (together: 0 <= x', y' < res and 0 <= z' <= res); a NaN fails.  Its cell is res * (int)x' + (int)y'.  A triangle
 *   belongs to the cells of its 2-D bounding box: (int) of the minimum and of the maximum of its rescaled corners per
 *   axis, clamped to [0, res - 1].  The cells only filter: a triangle that passes rule C4 for a point always lies in
 *   the point's cell, so the result does not depend on them.
 * Rule C4, the 2-D test, per triangle with rescaled corners t1, t2, t3 and point p:
 *   A00 = t1x - t3x, A10 = t1y - t3y, A01 = t2x - t3x, A11 = t2y - t3y;  det = A00 A11 - A01 A10; det == 0: no hit.
 *   s = sign(det), ad = |det|, y0 = px - t3x, y1 = py - t3y;
 *   u = (A11 y0 - A01 y1) s,  v = (-A10 y0 + A00 y1) s,  w = u + v;   hit iff 0 < u < ad, 0 < v < ad and 0 < w < ad.
 * Rule C5, the side, for a hit:  v1 = t3 - t1, v2 = t2 - t1, n = v1 x v2 (every component a b - c d);
 *   alpha = n0 (t1x - px) + n1 (t1y - py).  n2 == 0: the hit counts nowhere.  Otherwise depth = t1z |n2| + alpha sign(n2)
 *   and rhs = pz |n2|:  depth >= rhs adds to n0, depth < rhs adds to n1.
 * Rule C6.  contains = (n0 odd) and (n1 odd).
 *
 * Surface voxels.  Everything is float32, evaluated as written.
 *
 * Rule V1.  The corners are ((vertices + 0.5) * R)[faces] in f64, rounded once to f32 (the caller's work).
 * Rule V2.  A triangle's box is, per axis, (int) of the f32 minimum and maximum of its corners, clamped to [0, R - 1].
 * Rule V3.  For every voxel (i, j, k) of the box: triBoxOverlap with centre (i + .5, j + .5, k + .5) and half size .5:
 *   v0, v1, v2 = corner - centre;  e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2.  With (a, b) a pair of components of an
 *   edge and fa = |a|, fb = |b|, an axis test forms two projections pA, pB, takes their min and max, and fails (no
 *   overlap) iff min > rad || max < -rad with rad = fa * .5 + fb * .5.  The nine, in this order:
 *     edge 0:  X: a = e0z, b = e0y, p = a y - b z of v0 and v2;  Y: a = e0z, b = e0x, p = -a x + b z of v0 and v2;
 *              Z: a = e0y, b = e0x, p = a x - b y of v1 and v2;
 *     edge 1:  X of v0 and v2;  Y of v0 and v2;  Z of v0 and v1;
 *     edge 2:  X of v0 and v1;  Y of v0 and v1;  Z of v1 and v2.
 *   (X's rad is fa (of z) * .5 + fb (of y) * .5, Y's fa (of z) and fb (of x), Z's fa (of y) and fb (of x).)
 *   Then per axis x, y, z: min and max of the three v fail iff min > .5 || max < -.5.
 *   Then the plane: n = e0 x e1, d = -((n0 v0x + n1 v0y) + n2 v0z);  per axis vmin = n > 0 ? -.5 : .5, vmax = -vmin;
 *   ((n0 vmin0 + n1 vmin1) + n2 vmin2) + d > 0 fails;  otherwise overlap iff ((n0 vmax0 + n1 vmax1) + n2 vmax2) + d >= 0.
 * Rule V4.  A voxel is set if any triangle overlaps it.
 *
 * Surface samples (this project's rules; trimesh's scheme is the model).  Everything is float64.
 *
 * Rule S1.  area_f = 0.5 sqrt((cx^2 + cy^2) + cz^2) with c = (t1 - t0) x (t2 - t0).
 * Rule S2.  cum is the inclusive prefix of the areas (its summation order is NOT part of the contract);
 *   total = cum[F-1], t = u0 total; the face is the first f with cum[f] >= t (binary search), clamped to F - 1.
 * Rule S3.  a = u1, b = u2; if a + b > 1 then a = |a - 1|, b = |b - 1|;
 *   p = t0 + ((t1 - t0) a + (t2 - t0) b) per component.
 * Rule S4.  The normal is c / sqrt((cx^2 + cy^2) + cz^2), the zero vector for a face of area 0. */
#ifndef RFD_SAMPLE_H
#define RFD_SAMPLE_H
#ifdef __cplusplus
extern "C" {
#endif

/* tri (F,3,3) f64 -> rescaled (F,3,3) f64 (rule C2) and box (F,4) i32: x0, x1, y0, y1, the cells of rule C3.  One thread
 * per triangle.  Refused: F < 0, res < 2 or res > 32768. */
int rfd_sample_rescale(int F, const double *tri, double sx, double sy, double sz, double tx, double ty, double tz,
                       int res, double *rescaled, int *box, void *stream);

/* The two passes of the cell lists over box (F,4).  list == NULL: cursor (res^2) i32 += the number of triangles of every
 * cell (the caller clears it).  Otherwise cursor holds every cell's first slot, and every (cell, triangle) pair takes
 * the next slot of its cell and writes the triangle there.  The order inside a cell is whatever the atomics give; only
 * parities are read from it.  A workgroup works through 64 triangles, all its threads on one triangle's cells at a time,
 * and the cells of a triangle are dealt over gridDim.y workgroups, so a triangle that covers every cell costs no lane
 * more than 128 atomics. */
int rfd_sample_cells(int F, const int *box, int res, int *cursor, int *list, void *stream);

/* points (n,3) f64 -> contains (n) u8 and, unless null, n0, n1 (n) i32 (rules C2 - C6).  offsets (res^2 + 1) i32 and
 * list are the cell lists, rescaled the triangles of rfd_sample_rescale.  One thread per point, counters in registers. */
int rfd_sample_contains(int n, const double *points, double sx, double sy, double sz, double tx, double ty, double tz,
                        int res, int F, const double *rescaled, const int *offsets, const int *list,
                        unsigned char *contains, int *n0, int *n1, void *stream);

/* tri (F,3,3) f32 in voxel units (rule V1) -> grid (R,R,R) u8, set to 1 where a triangle overlaps (rules V2 - V4); the
 * caller clears it.  The split is that of rfd_sample_cells: (triangle, slab of its box).  Refused: R < 1 or R > 1024. */
int rfd_sample_voxelize(int F, const float *tri, int R, unsigned char *grid, void *stream);

/* tri (F,3,3) f64 -> area (F) f64 (rule S1) */
int rfd_sample_face_areas(int F, const double *tri, double *area, void *stream);

/* u (count,3) f64, cum (F) f64 -> points (count,3) f64, face (count) i32 and, unless null, normals (count,3) f64
 * (rules S2 - S4).  Refused: F < 1 with count > 0. */
int rfd_sample_surface(int count, int F, const double *tri, const double *cum, const double *u, double *points,
                       int *face, double *normals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_SAMPLE_H */
