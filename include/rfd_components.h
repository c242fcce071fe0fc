/* rfd_components.h -- connected components of all K meshes of a ragged batch at once: label the faces, measure every
 * component, keep the largest (or every one above a fraction of it) and compact the batch
 * (rfdnet_amd/iscnet/components.py drives these entries; tests/components_f64.py restates the rules in numpy float64 /
 * Python int and the kernels follow its order of operations).  The labelling is a lock-free union-find whose fixed
 * point is unique; the sums have a fixed shape.  No floating-point atomics, no workgroup waits for another: the result
 * does not depend on the grid, the batch or the order of execution.
 *
 * A batch is described by offsets as in rfd_decimate.h: vertices vend[k] .. vend[k+1]-1, faces tend[k] .. tend[k+1]-1
 * (K + 1 ints each, on the device), face indices local to their mesh.  Vertices are (V,3) f64, or f32 with
 * v_is_f32 != 0 (widened: exact).  All arithmetic below is f64, one rounding per written operation (the library is
 * built with -ffp-contract=off).
 *
 * Rule 1, valid faces.  A face of mesh k is valid if its three indices lie in [0, vend[k+1] - vend[k]).  An invalid
 *   face belongs to no component (label -1) and is never kept.  A face with a repeated index, or of zero area, is valid.
 * Rule 2, connectivity.  Two valid faces of one mesh are connected if they name a common vertex index; components are
 *   the transitive closure.  Positions play no part: two sheets that touch in space but share no index are two
 *   components, a triangle soup is one component per face.  A vertex no valid face names is in no component.
 * Rule 3, numbering.  The components of mesh k are numbered 0 .. n_k - 1 in ascending order of the smallest vertex
 *   index they name.  The global id is cbase[k] + local, cbase the prefix sum of the n_k, C = cbase[K].
 * Rule 4, measures, per component.  Its faces are visited in ascending face index.  Per face, with p0, p1, p2 its
 *   vertices:  n = (p1 - p0) x (p2 - p0),  L = sqrt((nx nx + ny ny) + nz nz)  (cross, dot of csrc/mesh_batch.h),
 *     a = 0.5 L if L is not 0 and finite, else 0;   t = dot(p0, p1 x p2) if finite, else 0.
 *   Both sums have the fixed shape of rfd_decimate.h rule 3: partial j (0..15) takes the component's faces j, j + 16,
 *   ... in order, starting from 0; then partial j += partial j + 8 (j < 8), j + 4 (j < 4), j + 2 (j < 2), j + 1 (j = 0).
 *     area = sum a,   volume = (sum t) / 6.0  (signed; it means something for a closed component only, and is reported
 *   for all).  Per axis, lo / hi are the min / max over the finite coordinates of the component's corners (+inf / -inf
 *   if there are none).  faces and vertices are integer counts.
 * Rule 5, selection, per mesh, on a measure m: faces (as f64), area, or abs_volume = |volume|.  The largest component
 *   is the first one, replaced by every later one whose m is greater: the greatest m, the lowest id among equals.
 *   Mode largest keeps it alone.  Mode fraction t (0 <= t <= 1) keeps the largest and every component with
 *   m >= t * m_largest (one multiply, one compare): t = 0 keeps all.  drop_cavities additionally drops every component
 *   other than the largest with volume * volume_largest < 0 (an inside-out shell).  A mesh without components stays
 *   empty.
 * Rule 6, compaction.  Kept faces stay in their order, the vertices they name stay in their order, coordinates are
 *   copied bit for bit in the input's type, indices are renumbered local to the mesh. */
#ifndef RFD_COMPONENTS_H
#define RFD_COMPONENTS_H
#ifdef __cplusplus
extern "C" {
#endif

#define RFD_COMPONENTS_BY_FACES 0
#define RFD_COMPONENTS_BY_AREA 1
#define RFD_COMPONENTS_BY_ABS_VOLUME 2

/* Rule 2: parent (V) i32 over the GLOBAL vertex indices, parent[i] = i on entry.  One thread per valid face unites its
 *   corners; on return every set is a tree whose root is its smallest index. */
int rfd_components_union(int F, int K, int V, const int *faces, const int *tend, const int *vend, int *parent,
                         void *stream);

/* root[i] = the root of i in parent (V) i32: a launch of its own, so that every link of the union is visible.  parent's
 *   paths are shortened on the way; its roots stay. */
int rfd_components_flatten(int V, int *parent, int *root, void *stream);

/* Rules 1 and 3, first half.  froot (F) i32: the root of the face's corners, -1 for an invalid face;  corner (F,3) i32:
 *   its GLOBAL vertex indices, -1 -1 -1 for an invalid face;  is_root (V) i32 and named (V) i32, zero on entry: 1 for
 *   the roots valid faces name and for the vertices they name. */
int rfd_components_face_roots(int F, int K, int V, const int *faces, const int *tend, const int *vend, const int *root,
                              int *froot, int *corner, int *is_root, int *named, void *stream);

/* Rule 3, second half.  rincl (V) i32: the inclusive prefix sum of is_root;  cbase (K + 1) i32
 *   -> glabel (F) / llabel (F) i32: the global / local id of every face, -1 for an invalid one;  vlabel (V) i32: the
 *   global id of every named vertex, -1 for the others. */
int rfd_components_labels(int F, int K, int V, const int *froot, const int *root, const int *named, const int *rincl,
                          const int *tend, const int *cbase, int *glabel, int *llabel, int *vlabel, void *stream);

/* Rule 4 for all C components.  rowptr (C + 1) / col: the faces of every component, ascending;  corner as above
 *   -> faces (C) i32, area (C) f64, volume (C) f64, lo (C,3) f64, hi (C,3) f64.  Sixteen lanes per component hold the
 *   sixteen partial sums. */
int rfd_components_measure(int C, int F, int V, int v_is_f32, const void *vertices, const int *corner, const int *rowptr,
                           const int *col, int *faces, double *area, double *volume, double *lo, double *hi,
                           void *stream);

/* Rule 5, one thread per mesh.  measure: RFD_COMPONENTS_BY_*;  largest_only != 0: mode largest, else mode fraction t
 *   -> keep_comp (C) u8, kept (K) i32: how many components of every mesh stay. */
int rfd_components_select(int K, int C, int measure, int largest_only, double t, int drop_cavities, const int *cbase,
                          const int *faces, const double *area, const double *volume, unsigned char *keep_comp,
                          int *kept, void *stream);

/* Rule 6, the flags: keep (F) u8 = the face's component stays;  used (V) i32, zero on entry: 1 for the vertices kept
 *   faces name. */
int rfd_components_mark(int F, int C, int V, const int *glabel, const int *corner, const unsigned char *keep_comp,
                        unsigned char *keep, int *used, void *stream);

/* Rule 6 for the faces:  f2[fincl[f] - 1][c] = (vincl[corner[f][c]] - 1) - vend2[k] for every kept face f of mesh k.
 *   fincl (F) / vincl (V) i32: the inclusive prefix sums of keep / used;  vend2 (K + 1) i32: the new vertex offsets. */
int rfd_components_compact_faces(int F, int K, int V, const int *tend, const int *corner, const unsigned char *keep,
                                 const int *fincl, const int *vincl, const int *vend2, int *f2, void *stream);

/* Rule 6 for the vertices:  row vincl[i] - 1 of v2 = row i of vertices for every used vertex i, bit for bit
 *   (3 f32 if v_is_f32, else 3 f64);  V2: the rows of v2. */
int rfd_components_gather_vertices(int V, int V2, int v_is_f32, const void *vertices, const int *used, const int *vincl,
                                   void *v2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_COMPONENTS_H */
