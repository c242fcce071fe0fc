/* rfd_objgrid.h -- the voxel grids of all objects of a scene in one ragged batch: the entries of csrc/objgrid.hip.
 * The rules B1 - B7, the layout of the words, the object table and what every launcher refuses are written out in
 * rfd_mesh_eval.h (section "The ragged batch"); tests/objgrid_ref.py restates them in numpy.
 * Every function takes a trailing stream and returns a hipError_t value (0 = success). */
#ifndef RFD_OBJGRID_H
#define RFD_OBJGRID_H
#ifdef __cplusplus
extern "C" {
#endif

/* tri (F,3,3) f32: rule B2's corners, face_obj (F) i32 -> bits of words (n_words) u64 set by integer atomicOr; the
 * caller clears words.  64 triangles per workgroup staged in LDS, one triangle's box of voxels dealt over the workgroup
 * and over gridDim.y. */
int rfd_objgrid_surface(int F, const float *tri, const int *face_obj, int N, const int *dim_host,
                        const long long *off_host, const int *dim, const long long *off, long long n_words,
                        unsigned long long *words, void *stream);

/* The two passes of rule B6 over tri (F,3,3) f64 in the unit cube and consts (N,6) f64.  list == NULL: cursor
 * (N * 1024) i32 += the number of triangles of every bin (the caller clears it).  Otherwise cursor holds every bin's
 * first slot and every (bin, triangle) pair takes the next slot of its bin and writes the triangle there; a slot outside
 * [0, n_pairs) is not written. */
int rfd_objgrid_bins(int F, const double *tri, const int *face_obj, int N, const int *dim_host, const int *dim,
                     const double *consts, int *cursor, int *list, int n_pairs, void *stream);

/* Rules B4 - B5: offsets (N * 1024 + 1) i32 and list (n_pairs) i32 are the bin lists -> inter (n_words) u64, the words
 * of I; whole words are stored, and only those of candidate columns (the caller clears inter).  One wave per column:
 * a lane per triangle of the list for C4 / C5, then a lane per z for the parities; the ballot is the word. */
int rfd_objgrid_interior(int F, const double *tri, int N, const int *dim_host, const long long *off_host,
                         const int *dim, const long long *off, long long n_words, const double *consts,
                         const int *offsets, const int *list, int n_pairs, unsigned long long *inter, void *stream);

/* Rule B7: words |= inter, cnt (N,2) i32 += |U|, |S| (cnt must be zero on entry) */
int rfd_objgrid_finish(int N, const int *dim_host, const long long *off_host, const int *dim, const long long *off,
                       long long n_words, unsigned long long *words, const unsigned long long *inter, int *cnt,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_OBJGRID_H */
