/* rfd_fuse.h -- the two device stages between the rasteriser and marching cubes that turn a triangle soup into a
 * watertight mesh (the reference's utils/shapenet/1_fuse_shapenetv2.py: depth maps from views on a sphere, fused into a
 * truncated signed distance field): rfd_depth_from_keys makes one depth map out of the rasteriser's key buffer,
 * rfd_tsdf_fuse fuses a stack of depth maps into a volume.  The fusion's rules are those of the reference's
 * external/pyfusion (fusion.h, fusion.cpp), spelled out; given the same depth maps it gives the same bits.  They are
 * restated in numpy in tests/fuse_ref.py.
 *
 * Everything below is f32 unless said otherwise, evaluated as written (no fused multiply-add), divisions are IEEE.
 *
 * Rule 1, voxel centre.  Voxel (d, h, w) of the volume (D,H,W) has x = (float)((w + 0.5) * (double)vx_size - 0.5),
 *   y the same from h and z from d.
 * Rule 2, projection, per view v in the order 0 .. V-1, with R, K (row order) and T of that view:
 *   xt = ((R0 x + R1 y) + R2 z) + T0, yt and zt likewise from rows 1 and 2 of R;
 *   u = (K0 xt + K1 yt) + K2 zt, v and dd likewise from rows 1 and 2 of K;  u = u / dd, v = v / dd.
 * Rule 3, pixel.  tu = u + 0.5f, tv = v + 0.5f.  The voxel is on the image iff tu > -1 && tu < cols && tv > -1 &&
 *   tv < rows: comparisons of floats, which a NaN fails, decided BEFORE any conversion to an integer (wherever C defines
 *   the reference's `int(tu) >= 0 && int(tu) < cols` it is the same test).  The pixel is then row (int)tv, column (int)tu.
 *   No index is formed from a float that has not passed the test.
 * Rule 4, sample.  g = depth[v][row][column]; if unknown_is_free and g < 0 then g = 1e9f; dist = g - dd.  The sample is
 *   valid iff g > 0 && dist >= -truncation (a NaN depth is never valid); a valid sample adds
 *   fminf(truncation, fmaxf(-truncation, dist)) to the voxel's sum and 1 to its count.  The sum runs in view order.
 * Rule 5, result.  tsdf = sum / (float)count where count > 0, else unobserved_value.  The reference's tsdf_gpu is
 *   unobserved_value = -truncation and its tsdfmask_gpu is count > 0; the field its pipeline goes on with (the mask
 *   applied) is unobserved_value = +truncation, here in one pass.
 *
 * Rule 6, depth from keys (the per-view post-processing of the reference's render(), on the key buffer that
 *   rfd_raster_triangles left, include/rfd_render.h rule 3): a pixel with key 0 has z = far, any other
 *   z = (float)(1 / (double)invz) with invz the f32 in the key's high word, and z = far where z > far;  e = z - offset;
 *   depth = the minimum of e over the pixel's 3x3 neighbourhood cut at the image border (scipy's grey_erosion of size
 *   (3,3) with its `reflect` border, which is the edge-clamped minimum). */
#ifndef RFD_FUSE_H
#define RFD_FUSE_H
#ifdef __cplusplus
extern "C" {
#endif

/* keys (H,W) u64 -> depth (H,W) f32 (rule 6), one thread per pixel.  Refused: W or H outside 1..8192. */
int rfd_depth_from_keys(int W, int H, const unsigned long long *keys, float far, float offset, float *depth,
                        void *stream);

/* depth (V,rows,cols) f32, K (V,9), R (V,9), T (V,3) f32, all on the device -> tsdf (D,H,W) f32 and, unless it is a
 * null pointer, count (D,H,W) i32 (rules 1-5).  One thread per voxel with the view loop inside; a wave owns a brick of
 * 4x4x4 voxels.  view_chunk: 0 = the library's choice, c > 0 = one launch per c views, which carries sum and count
 * through tsdf and count between the launches, in view order, so the bits are those of one launch (without `count` there
 * is nowhere to carry the count: the views then run in one launch).  V = 0 is valid: unobserved_value everywhere.
 * Refused, before anything is launched: a negative V, D, H, W or view_chunk, rows or cols outside 1..8192,
 * D H W or V rows cols beyond 2^31 - 1, a null pointer for an array that would be read or written. */
int rfd_tsdf_fuse(int V, int rows, int cols, const float *depth, const float *K, const float *R, const float *T, int D,
                  int H, int W, float vx_size, float truncation, int unknown_is_free, float unobserved_value,
                  int view_chunk, float *tsdf, int *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_FUSE_H */
