/* rfd_render.h -- a depth-tested rasteriser for the placed scene (demo.py:329-377 renders it through VTK): triangles
 * of the object meshes and the scan's points, one image per call, on the device the meshes live on.
 *
 * An image costs one clear (of the key buffer) and three launches: rfd_raster_project, rfd_raster_triangles (which
 * draws the scan points in the same launch, rule 4) and rfd_raster_shade.  Only atomicMax on 64-bit
 * words; no workgroup waits for another; the result does not depend on the order of execution.
 *
 * camera: 16 doubles on the host, m[0..11] the 3x4 world-to-view matrix in row order (view frame: x right, y down,
 * z forward), then fx, fy, cx, cy in pixels.  Pixel (i, j) (column, row) has its centre at (i + 0.5, j + 0.5).
 *
 * Rule 1, projection, in f64, no fused multiply-add, for a point (X, Y, Z) (f32, widened):
 *   xv = ((m0 X + m1 Y) + m2 Z) + m3,  yv and zv likewise from rows 1 and 2;  q = 1 / zv;
 *   sx = (fx xv) q + cx,  sy = (fy yv) q + cy;  ix = floor(256 sx + 0.5), iy likewise (int32: 1/256 pixel).
 * Rule 2, validity, decided before any conversion to an integer: a point is valid iff X, Y, Z are finite, zv >= near and
 *   |sx| <= 2^20 and |sy| <= 2^20 (comparisons that a NaN fails).  An invalid vertex removes every triangle that uses
 *   it, and so does a vertex index outside [0, V); nothing is clipped.
 * Rule 3, triangles.  With the pixel centre P = (256 i + 128, 256 j + 128) and int64 arithmetic on the snapped
 *   coordinates, E_0 = (x2 - x1)(Py - y1) - (y2 - y1)(Px - x1), E_1 and E_2 the same for the edges 2->0 and 0->1,
 *   A = E_0 + E_1 + E_2 (the same at every pixel; |E| < 2^60).  A = 0: the triangle covers nothing.  A < 0: every E and
 *   every edge vector is negated (no culling).  The pixel is covered iff for every edge E > 0, or E = 0 and the edge
 *   vector (dx, dy) has dy < 0 or (dy = 0 and dx > 0): the top-left rule.  There, in f64,
 *   w_i = (double)E_i / (double)A,  invz = (float)((w_0 q_0 + w_1 q_1) + w_2 q_2),
 *   and atomicMax(key[j][i], ((u64)bits(invz) << 32) | (0xffffffff - f)).  The key buffer is cleared to 0.
 *   The bounding box is clamped to the image first; a box of more than 64 pixels is walked by the whole workgroup.
 * Rule 4, points.  Scan point n is the square of point_px x point_px pixels (odd, 1..63) centred on the pixel
 *   (ix >> 8, iy >> 8), cut at the image border, with invz = (float)q and the primitive index F + n.
 * Rule 5, shading, one thread per pixel.  key = 0: ids -1, depth +inf, white.  Otherwise prim = 0xffffffff - low word,
 *   depth = (float)(1 / (double)invz), ids = prim, and in f32: a scan point is the grey 0.55; a face with the (placed, f32)
 *   corners a, b, c has n = (b - a) x (c - a), g = ((a + b) + c) / 3, v = eye - g,
 *   s = 0.3 + 0.7 |n . v| / (sqrt(n . n) sqrt(v . v))  (0.3 where that is not a number), colour = palette[class] s,
 *   class = obj_class[face_obj[f]] (both clamped into their tables).  A channel is floor(255 c + 0.5), cut to 0..255. */
#ifndef RFD_RENDER_H
#define RFD_RENDER_H
#ifdef __cplusplus
extern "C" {
#endif

/* Projects the V vertices and then the N scan points (rows V .. V+N-1 of the outputs) in one launch.
 *   vertices (V,3) f32, points: N rows of `point_stride` floats, xyz first; camera: 16 doubles on the host;
 *   q (V+N) f64, sxy (V+N,2) i32, valid (V+N) u8.  Invalid rows get q = 0, sxy = 0. */
int rfd_raster_project(int V, int N, int point_stride, const float *vertices, const float *points, const double *camera,
                       double near, double *q, int *sxy, unsigned char *valid, void *stream);

/* Clears keys (H,W) u64 and draws the F triangles and the N points (rules 3 and 4) in one launch.
 *   faces (F,3) i32 into the first V rows of q / sxy / valid. */
int rfd_raster_triangles(int V, int F, int N, int W, int H, int point_px, const int *faces, const double *q,
                         const int *sxy, const unsigned char *valid, unsigned long long *keys, void *stream);

/* keys -> ids (H,W) i32, depth (H,W) f32, image (H,W,3) u8 (rule 5).
 *   face_obj (F) i32, obj_class (K) i32, palette (C,3) f32, eye: 3 doubles on the host (rounded to f32).  Only faces
 *   that rfd_raster_triangles drew are read, so their vertex indices are in range. */
int rfd_raster_shade(int F, int K, int C, int W, int H, const float *vertices, const int *faces, const int *face_obj,
                     const int *obj_class, const float *palette, const double *eye, const unsigned long long *keys,
                     int *ids, float *depth, unsigned char *image, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_RENDER_H */
