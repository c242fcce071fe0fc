/* rfd_fit.h -- fit_mesh_to_scan's optimisation on the device (models/iscnet/modules/network.py:182-303): Adam steps on
 * a one-sided Chamfer loss over the centre and heading of every box, with the nearest-neighbour search restricted to
 * the points that can matter and the gradient in closed form.
 *
 * The problem is ragged (CSR): object p owns rows obj_off[p] .. obj_off[p+1] of `obj` (its mesh points, normalised and
 * scaled by the box sizes; where the mesh has fewer rows than the reference's padding, ONE extra zero row at the end
 * stands for all padded rows: they are identical, land on the box centre, and the lowest index wins a tie) and rows
 * scan_off[p] .. scan_off[p+1] of `scan` (the scan points inside its enlarged box, in scan order).  Tile k is at most
 * 256 * points_per_thread scan rows of object tile_obj[k] starting at row tile_start[k] of `scan`; the tiles of an
 * object partition its rows.  params (P,4) = cx, cy, cz, theta.
 *
 * Arithmetic contract.  o' = (ox cos + oy (-sin) + cx, ox sin + oy cos + cy, oz + cz) and d = dx dx + dy dy + dz dz with
 * dx = o'x - sx: fp32, summed left to right, no fma, strict '<' in index order (rfd_chamfer_forward's search); cos and
 * sin are the f64 functions of theta rounded to fp32, evaluated once per workgroup: the correctly rounded fp32 values
 * (a host restatement gets the same bits from any libm, which it would not from an fp32 sine of its own).  With
 * r = o'_nn - s and q = o'_nn - c (fp32 differences) a scan point adds d to the loss, 2 r to d/dc and
 * 2 (r_x (-q_y) + r_y q_x) to d/dtheta: formed and summed in f64 in a fixed order, scaled by loss_scale, the gradient
 * rounded to fp32.  The loss is the f64 sum over objects in order, rounded once.  The update is torch.optim.Adam's
 * (betas 0.9 / 0.999, eps 1e-8) in fp32: m = fma(w1, g - m, m); v = fma(w2 g, g, v b2); p += (-step m) / (sqrt(v) / c2 +
 * eps), the step-dependent scalars computed in double on the host.  No atomics: two calls are bitwise equal. */
#ifndef RFD_FIT_H
#define RFD_FIT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of rfd_fit_pose_run's workspace: five f64 partial sums per tile, one f64 loss per object, Adam's two moments */
size_t rfd_fit_pose_workspace_bytes(int P, int n_tiles);

/* Enqueues `iterations` iterations on `stream`, two launches each and nothing else.
 *   obj (n_obj,3) f32, obj_off (P+1) i32, scan (n_scan,3) f32, scan_off (P+1) i32, tile_obj / tile_start (n_tiles) i32,
 *   points_per_thread 1 or 4 (the tiling's), loss_scale: the factor on the summed squared distances,
 *   params (P,4) f32 in / out, best_params (P,4) f32, best_loss (1) f32, best_iter (1) i32: the parameters, loss and
 *   index of the first iteration with the lowest loss (strictly below 1e6) BEFORE its update,
 *   hist_loss (iterations) f32, hist_params (iterations,P,4) f32: loss and parameters before every update, or NULL,
 *   workspace: rfd_fit_pose_workspace_bytes(P, n_tiles) bytes, 8-byte aligned.
 * Offsets and tile entries outside their arrays are clamped into them.  P <= 0 or n_tiles <= 0: nothing is launched. */
int rfd_fit_pose_run(int P, int n_obj, int n_scan, int n_tiles, int points_per_thread, int iterations, double lr,
                     double loss_scale, const float *obj, const int *obj_off, const float *scan, const int *scan_off,
                     const int *tile_obj, const int *tile_start, float *params, float *best_params, float *best_loss,
                     int *best_iter, float *hist_loss, float *hist_params, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFD_FIT_H */
