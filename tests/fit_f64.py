"""The ragged restatement of fit_mesh_to_scan's optimisation (include/rfd_fit.h, csrc/fit_pose.hip) in numpy: float64
throughout, or -- fp32=True, the same code -- with the kernel's number formats: fp32 parameters, transform, distances and
Adam, f64 sums.  No padding: the problem is the CSR layout of rfd_fit.h, the one extra zero row per short mesh included.

The search is brute force over (scan point, mesh row) pairs with numpy's argmin, which returns the FIRST minimum: the
lowest index wins a tie, as in the kernel.  F_FIT's problem takes about a minute for 100 iterations, which is why its
histories are a fixture (tests/golden/make_fit_device_fixture.py)."""
import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
F = np.float32


def fma32(a, b, c):
    """the correctly rounded fp32 a * b + c of fp32 arrays: the product is exact in f64, the sum is rounded to odd in
    f64 (TwoSum's error term says on which side of it the exact value lies), so the final rounding to fp32 is the only
    one that counts"""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even & np.isfinite(s), np.nextafter(s, toward), s)
    return s.astype(F)


def adam_step(p, m, v, g, t, lr, fp32):
    """one step (t = 1, 2, ...) of torch.optim.Adam's defaults on arrays (none is modified): -> p, m, v.
    fp32: the operations of torch's single-tensor Adam on CPU fp32 tensors, bit for bit -- exp_avg.lerp_ is
    fma(w, g - m, m), exp_avg_sq.mul_(beta2).addcmul_(g, g, value) is fma(value * g, g, v * beta2), addcdiv_ is
    p + (value * m) / denom; the Python floats (1 - beta ** t, lr / (.), (.) ** 0.5) are rounded to fp32 where they meet
    a tensor."""
    bc1, bc2 = 1 - BETA1 ** t, 1 - BETA2 ** t
    step_size, bc2_sqrt = lr / bc1, bc2 ** 0.5
    if not fp32:
        m = m + (1 - BETA1) * (g - m)
        v = v * BETA2 + ((1 - BETA2) * g) * g
        return p + (-step_size * m) / (np.sqrt(v) / bc2_sqrt + EPS), m, v
    assert p.dtype == m.dtype == v.dtype == g.dtype == F
    m = fma32(F(1 - BETA1), g - m, m)
    v = fma32(F(1 - BETA2) * g, g, v * F(BETA2))
    den = np.sqrt(v) / F(bc2_sqrt) + F(EPS)
    return p + (F(-step_size) * m) / den, m, v


def posed(o, par, dt):
    """rows o (V,3) under cx, cy, cz, theta: products summed left to right; cos and sin are the correctly rounded ones"""
    c, s = dt(np.cos(np.float64(par[3]))), dt(np.sin(np.float64(par[3])))
    x = o[:, 0] * c + o[:, 1] * (-s) + par[0]
    y = o[:, 0] * s + o[:, 1] * c + par[1]
    z = o[:, 2] + par[2]
    return np.stack([x, y, z], 1).astype(dt)


def object_terms(o, sc, par, dt):
    """one object: -> (sum of squared nearest distances, the four gradient sums, nearest indices), sums in f64"""
    o2 = posed(o, par, dt)
    chunk = max(1, 1000000 // o.shape[0])
    nn = np.empty(sc.shape[0], np.int64)
    dist = np.empty(sc.shape[0], dt)
    for a in range(0, sc.shape[0], chunk):
        d = o2[None, :, :] - sc[a:a + chunk, None, :]
        d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        nn[a:a + chunk] = d.argmin(1)
        dist[a:a + chunk] = d[np.arange(d.shape[0]), nn[a:a + chunk]]
    r = (o2[nn] - sc).astype(np.float64)                       # fp32 differences, then f64
    q = (o2[nn] - par[None, :3]).astype(np.float64)
    sums = np.array([dist.astype(np.float64).sum(), (2.0 * r[:, 0]).sum(), (2.0 * r[:, 1]).sum(), (2.0 * r[:, 2]).sum(),
                     (2.0 * (r[:, 0] * -q[:, 1] + r[:, 1] * q[:, 0])).sum()])
    return sums, nn


def terms(obj, obj_off, scan, scan_off, params, fp32=False):
    """-> (P,5) f64: per object the summed squared distances and d/d(cx, cy, cz, theta) of them, unscaled"""
    dt = F if fp32 else np.float64
    out = np.zeros((len(obj_off) - 1, 5))
    for p in range(len(obj_off) - 1):
        out[p] = object_terms(np.asarray(obj[obj_off[p]:obj_off[p + 1]], dt), np.asarray(scan[scan_off[p]:scan_off[p + 1]], dt),
                              np.asarray(params[p], dt), dt)[0]
    return out


def fit(obj, obj_off, scan, scan_off, params0, loss_scale, lr=0.01, iterations=100, fp32=False):
    """the loop of rfd_fit_pose_run -> {'hist_loss' (T), 'hist_params' (T,P,4): the state before every update,
    'best_iter', 'best_loss', 'best_params'}: the first iteration with the lowest loss (strictly below 1e6)"""
    dt = F if fp32 else np.float64
    par = np.array(params0, dt)
    m, v = np.zeros_like(par), np.zeros_like(par)
    hist_loss, hist_params = np.zeros(iterations, dt), np.zeros((iterations,) + par.shape, dt)
    best_loss, best_iter, best_params = dt(1e6), -1, par.copy()
    for it in range(iterations):
        sums = terms(obj, obj_off, scan, scan_off, par, fp32)
        total = 0.0
        for p in range(sums.shape[0]):                           # objects in ascending order
            total += sums[p, 0]
        loss = dt(total * loss_scale)
        grad = (sums[:, 1:] * loss_scale).astype(dt)
        hist_loss[it], hist_params[it] = loss, par
        if loss < best_loss:
            best_loss, best_iter, best_params = loss, it, par.copy()
        par, m, v = adam_step(par, m, v, grad, it + 1, lr, fp32)
    return {'hist_loss': hist_loss, 'hist_params': hist_params, 'best_iter': best_iter, 'best_loss': best_loss,
            'best_params': best_params}


def box_corners(sizes, best_params):
    """the corners fit.finish_fit builds from the best parameters: (P,8,3) float64, upright camera frame"""
    import torch
    from rfdnet_amd.iscnet import fit as F_
    best = torch.as_tensor(np.asarray(best_params, np.float64))
    return F_.get_3d_box(torch.as_tensor(np.asarray(sizes, np.float64)), -best[:, 3],
                         F_.flip_axis_to_camera(best[:, :3])).numpy()
