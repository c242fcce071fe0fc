"""Generator3D.refine_mesh (generator.py:226-289) restated in closed form, float64, plain torch on the CPU: the ground truth
of the refinement tests.

The decoder is piecewise linear in the query point, so the reference's double backward needs the logit l, its input gradient
g (one first-order autograd pass) and the derivatives of the sigmoid only -- the formulas csrc/mesh_refine.hip evaluates in
fp32.  tests/golden/make_refine_fixture.py checks this restatement against full double-backward autograd."""
import numpy as np
import torch

from normals_f64 import decoder_torch

EPS = 1e-10
LR, ALPHA, RMS_EPS = 1e-4, 0.99, 1e-8       # torch.optim.RMSprop([v], lr=1e-4) defaults


def value_and_grad(sd, q, z, c):
    """q (F,3) f64 tensor -> logit (F,), d logit / d q (F,3)"""
    qq = q.detach().clone().requires_grad_()
    with torch.enable_grad():
        l = decoder_torch(sd, qq[None], z[None], c[None])[0]
        g, = torch.autograd.grad(l.sum(), qq)
    return l.detach(), g


def face_terms(v, faces, e, l, g, tau):
    """-> loss, corner gradients (F,3,3) of  mean (s - tau)^2 + 0.01 mean |nf - nt|^2"""
    F = faces.shape[0]
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    a, b = v1 - v0, v2 - v1
    cr = torch.cross(a, b, dim=1)
    r = cr.norm(dim=1, keepdim=True)
    nf = cr / (r + EPS)
    s = torch.sigmoid(l)[:, None]
    s1 = s * (1 - s)
    s2 = s1 * (1 - 2 * s)
    m = s1 * g.norm(dim=1, keepdim=True) + EPS
    nt = -s1 * g / m
    d = nf - nt
    loss = ((s - tau) ** 2).mean() + 0.01 * (d ** 2).sum(1).mean()
    gq = (2 * (s - tau) * s1 / F + (0.02 / F) * (d * g).sum(1, keepdim=True) * s2 * EPS / m ** 2) * g
    u = (0.02 / F) * d
    uc = (u * cr).sum(1, keepdim=True)
    w = torch.where(r > 0, u / (r + EPS) - cr * uc / (r * (r + EPS) ** 2).clamp_min(1e-300), u / EPS)
    da, db = torch.cross(b, w, dim=1), torch.cross(w, a, dim=1)
    G = torch.stack([e[:, 0:1] * gq - da, e[:, 1:2] * gq + da - db, e[:, 2:3] * gq + db], dim=1)
    return loss, G


def vertex_grad(v, faces, e, sd, z, c, tau):
    """one evaluation at vertices v with weights e -> loss (float), d loss / d v (V,3)"""
    q = (e[:, 0:1] * v[faces[:, 0]] + e[:, 1:2] * v[faces[:, 1]]) + e[:, 2:3] * v[faces[:, 2]]
    l, g = value_and_grad(sd, q, z, c)
    loss, G = face_terms(v, faces, e, l, g, tau)
    out = torch.zeros_like(v)
    out.index_add_(0, faces.reshape(-1), G.reshape(-1, 3))
    return float(loss), out


def _t(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype)).double()


def refine_f64(sd, v0, faces, z, c, eps, tau, return_grad=False, snapshots=None):
    """v0 (V,3) (rounded to f32 like torch.FloatTensor), faces (F,3), one code z (Z,), c (C,), eps (steps,F,3) (rounded to
    f32: the reference uploads its draw as a FloatTensor) -> refined vertices (V,3) f64 numpy [, the first step's gradient].
    snapshots (a dict): receives {n: the vertices after n steps} for the step counts it has as keys"""
    v = _t(v0)
    faces = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    z, c, eps = _t(z), _t(c), _t(eps)
    sq = torch.zeros_like(v)
    first = np.zeros(tuple(v.shape))
    for it, e in enumerate(eps):
        if faces.shape[0] == 0:
            break
        _, G = vertex_grad(v, faces, e, sd, z, c, tau)
        if it == 0:
            first = G.numpy().copy()
        sq = ALPHA * sq + (1 - ALPHA) * G * G
        v = v - LR * G / (sq.sqrt() + RMS_EPS)
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = v.numpy().copy()
    return (v.numpy(), first) if return_grad else v.numpy()


def loss_f64(sd, v, faces, z, c, tau, e=None):
    """the loss at weights e (default: the barycentre) on vertices v, float64"""
    faces = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    if e is None:
        e = np.full((faces.shape[0], 3), np.float32(1.0 / 3))       # as an uploaded FloatTensor
    return vertex_grad(torch.as_tensor(np.asarray(v, dtype=np.float64)), faces, torch.as_tensor(np.asarray(e, np.float64)),
                       sd, _t(z), _t(c), tau)[0]
