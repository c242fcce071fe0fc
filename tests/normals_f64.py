"""Input gradient of DecoderCBatchNorm (occ_decoder.py:110-123, layers.py:98-107, 226-242) by torch autograd of a
restatement, in float64 (the ground truth of the normals tests) or float32 (the same operations the reference's modules
run: its own fp32 autograd, Generator3D.estimate_normals, generator.py:200-224).  CPU only."""
import numpy as np
import torch


def decoder_torch(sd, p, z, c, eps=1e-5, record=None):
    """sd: state_dict (numpy arrays, reference key names); p (K,T,3), z (K,Z), c (K,C) tensors of one dtype -> (K,T).
    record (a list): receives the 11 ReLU inputs (K,T,256)"""
    def relu(x):
        if record is not None:
            record.append(x.detach())
        return torch.relu(x)

    dt = p.dtype
    g = lambda k: torch.as_tensor(np.asarray(sd[k])).to(dt)

    def cbn(prefix, x):
        gamma = c @ g(prefix + ".conv_gamma.weight")[:, :, 0].T + g(prefix + ".conv_gamma.bias")
        beta = c @ g(prefix + ".conv_beta.weight")[:, :, 0].T + g(prefix + ".conv_beta.bias")
        nrm = (x - g(prefix + ".bn.running_mean")) / torch.sqrt(g(prefix + ".bn.running_var") + eps)
        return gamma[:, None, :] * nrm + beta[:, None, :]

    net = p @ g("fc_p.weight")[:, :, 0].T + g("fc_p.bias")
    if z.shape[1] > 0:
        net = net + (z @ g("fc_z.weight").T + g("fc_z.bias"))[:, None, :]
    for i in range(5):
        b = "blocks.%d." % i
        a0 = relu(cbn(b + "bn_0", net))
        h = a0 @ g(b + "fc_0.weight")[:, :, 0].T + g(b + "fc_0.bias")
        a1 = relu(cbn(b + "bn_1", h))
        net = net + a1 @ g(b + "fc_1.weight")[:, :, 0].T + g(b + "fc_1.bias")
    a = relu(cbn("bn", net))
    return a @ g("fc_out.weight")[0, :, 0] + g("fc_out.bias")[0]


def input_grad(sd, p, z, c, dtype=torch.float64, return_margin=False):
    """p (K,T,3) (f32 values: the fp32 vertices), z (K,Z), c (K,C) numpy -> d logit / d p (K,T,3) numpy of `dtype`
    [, margin (K,T): min over the 11 ReLUs of min_channel |input| / max_channel |input| -- how close the point sits to a
    kink of the piecewise-linear gradient, relative to the layer's scale]"""
    pt = torch.as_tensor(np.asarray(p, dtype=np.float32)).to(dtype).requires_grad_()
    zt = torch.as_tensor(np.asarray(z, dtype=np.float32)).to(dtype)
    ct = torch.as_tensor(np.asarray(c, dtype=np.float32)).to(dtype)
    rec = []
    with torch.enable_grad():
        decoder_torch(sd, pt, zt, ct, record=rec).sum().backward()
    if not return_margin:
        return pt.grad.numpy()
    margin = torch.stack([x.abs().min(-1).values / x.abs().max(-1).values.clamp_min(1e-300) for x in rec]).min(0).values
    return pt.grad.numpy(), margin.numpy()


def normals_of(grad):
    """-g / |g| (float64 arithmetic)"""
    g = np.asarray(grad, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return -g / np.linalg.norm(g, axis=-1, keepdims=True)


KINK_MARGIN = 2.0 ** -20      # a ReLU input this close to 0 (relative to its layer) may take either side in fp32 arithmetic
KINK_JUMP = 0.05              # bound on a normal there: the gradient jumps by one channel's share


def contract(kernel_n, ref32_n, f64_n, margin=None, tol=1e-4):
    """The precision contract: |kernel - f64| <= tol per component, except
      * where the reference's fp32 normals are > tol from f64 themselves: the kernel may be off by 2x the reference's error;
      * where a ReLU input of the float64 evaluation is within KINK_MARGIN of its kink (margin from input_grad): the
        gradient is discontinuous there and ANY fp32-class evaluation -- the reference's included -- may land on the other
        side (then its normal is off by one channel's share, ~1e-3 .. 1e-2): bounded by KINK_JUMP.
    -> (bad vertex mask, exception vertex mask, kernel error per vertex)"""
    ek = np.abs(np.asarray(kernel_n, np.float64) - f64_n).max(-1)
    er = np.abs(np.asarray(ref32_n, np.float64) - f64_n).max(-1)
    exc = er > tol
    bound = np.where(exc, np.maximum(2 * er, tol), tol)
    if margin is not None:
        kink = np.asarray(margin) < KINK_MARGIN
        bound = np.where(kink, np.maximum(bound, KINK_JUMP), bound)
        exc = exc | kink
    bad = ek > bound
    return bad, exc, ek
