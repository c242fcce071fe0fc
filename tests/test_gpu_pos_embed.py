"""GPU (-m gpu): fc_pos of the skip-propagation encoder (csrc/pos_embed.hip) away from the network's own shape.

tests/test_gpu_gemm.py runs pos_embed_kernel at M = 1152, N = 1024, d = 4 and pos_embed_frag_kernel at M = 6144,
N = 1024: one full column pass, whole row blocks, whole workgroups, no grid-stride repeat.  Here: a ragged last row
block, fewer columns than one pass (idle threads) and more (a second pass with the weights reloaded), d = 0, 1, 3, 8,
row strides on x and W, a group count that does not divide M, masks that are not 0 / 1 -- against float64 under a
bound derived from the kernel's operations -- and the frag kernel at one row block, at a last workgroup that does not
fill its four waves, and past the workgroup cap, where every wave repeats its grid-stride loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F_BOX = 8           # box-feature columns of W behind the d point columns: W's row stride is d + 8 > d
U = 2.0 ** -24      # unit roundoff of fp32


def _inputs(M, rpg, N, d, seed, soft_mask=False):
    """x (M, d) and W[:, :d] as column windows of wider matrices (row strides d + 5 and d + 8), mask, bias and the
    per-group term.  `group` is an INPUT of the kernel (the caller's box_feature . W[:, d:]^T, fp32)."""
    rng = np.random.default_rng(seed)
    G = -(-M // rpg)
    xw = torch.from_numpy(rng.standard_normal((M, d + 5)).astype(np.float32)).cuda()
    x = xw[:, 2:2 + d]
    W = torch.from_numpy((rng.standard_normal((N, d + F_BOX)) * 0.3).astype(np.float32)).cuda()
    if soft_mask:                                   # the kernel MULTIPLIES by the mask: any value, either sign, zeros
        mask = rng.uniform(-1.5, 1.5, M).astype(np.float32)
        mask[rng.random(M) < 0.2] = 0.0
    else:
        mask = (rng.random(M) > 0.4).astype(np.float32)
    mask = torch.from_numpy(mask).cuda()
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    box = torch.from_numpy(rng.standard_normal((G, F_BOX)).astype(np.float32)).cuda()
    group = torch.nn.functional.linear(box, W[:, d:]).contiguous()
    assert x.shape == (M, d) and x.stride(0) == d + 5 > d and W.stride(0) == d + F_BOX > d and group.shape == (G, N)
    return x, mask, W, bias, box, group


def _window(M, N):
    """(M, N) output window at column 4 of a (M, N + 8) buffer of sevens"""
    buf = torch.full((M, N + 8), 7.0, device="cuda")
    return buf, buf[:, 4:4 + N]


# (M, rows_per_group, N, d, mask not 0 / 1)
PLAIN_CASES = [(1, 1, 4, 1, False), (65, 65, 36, 3, True), (200, 50, 1028, 8, False), (130, 64, 2048, 0, False),
               (1152, 192, 1024, 4, False)]


@pytest.mark.parametrize("M,rpg,N,d,soft", PLAIN_CASES, ids=["%dx%d-g%d-d%d" % (c[0], c[2], c[1], c[3]) for c in PLAIN_CASES])
def test_pos_embed_ragged_shapes_against_float64(hip, M, rpg, N, d, soft):
    """out = linear(cat([x, box]) * mask) with group = box . W[:, d:]^T handed in, per element within
        (d + 3) 2^-24 (|m| (sum_j |x_j W_nj| + |g_n|) + |b_n|):
    the kernel does d fmas, one add and one fma on fp32 inputs, each within 2^-24 of its exact result; the bound is
    that many roundings (and one to spare) of the sum of the magnitudes."""
    from rfdnet_amd import pos_embed
    x, mask, W, bias, box, group = _inputs(M, rpg, N, d, seed=M + N + d, soft_mask=soft)
    if M == 130:
        assert group.shape[0] == 3                  # 64 + 64 + 2 rows
    buf, out = _window(M, N)
    pos_embed.pos_embed(x, mask, W, bias, group, rpg, out)
    hip.device_status()
    rows = torch.arange(M, device="cuda") // rpg
    xd, Wd, g, m, b = x.double(), W[:, :d].double(), group.double()[rows], mask.double()[:, None], bias.double()
    want = b + m * (xd @ Wd.t() + g)
    bound = (d + 3) * U * (m.abs() * (xd.abs() @ Wd.abs().t() + g.abs()) + b.abs())
    err = (out.double() - want).abs()
    print("pos_embed %s: max err %.3e, max err / bound %.3f" % ((M, rpg, N, d), err.max().item(),
                                                                (err / bound).max().item()))
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.all(buf[:, :4] == 7.0) and torch.all(buf[:, 4 + N:] == 7.0)
    # the same numbers as the composition the kernel replaces, with the box feature in the matrix
    full = torch.cat([x, box[rows]], 1).double() * m
    comp = torch.nn.functional.linear(full, W.double(), b)
    assert (out.double() - comp).abs().max().item() < 1e-5 * max(1.0, comp.abs().max().item())


def test_pos_embed_range_flag_at_a_ragged_shape(hip):
    """RFD_STATUS_GEMM_RANGE is raised when a stored value x 2^sa reaches 65504, the largest f16 -- and is clear
    just below it -- also in the last, single-row block (M = 65) and the last columns of a short pass (N = 36)"""
    from rfdnet_amd import gemm, pos_embed
    M, rpg, N, d = 65, 65, 36, 3
    x = torch.zeros(M, d, device="cuda")
    W = torch.zeros(N, d, device="cuda")
    bias = torch.zeros(N, device="cuda")
    edge = np.float32(65504.0 / 2 ** gemm.SA)
    below = np.nextafter(edge, np.float32(0))
    for row, col, sign in ((64, 35, 1.0), (64, 0, -1.0), (0, 33, 1.0)):
        mask = torch.zeros(M, device="cuda")
        mask[row] = sign                            # out[row][col] = fma(+-1, 0 + group, 0) = +-group exactly, 0 elsewhere
        group = torch.zeros(1, N, device="cuda")
        buf, out = _window(M, N)
        group[0, col] = float(below)
        pos_embed.pos_embed(x, mask, W, bias, group, rpg, out)
        hip.device_status()                          # clear
        assert float(out[row, col]) == sign * float(below) and int((out != 0).sum()) == 1
        group[0, col] = float(edge)
        pos_embed.pos_embed(x, mask, W, bias, group, rpg, out)
        with pytest.raises(hip.RfdHipError, match="split-precision GEMM") as e:
            hip.device_status()
        assert e.value.status & 4
        assert float(out[row, col]) == sign * float(edge)   # the stored value is right: the flag is about the consumer
    hip.device_status()


def _frag_case(hip, M, N, d, rpg, seed):
    from rfdnet_amd import gemm, pos_embed
    x, mask, W, bias, _, group = _inputs(M, rpg, N, d, seed=seed)
    plain = torch.empty(M, N, device="cuda")
    pos_embed.pos_embed(x, mask, W, bias, group, rpg, plain)
    cat = gemm.frag_empty(M, N + 32, "cuda")
    cat.view(torch.int16).fill_(0x7c00)                              # f16 inf
    pos_embed.pos_embed_frag(x, mask, W, bias, group, rpg, cat[:, 1:], gemm.SA)
    hip.device_status()
    want = gemm.rows_to_frag(plain, sa=gemm.SA)
    hip.device_status()
    assert (want != 0).any()
    assert torch.equal(cat[:, 1:], want)                             # bit for bit
    assert (cat[:, 0].view(torch.int16) == 0x7c00).all()            # the neighbouring channel block is untouched


@pytest.mark.parametrize("M,N,d,rpg", [(32, 32, 1, 32), (160, 96, 3, 32)], ids=["one-block", "ragged-workgroup"])
def test_pos_embed_frag_small_and_ragged_matches_pos_embed(hip, M, N, d, rpg):
    """one row block and one channel block (three idle waves); five row blocks, i.e. a second workgroup with one live
    wave: the frag rows hold exactly split(relu(fp32 fc_pos) 2^sa)"""
    _frag_case(hip, M, N, d, rpg, seed=M + d)


def test_pos_embed_frag_past_the_workgroup_cap(hip):
    """64 CUs + 3 row blocks = 16 CUs + 1 workgroups of four waves against a cap of 8 CUs: every wave goes through
    its grid-stride loop at least twice and the last pass is ragged (about 70 MB per buffer on 256 CUs)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _frag_case(hip, 32 * (64 * cus + 3), 32, 8, 32, seed=5)
