"""Inputs of the chain / head tests (tests/test_chain_cases_cpu.py proves them admissible from chain_f64 alone,
tests/test_gpu_chain.py runs them on the kernels).  Everything is seeded on the host with numpy, so both tiers see the
same numbers; the float64 reference of a case is computed once and shared (the builders are cached: treat what they
return as read-only).

Exposure batches.  chain_kernel's only output is the max over a proposal's P rows, which hides every row but the
winner.  A batch of B = P proposals makes every row position the only possible winner once: proposal b holds one fixed
background row everywhere except at row b, which is a hot row.  The reference needs the P + 1 distinct rows only."""
import functools
import types

import numpy as np
import torch

import chain_f64

# (mode, d, P, c3, relu3): P = 512 is one pass, 1024 / 1536 take the weight ring across a pass boundary; c3 = 64 is one
# piece per pass, 320 five (a count the ring's three slots do not divide); B = P >= 512 proposals > 256 CUs
EXPOSURE = [(0, 64, 512, 1024, False), (0, 64, 1024, 1024, True), (1, 3, 512, 256, True), (1, 7, 1024, 1024, True),
            (2, 64, 512, 64, True), (2, 64, 1024, 1024, True), (0, 64, 1536, 320, False)]
VARIANTS = ("same", "distinct")          # 1a: the same hot row in every proposal; 1b: a different one per proposal
EXACT_CONFIG = EXPOSURE[0]
B3_SHIFT = -1.0                          # relu3 off: pooled values of either sign
N_WAVES = 8
# seed of the one hot row of a "same" batch where the default leaves a sign combination in fewer than 4 channels
# (hot < 0 < background is rare once b3 is shifted down; tests/test_chain_cases_cpu.py holds the chosen seed to it)
SAME_SALT = {(0, 64, 1536, 320, False): 7}


def config_id(cfg):
    return "mode%d-d%d-P%d-c%d-relu%d" % (cfg[0], cfg[1], cfg[2], cfg[3], cfg[4])


def lin(rng, n, k):
    """(W, b) like tests/test_gpu_chain.py::layers: uniform +-2 / sqrt(k), bias 0.3 N(0, 1)"""
    return (((rng.random((n, k)) * 2 - 1) * 2. / np.sqrt(k)).astype(np.float32),
            (rng.standard_normal(n) * 0.3).astype(np.float32))


def chain_layers(rng, mode, d, c3):
    return (lin(rng, 64, d) if mode else None), lin(rng, 128, 64), lin(rng, c3, 128)


def to_device(layers, device="cuda"):
    return tuple(None if l is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in l)
                 for l in layers)


def _seed(cfg, salt=0):
    mode, d, P, c3, relu3 = cfg
    return 100003 * mode + 1009 * d + 31 * P + 7 * c3 + relu3 + 1000003 * salt


def _exposure_from(cfg, variant, layers, bg, hot):
    mode, d, P, c3, relu3 = cfg
    l1, l2, l3 = layers
    rows = chain_f64.chain_rows(np.concatenate([bg[None], hot]), l1, l2, l3, relu3)
    bg_out, hot_out = rows[0], rows[1:]
    ref = np.maximum(bg_out[None], hot_out)                       # (P, c3): proposal b = max(background, hot row b)
    return types.SimpleNamespace(cfg=cfg, variant=variant, mode=mode, d=d, P=P, c3=c3, relu3=relu3, layers=layers,
                                 bg=bg, hot=hot, bg_out=bg_out, hot_out=hot_out, ref=ref,
                                 tol=chain_f64.tolerance(ref), dec=chain_f64.decisive(ref))


@functools.lru_cache(maxsize=None)
def exposure(cfg, variant):
    """-> namespace: layers (numpy fp32), bg (d,), hot (P, d) fp32 rows (row b = the hot row of proposal b), and the
    float64 reference: bg_out (c3,), hot_out (P, c3), ref (P, c3), tol, dec"""
    mode, d, P, c3, relu3 = cfg
    rng = np.random.default_rng(_seed(cfg))
    l1, l2, l3 = chain_layers(rng, mode, d, c3)
    if not relu3:
        l3 = (l3[0], l3[1] + np.float32(B3_SHIFT))
    bg = (rng.standard_normal(d) * 0.5).astype(np.float32)
    hot = (rng.standard_normal((P, d)) * 1.5).astype(np.float32)
    if variant == "same":
        salt = SAME_SALT.get(cfg, 1)
        one = (np.random.default_rng(_seed(cfg, salt)).standard_normal(d) * 1.5).astype(np.float32)
        hot = np.ascontiguousarray(np.broadcast_to(one, (P, d)))
    else:
        assert variant == "distinct"
    return _exposure_from(cfg, variant, (l1, l2, l3), bg, hot)


def exposure_x(case, device="cuda"):
    """x (P * P, d): a view of the background row, materialised, with hot row b written to row b of proposal b"""
    P = case.P
    x = torch.from_numpy(case.bg).to(device).expand(P * P, case.d).contiguous()
    at = torch.arange(P, device=device)
    x.view(P, P, case.d)[at, at] = torch.from_numpy(case.hot).to(device)
    return x


def decided(case):
    """-> (hot_wins, bg_wins): (P, c3) masks of the channels a proposal's hot row / the background decides"""
    gap = case.hot_out - case.bg_out[None]
    return gap >= case.dec, -gap >= case.dec


def sign_combinations(case, pre_bias=False):
    """relu3 off -> three (P, c3) masks over (proposal, channel): background < 0 < hot decisively; hot < 0 <
    background decisively; both negative with the hot row decisively the larger.  pre_bias: of the values the LDS
    atomic maximum sees, i.e. before b3 is added (the kernel adds the bias after the pool)."""
    assert not case.relu3
    off = chain_f64.f64(case.layers[2][1]) if pre_bias else 0.
    bg, hot = (case.bg_out - off)[None], case.hot_out - off
    return ((bg < 0) & (hot > 0) & (hot - bg >= case.dec), (hot < 0) & (bg > 0) & (bg - hot >= case.dec),
            (bg < 0) & (hot < 0) & (hot - bg >= case.dec))


# ---- exact channels: zero rows of W3 whose output is b3 itself, and one channel that no row lifts above zero
EXACT_ZERO = ((0, 0.), (21, 1.25), (463, -1.25), (522, -1.25), (960, 0.), (1023, 1.25))     # (channel, b3)
EXACT_NEGATIVE = (333, -8.)             # far enough below every row's W3 . h, without widening max |ref| much


@functools.lru_cache(maxsize=None)
def exact(relu3):
    """the mode 0, P = 512 exposure batch (distinct hot rows) with the channels above rewritten"""
    base = exposure(EXACT_CONFIG, "distinct")
    W3, b3 = base.layers[2][0].copy(), base.layers[2][1].copy()
    if relu3:
        b3 -= np.float32(B3_SHIFT)         # as drawn: under the ReLU a lowered bias leaves the background little to decide
    for ch, b in EXACT_ZERO:
        W3[ch], b3[ch] = 0., b
    b3[EXACT_NEGATIVE[0]] = EXACT_NEGATIVE[1]
    cfg = base.cfg[:4] + (relu3,)
    return _exposure_from(cfg, "distinct", (None, base.layers[1], (W3, b3)), base.bg, base.hot)


# ---- dense random batches (invariances, row stride): arguments of dense()
INVARIANCE = (2, 64, 1536, 3, 1024, 77)
INVARIANCE_MODE1 = (1, 4, 1024, 3, 1024, 78)
STRIDE = ((0, 64, 512, 5, 256, 79), (2, 64, 512, 5, 256, 80))
LDX = (68, 128)


@functools.lru_cache(maxsize=None)
def dense(mode, d, P, B, c3, seed):
    """i.i.d. rows 1.5 N(0, 1) like the older tests -> namespace: layers, x (B * P, d), perm (B, P) row permutations"""
    rng = np.random.default_rng(seed)
    layers = chain_layers(rng, mode, d, c3)
    x = (rng.standard_normal((B * P, d)) * 1.5).astype(np.float32)
    perm = np.stack([rng.permutation(P) for _ in range(B)])
    return types.SimpleNamespace(mode=mode, d=d, P=P, B=B, c3=c3, layers=layers, x=x, perm=perm,
                                 prop_perm=np.roll(np.arange(B), 1))


def permute_rows(x, P, perm):
    """rows of every proposal in the order perm[b] (numpy (B, P)); x a (B * P, d) tensor"""
    B = x.shape[0] // P
    index = torch.from_numpy(perm + P * np.arange(B)[:, None]).reshape(-1).to(x.device)
    return x[index]


def strided(x, ldx, shift=4, fill=7.5):
    """x (M, d) as a column slice of a wider buffer: rows ldx floats apart, the base `shift` floats behind an allocation's
    start; what lies between the rows is `fill`, not zero"""
    M, d = x.shape
    flat = torch.full((shift + M * ldx + 16,), fill, dtype=x.dtype, device=x.device)
    view = flat[shift:shift + M * ldx].view(M, ldx)[:, :d]
    view.copy_(x)
    return view


# ---- the head
HEAD_P = (128, 384)
HEAD_B = 300


@functools.lru_cache(maxsize=None)
def head(P, n_cls=2):
    """-> namespace: Wa, lb, lc, (Wd, bd), gbias (B, 512), one x row, x (B * P, 64) distinct rows, perm (B, P)"""
    rng = np.random.default_rng(4000 + P)                 # the hidden layers do not depend on n_cls
    (Wa, _), lb, lc, (Wd, bd) = lin(rng, 512, 64), lin(rng, 256, 512), lin(rng, 128, 256), lin(rng, 2, 128)
    gbias = rng.standard_normal((HEAD_B, 512)).astype(np.float32)
    row = (rng.standard_normal(64) * 1.5).astype(np.float32)
    x = (rng.standard_normal((HEAD_B * P, 64)) * 1.5).astype(np.float32)
    perm = np.stack([rng.permutation(P) for _ in range(HEAD_B)])
    return types.SimpleNamespace(P=P, B=HEAD_B, n_cls=n_cls, Wa=Wa, lb=lb, lc=lc, Wd=Wd[:n_cls].copy(),
                                 bd=bd[:n_cls].copy(), gbias=gbias, row=row, x=x, perm=perm)


@functools.lru_cache(maxsize=None)
def head_one_row_ref(P, shared_gbias):
    """float64 scores (B, 2) of the one x row under gbias[0] everywhere (shared_gbias) or under each proposal's own"""
    c = head(P)
    gb = np.broadcast_to(c.gbias[0], c.gbias.shape) if shared_gbias else c.gbias
    return chain_f64.head_scores(np.broadcast_to(c.row, (c.B, 64)), 1, c.Wa, gb, c.lb, c.lc, c.Wd, c.bd)


@functools.lru_cache(maxsize=None)
def head_hidden_ref(P):
    """float64 (B * P, 128) last hidden layer of the distinct rows: shared by the n_cls = 1 and 2 cases"""
    c = head(P)
    return chain_f64.head_hidden(c.x, P, c.Wa, c.gbias, c.lb, c.lc)
