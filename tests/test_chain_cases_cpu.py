"""CPU tier of the chain / head tests: proves from the float64 restatement alone (tests/chain_f64.py) that every case of
tests/chain_cases.py is admissible, i.e. that the property the GPU tier checks on the kernel is decided by a margin no
admissible rounding can close.  No GPU, no kernel.

"Decides" = beats the other candidate by at least 100 x the GPU tier's tolerance (chain_f64.decisive)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cases  # noqa: E402
import chain_f64  # noqa: E402

IDS = [cases.config_id(c) for c in cases.EXPOSURE]


def test_f64_restatement_is_the_composition_of_the_layers():
    """chain_f64 against torch's float64 layers on the CPU, rows before the pool and pooled, all modes, relu3 on / off;
    the head likewise"""
    rng = np.random.default_rng(5)
    lin = torch.nn.functional.linear
    for mode, d in ((0, 64), (1, 3), (1, 8), (2, 64)):
        layers = cases.chain_layers(rng, mode, d, 128)
        x = rng.standard_normal((24, d)).astype(np.float32)
        for relu3 in (False, True):
            h = torch.from_numpy(x).double()
            for i, l in enumerate(layers):
                if l is not None:
                    h = lin(h, torch.from_numpy(l[0]).double(), torch.from_numpy(l[1]).double())
                    h = torch.relu(h) if i < 2 or relu3 else h
            rows = chain_f64.chain_rows(torch.from_numpy(x), *cases.to_device(layers, "cpu"), relu3)
            np.testing.assert_allclose(rows, h.numpy(), rtol=0, atol=1e-12)
            assert relu3 or (rows < 0).any()
            np.testing.assert_array_equal(chain_f64.chain_pool(x, *layers, 8, relu3), rows.reshape(3, 8, -1).max(1))
    c = cases.head(128)
    x, P = c.x[:256], 128
    h = torch.relu(lin(torch.from_numpy(x).double(), torch.from_numpy(c.Wa).double())
                   + torch.from_numpy(c.gbias[:2]).double().repeat_interleave(P, 0))
    for W, b in (c.lb, c.lc):
        h = torch.relu(lin(h, torch.from_numpy(W).double(), torch.from_numpy(b).double()))
    want = lin(h, torch.from_numpy(c.Wd).double(), torch.from_numpy(c.bd).double()).numpy()
    got = chain_f64.head_scores(x, P, c.Wa, c.gbias[:2], c.lb, c.lc, c.Wd, c.bd)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("cfg", cases.EXPOSURE, ids=IDS)
def test_exposure_batch_is_admissible(cfg, variant):
    """every hot row decides at least max(4, c3 / 32) channels and the background at least as many against it; in the
    distinct variant consecutive proposals differ decisively in at least 4 channels"""
    case = cases.exposure(cfg, variant)
    assert case.hot.shape == (case.P, case.d) and case.ref.shape == (case.P, case.c3)
    assert (case.hot[0] == case.hot).all() == (variant == "same")
    hot_wins, bg_wins = cases.decided(case)
    need = max(4, case.c3 // 32)
    n_hot, n_bg = hot_wins.sum(1), bg_wins.sum(1)
    print("%s %s: |ref| up to %.2f, decisive gap %.2e; channels decided by the hot row: min %d of %d (%.1f %%), by the "
          "background: min %d (%.1f %%)" % (cases.config_id(cfg), variant, np.abs(case.ref).max(), case.dec,
                                            n_hot.min(), case.c3, 100. * n_hot.min() / case.c3, n_bg.min(),
                                            100. * n_bg.min() / case.c3))
    assert n_hot.min() >= need and n_bg.min() >= need
    if variant == "distinct":
        apart = (np.abs(case.ref[1:] - case.ref[:-1]) >= case.dec).sum(1)
        print("consecutive proposals differ decisively in at least %d channels" % apart.min())
        assert apart.min() >= 4
        assert len(np.unique(case.hot, axis=0)) == case.P


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("cfg", [c for c in cases.EXPOSURE if not c[4]],
                         ids=[cases.config_id(c) for c in cases.EXPOSURE if not c[4]])
def test_exposure_batch_without_relu_has_every_sign_combination(cfg, variant):
    """relu3 off: background < 0 < hot, hot < 0 < background and both negative with the hot row the larger, each in
    at least 1000 (proposal, channel) pairs and in at least 4 channels, the first for hot rows in each of the 8 waves.
    Asserted twice: of the outputs, and of the values before b3 is added -- the kernel pools BEFORE the bias
    (max commutes with it), so those are the values whose sign chooses the branch of atomic_max_float."""
    case = cases.exposure(cfg, variant)
    for pre_bias in (False, True):
        masks = cases.sign_combinations(case, pre_bias)
        counts = [int(m.sum()) for m in masks]
        channels = [int(m.any(0).sum()) for m in masks]
        print("%s %s %s: bg < 0 < hot %d, hot < 0 < bg %d, bg < hot < 0 %d pairs (%s channels)"
              % (cases.config_id(cfg), variant, "before the bias" if pre_bias else "outputs", *counts, channels))
        assert min(counts) >= 1000 and min(channels) >= 4
        per_wave = masks[0].any(1).reshape(cases.N_WAVES, -1).any(1)       # hot row b sits in wave b // (P / 8)
        assert per_wave.all()
    assert (case.ref < 0).any() and (case.ref > 0).any()


@pytest.mark.parametrize("cfg", [cases.EXPOSURE[2], cases.EXPOSURE[0]], ids=[IDS[2], IDS[0]])
def test_exposure_builder_places_the_hot_rows(cfg):
    """exposure_x on the CPU: proposal b is the background row everywhere but at row b"""
    case = cases.exposure(cfg, "distinct")
    x = cases.exposure_x(case, "cpu").numpy().reshape(case.P, case.P, case.d)
    assert x.flags["C_CONTIGUOUS"]
    at = np.arange(case.P)
    np.testing.assert_array_equal(x[at, at], case.hot)
    off = np.ones((case.P, case.P), bool)
    off[at, at] = False
    assert (x[off] == case.bg).all()
    if case.d <= 8:                      # small enough to pool the whole batch in float64: it is the (P + 1)-row reference
        full = chain_f64.chain_pool(x.reshape(-1, case.d), *case.layers, case.P, case.relu3)
        np.testing.assert_array_equal(full, case.ref)


@pytest.mark.parametrize("relu3", [False, True])
def test_exact_channels(relu3):
    """zero rows of W3: the float64 output is b3 (relu3 off) or max(b3, 0) itself; the deep-negative channel stays
    decisively below zero in every row; the other channels are still an admissible exposure batch"""
    case = cases.exact(relu3)
    for ch, b in cases.EXACT_ZERO:
        assert (case.layers[2][0][ch] == 0).all()
        assert (case.ref[:, ch] == (max(b, 0.) if relu3 else b)).all()
    assert {b for _, b in cases.EXACT_ZERO} == {0., 1.25, -1.25}
    ch, b = cases.EXACT_NEGATIVE
    raw = cases.exact(False)
    assert max(raw.bg_out[ch], raw.hot_out[:, ch].max()) <= -raw.dec
    if relu3:
        assert (case.ref[:, ch] == 0).all()
    hot_wins, bg_wins = cases.decided(case)
    assert min(hot_wins.sum(1).min(), bg_wins.sum(1).min()) >= 32


def test_dense_batches_are_permuted_for_real():
    """the invariance cases: no permutation is the identity, and no two rows of a proposal agree in a pooled channel's
    winner by construction -- the rows are i.i.d."""
    for args in (cases.INVARIANCE, cases.INVARIANCE_MODE1):
        c = cases.dense(*args)
        assert (c.perm != np.arange(c.P)).mean() > 0.99 and (c.prop_perm != np.arange(c.B)).any()
        assert sorted(c.prop_perm) == list(range(c.B)) and (np.sort(c.perm, 1) == np.arange(c.P)).all()
        x = torch.from_numpy(c.x)
        moved = cases.permute_rows(x, c.P, c.perm).numpy().reshape(c.B, c.P, c.d)
        for b in range(c.B):
            np.testing.assert_array_equal(moved[b], c.x.reshape(c.B, c.P, c.d)[b][c.perm[b]])


def test_strided_view():
    x = torch.arange(5 * 64, dtype=torch.float32).view(5, 64)
    for ldx in (66, 68, 128):
        v = cases.strided(x, ldx)
        assert v.stride() == (ldx, 1) and v.storage_offset() == 4 and torch.equal(v, x)
        assert (v.data_ptr() - v.untyped_storage().data_ptr()) == 16
    assert cases.strided(x, 68, shift=1).storage_offset() == 1


@pytest.mark.parametrize("P", cases.HEAD_P)
def test_head_cases_are_admissible(P):
    """distinct gbias per proposal: consecutive proposals' scores of the one x row differ decisively (in some class);
    the shared-gbias scores are one value"""
    own, shared = cases.head_one_row_ref(P, False), cases.head_one_row_ref(P, True)
    assert own.shape == (cases.HEAD_B, 2) and (shared == shared[0]).all()
    dec = chain_f64.decisive(own)
    apart = np.abs(own[1:] - own[:-1]).max(1)
    print("head P %d: |score| up to %.2f, decisive gap %.2e, consecutive proposals at least %.2e apart"
          % (P, np.abs(own).max(), dec, apart.min()))
    assert apart.min() >= dec
    c = cases.head(P)
    assert (c.perm != np.arange(P)).mean() > 0.95 and cases.HEAD_B > 256
