"""CPU: rfdnet_amd/ragged.py, the host side of a ragged batch (DESIGN.md "Ragged batches"), against the expressions its
callers wrote out by hand before the module existed -- the concatenate / cumsum prefix, the np.repeat owner map, the Python
loop of DecoderCBatchNorm.normals for the group prefix, the per-round tile arithmetic of Generator3D._grids_mise and the
double loop of fit.fit_tiles, all restated literally below.  Equality is exact and dtypes are checked; the layout's
properties (no block spans two segments, an empty segment owns none, a segment's blocks are consecutive) are checked
on every case as well."""
import tracemalloc

import numpy as np
import pytest
import torch

from rfdnet_amd import ragged

CASES = [[], [0], [0, 0, 0], [1], [256], [257], [0, 5, 0, 1024, 1, 0], [255, 256, 257, 0, 1025],
         np.random.default_rng(0).integers(0, 5000, size=40).tolist()]
SIZES = [128, 16, 256, 1024]
ids = lambda c: "K%d_n%d" % (len(c), sum(c))


# ---- the expressions the module replaced ---------------------------------------------------------------------------------
def prefix_by_hand(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])


def owners_by_hand(counts):
    return np.repeat(np.arange(len(counts)), np.asarray(counts, np.int64))


def group_prefix_loop(counts, size):
    gprefix = [0]
    for n in counts:
        gprefix.append(gprefix[-1] + (n + size - 1) // size)
    return gprefix


def fit_tiles_loop(n_scan_points, step):
    tile_obj, tile_start, at = [], [], 0
    for p, n in enumerate(n_scan_points):
        for s in range(at, at + n, step):
            tile_obj.append(p)
            tile_start.append(s)
        at += n
    return np.asarray(tile_obj, np.int32), np.asarray(tile_start, np.int32)


def same(got, want):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape)
    np.testing.assert_array_equal(got, want)


# ---- prefix, owners, blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", CASES, ids=ids)
def test_offsets_and_owners(counts):
    off = ragged.offsets(counts)
    same(off, prefix_by_hand(counts))
    assert off.dtype == np.int64 and off.shape == (len(counts) + 1,) and off[0] == 0
    own = ragged.owners(counts)
    same(own, owners_by_hand(counts))
    assert own.shape == (sum(counts),)
    for k, n in enumerate(counts):                          # an empty segment repeats an offset and owns nothing
        assert off[k + 1] - off[k] == n and np.all(own[off[k]:off[k + 1]] == k)
    same(ragged.offsets(np.asarray(counts, np.int32)), off)                     # any integer input, same answer


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("counts", CASES, ids=ids)
def test_blocks_and_group_prefix(counts, size):
    per = ragged.blocks(counts, size)
    same(per, np.asarray([-(-n // size) for n in counts], np.int64))
    assert all(b == 0 for b, n in zip(per, counts) if n == 0)
    gprefix = ragged.offsets(per)
    assert gprefix.dtype == np.int64 and gprefix.tolist() == group_prefix_loop(counts, size)
    assert int(ragged.blocks(sum(counts), size)) == -(-sum(counts) // size)     # a plain number: the uniform callers


# ---- padded tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("counts", CASES, ids=ids)
def test_padded_tiles(counts, size):
    K = len(counts)
    cnt = np.asarray(counts, np.int64)
    # Generator3D._grids_mise and refine_meshes, as they were
    tiles = (cnt + size - 1) // size
    offs = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * size if K else np.zeros(0, np.int64)
    tprefix = np.concatenate([[0], np.cumsum(tiles)])
    tile_prop = np.repeat(np.arange(K, dtype=np.int32), tiles)

    got = ragged.padded_tiles(counts, size)
    same(got.per, tiles)
    same(got.prefix, tprefix.astype(np.int64))
    same(got.owner.astype(np.int32), tile_prop)
    assert got.owner.dtype == np.int64
    same(got.slot[:-1], offs.astype(np.int64))
    assert got.slot.dtype == np.int64 and got.slot[-1] == size * tiles.sum() and len(got.owner) == tiles.sum()
    # properties: block b holds the slots b * size .. (b + 1) * size; segment k's items sit at slot[k] .. slot[k] + counts[k]
    for k in range(K):
        mine = np.nonzero(got.owner == k)[0]
        assert len(mine) == (0 if counts[k] == 0 else -(-counts[k] // size))
        assert mine.tolist() == list(range(got.prefix[k], got.prefix[k + 1]))   # consecutive, in segment order
        assert got.slot[k + 1] - got.slot[k] == len(mine) * size                 # whole blocks: none spans two segments
        assert got.slot[k] + counts[k] <= got.slot[k + 1] < got.slot[k] + counts[k] + size


# ---- unpadded runs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("counts", CASES, ids=ids)
def test_runs(counts, size):
    owner, start = ragged.runs(counts, size)
    want_owner, want_start = fit_tiles_loop(counts, size)
    same(owner, want_owner)
    same(start, want_start)
    off = prefix_by_hand(counts)
    end = np.minimum(start.astype(np.int64) + size, off[owner.astype(np.int64) + 1])
    assert np.all(start >= off[owner]) and np.all(end > start)                  # inside its segment, never empty
    covered = np.concatenate([np.arange(s, e) for s, e in zip(start, end)]) if len(start) else np.zeros(0, np.int64)
    np.testing.assert_array_equal(covered, np.arange(off[-1]))                  # every item once, in order
    assert np.all(np.diff(owner) >= 0) and set(owner.tolist()) == {k for k, n in enumerate(counts) if n}


@pytest.mark.parametrize("points_per_thread,step", [(1, 256), (4, 1024)])
def test_runs_at_the_fit_kernel_steps(points_per_thread, step):
    from rfdnet_amd.iscnet import fit
    assert fit.RUN_WIDTH * points_per_thread == step
    for counts in CASES:
        got, want = ragged.runs(counts, fit.RUN_WIDTH * points_per_thread), fit_tiles_loop(counts, step)
        same(got[0], want[0])
        same(got[1], want[1])


# ---- range guards -----------------------------------------------------------------------------------------------------------
def raises_cheaply(call, match):
    tracemalloc.start()
    try:
        with pytest.raises(ValueError, match=match):
            call()
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert peak < 1 << 20, peak


def test_range_guards():
    raises_cheaply(lambda: ragged.offsets([2 ** 30, 2 ** 30]), str(2 ** 31))            # names the total
    raises_cheaply(lambda: ragged.owners([2 ** 30, 2 ** 30]), str(2 ** 31))
    raises_cheaply(lambda: ragged.runs([2 ** 30, 2 ** 30], 1024), str(2 ** 31))
    assert ragged.offsets([2 ** 31 - 100])[-1] == 2 ** 31 - 100                          # the unpadded total fits ...
    raises_cheaply(lambda: ragged.padded_tiles([2 ** 31 - 100], 128), str(2 ** 31))     # ... the padded one does not
    assert ragged.offsets([2 ** 30, 2 ** 30 - 1])[-1] == 2 ** 31 - 1                     # the last total that fits


# ---- the two device-facing helpers, on CPU tensors ---------------------------------------------------------------------------
def test_to_int32():
    counts = CASES[-1]
    tiles = ragged.padded_tiles(counts, 128)
    stacked = np.stack([ragged.offsets(counts), tiles.prefix, tiles.slot, ragged.offsets(ragged.blocks(counts, 16))])
    t = ragged.to_int32(stacked, torch.device('cpu'))
    assert t.dtype == torch.int32 and tuple(t.shape) == (4, len(counts) + 1) and t.is_contiguous()
    np.testing.assert_array_equal(t.numpy(), stacked)
    rows = list(t)
    assert len(rows) == 4
    for i, r in enumerate(rows):                            # one tensor, one copy: the rows are views of it
        assert r.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
        assert r.data_ptr() == t.data_ptr() + 4 * i * t.shape[1] and r.is_contiguous()
    flat = ragged.to_int32(tiles.owner, 'cpu')
    assert flat.dtype == torch.int32 and flat.tolist() == tiles.owner.tolist()
    assert ragged.to_int32(stacked[:, ::2], 'cpu').is_contiguous()              # a strided input comes back contiguous
    assert ragged.to_int32([], 'cpu').shape == (0,)
    assert ragged.to_int32([2 ** 31 - 1, -2 ** 31], 'cpu').tolist() == [2 ** 31 - 1, -2 ** 31]      # the range's two ends
    for bad in ([0, 2 ** 31], [-2 ** 31 - 1], np.stack([[0, 1], [2, 2 ** 40]])):
        with pytest.raises(ValueError):
            ragged.to_int32(bad, 'cpu')
    with pytest.raises(ValueError):
        ragged.to_int32(np.zeros((2, 2, 2), np.int64), 'cpu')
    with pytest.raises(ValueError):
        ragged.to_int32([0.5, 1.0], 'cpu')


@pytest.mark.parametrize("K,per", [(0, 3), (1, 1), (5, 0), (3, 7)])
def test_uniform_maps(K, per):
    dev = torch.device('cpu')
    tile_prop, tile_src = ragged.uniform_maps(K, per, dev)
    assert tile_prop.dtype == torch.int32 and tile_src.dtype == torch.int32
    assert torch.equal(tile_prop, torch.arange(K, dtype=torch.int32).repeat_interleave(per))
    assert torch.equal(tile_src, torch.arange(per, dtype=torch.int32).repeat(K))
    assert tile_prop.tolist() == ragged.owners([per] * K).tolist()              # the uniform case of the owner map
    only, none = ragged.uniform_maps(K, per, dev, src=False)
    assert none is None and torch.equal(only, tile_prop)
