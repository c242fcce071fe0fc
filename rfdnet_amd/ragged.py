"""The host side of a ragged batch (DESIGN.md "Ragged batches"): K segments of unequal length laid back to back in flat
buffers, described by an exclusive prefix `off` (K + 1), an owner map (the segment of every item) and a block map (the
segments cut into blocks of a fixed size that never span two segments).  Functions over small host arrays, nothing else:
numpy in, numpy out (int64 unless said otherwise); to_int32() and uniform_maps() are the two that touch a device.
Every consumer indexes with int32, so every total is checked against 2^31 here, before anything of that size exists."""
from collections import namedtuple

import numpy as np
import torch

INT32_END = 2 ** 31


def offsets(counts):
    """per-segment counts (K) -> the exclusive prefix (K + 1,): segment k owns off[k] .. off[k+1]; an empty segment repeats
    an offset.  ValueError when the total does not fit an int32."""
    off = np.zeros(np.size(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64).reshape(-1), out=off[1:])
    if off[-1] >= INT32_END:
        raise ValueError("ragged batch of %d items: the total must stay below 2^31 (int32 offsets)" % off[-1])
    return off


def owners(counts):
    """per-segment counts (K) -> (sum,): the segment of every item"""
    offsets(counts)                     # the range check, before the array is made
    return np.repeat(np.arange(np.size(counts)), np.asarray(counts, dtype=np.int64).reshape(-1))


def blocks(counts, size):
    """the number of `size`-blocks of every segment (ceiling division; an empty segment has none)"""
    return (np.asarray(counts, dtype=np.int64) + (size - 1)) // size


PaddedTiles = namedtuple('PaddedTiles', 'per prefix owner slot')


def padded_tiles(counts, size):
    """The padded-tile layout: every segment rounded up to whole blocks of `size` slots -> PaddedTiles(per (K): the blocks
    of every segment, prefix (K + 1): their exclusive prefix, owner (prefix[-1]): the segment of every block (tile_prop),
    slot (K + 1) = size * prefix: where every segment's slots begin; slot[-1] slots in all).  ValueError when the PADDED
    slot count does not fit an int32."""
    per = blocks(counts, size).reshape(-1)
    prefix = offsets(per)
    slot = prefix * size
    if slot[-1] >= INT32_END:
        raise ValueError("ragged batch padded to %d slots of %d-blocks: the total must stay below 2^31 (int32 offsets)"
                         % (slot[-1], size))
    return PaddedTiles(per, prefix, owners(per), slot)


def runs(counts, step):
    """The unpadded-run layout: every segment cut into runs of at most `step` items -> (owner, start) int32 arrays, one
    entry per run: its segment and its first item's row in the flat buffer."""
    off = offsets(counts)
    per = blocks(counts, step).reshape(-1)
    owner = owners(per)
    start = off[owner] + (np.arange(len(owner)) - offsets(per)[owner]) * step
    return owner.astype(np.int32), start.astype(np.int32)


def to_int32(a, device, non_blocking=False):
    """host integer array, 1-D or stacked 2-D -> one contiguous int32 tensor on `device` (ONE copy: the rows of a
    stacked array are views of it).  ValueError for a value outside the int32 range."""
    a = np.asarray(a)
    if a.ndim not in (1, 2) or (a.size and a.dtype.kind not in 'iu'):
        raise ValueError("to_int32: a 1-D or 2-D integer array, not %s %s" % (a.dtype, a.shape))
    if a.size and (int(a.min()) < -INT32_END or int(a.max()) >= INT32_END):
        raise ValueError("to_int32: values in [%d, %d] do not fit an int32" % (a.min(), a.max()))
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device, non_blocking=non_blocking)


def uniform_maps(K, per, device, src=True):
    """K segments of `per` blocks each that all read ONE source list of `per` blocks, built on the device
    -> (tile_prop (K * per) i32: the segment of every block, tile_src (K * per) i32: the source block it reads, or None
    with src=False)"""
    tile_prop = torch.arange(K, dtype=torch.int32, device=device).repeat_interleave(per)
    return tile_prop, torch.arange(per, dtype=torch.int32, device=device).repeat(K) if src else None
