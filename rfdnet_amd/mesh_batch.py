"""The host side of a flat mesh batch (v, f, vend, tend): K meshes laid back to back, the ragged batch of ragged.py with two
prefixes, `vend` over the vertices and `tend` over the faces, whose indices are local to their mesh
(Generator3D.last_buffers).  What the stages over such a batch share: the checks of their arguments, the vertex -> corner
rows they walk on the device, and the new offsets a stage that drops vertices and faces ends with (csrc/mesh_batch.h is
the device side)."""
import numpy as np
import torch

from . import _lib, ragged


def _ascending(end, what):
    end = np.asarray([int(x) for x in end], dtype=np.int64)
    if end.ndim != 1 or end.size < 1 or end[0] != 0 or (np.diff(end) < 0).any():
        raise ValueError("%s: K + 1 ascending offsets starting at 0" % what)
    ragged.offsets(np.diff(end))            # the total stays below 2^31
    return end


def check_offsets(vend, tend):
    """-> (vend, tend, K): the offsets as int64 arrays of K + 1 entries each.  ValueError for anything else."""
    vend, tend = _ascending(vend, "vend"), _ascending(tend, "tend")
    if len(tend) != len(vend):
        raise ValueError("vend and tend describe %d and %d meshes" % (len(vend) - 1, len(tend) - 1))
    return vend, tend, len(vend) - 1


def check_tensors(v, f):
    """the batch is on a GPU (RuntimeError) and its vertices are float64 or float32 (TypeError)"""
    _lib.need_gpu(v, f)
    if v.dtype not in (torch.float64, torch.float32):
        raise TypeError("vertices must be float64 or float32, not %s" % v.dtype)


def corner_csr(faces, n_rows):
    """faces (F,3) integer tensor of row indices (GLOBAL vertex indices, or whatever its corners are grouped by)
    -> (rowptr (n_rows + 1,) i32, col (3F,) i32): the corners 3 f + c of row r are col[rowptr[r]:rowptr[r+1]], ascending
    (a stable sort of the flattened faces).  A row no face names is empty; an index outside [0, n_rows), a dead face's
    -1 -1 -1 included, is in no row.  No host synchronisation."""
    flat = faces.reshape(-1).long().clamp(max=n_rows)
    assert flat.numel() < 2 ** 31
    skey, col = torch.sort(torch.where(flat >= 0, flat, n_rows), stable=True)
    rowptr = torch.searchsorted(skey, torch.arange(n_rows + 1, dtype=torch.int64, device=faces.device))
    return rowptr.int(), col.int()


def compacted_offsets(used, keep, v_at, f_at):
    """used / keep: the flags of the rows that become vertices and of the faces that stay; v_at / f_at (K + 1,) int64:
    where the meshes begin among them -> (vincl, fincl: the inclusive prefix sums, i32; bounds (2, K + 1) i32: the new
    vend and tend, still on the device so that the caller decides what else its one D2H copy carries)"""
    vincl = torch.cumsum(used, 0, dtype=torch.int32)
    fincl = torch.cumsum(keep, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=used.device)
    return vincl, fincl, torch.stack([torch.cat([zero, vincl])[v_at], torch.cat([zero, fincl])[f_at]])
