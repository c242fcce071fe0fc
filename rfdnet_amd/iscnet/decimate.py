"""Mesh decimation on the device: vertex clustering with a quadric-placed representative per cell, for all K meshes of
a scene at once on the flat buffers marching cubes leaves (csrc/mesh_decimate.hip, include/rfd_decimate.h: the five
rules; tests/decimate_f64.py restates them in numpy float64).

The reference thins a mesh by sequential quadric edge collapse on the host (generator.py:189-191, simplify_mesh); its
parallel form, with a face budget and the topology kept, is simplify.py.  Clustering is the cheap thinning: every vertex falls into a cell
of a `cells`^3 grid over its mesh's cube, every occupied cell becomes one vertex placed where the quadrics of the
faces around it are smallest (kept inside the cell), faces that collapse are dropped, coincident survivors are
reduced mod 2 (so a closed mesh keeps even edge counts), and what no face names any more is compacted away.
Deterministic: stable sorts and prefix sums between the kernels, fixed-shape sums inside them, no atomics."""
import numpy as np
import torch

from .. import _lib, mesh_batch, ragged

PADDING = 0.1           # Generator3D's default: the default cube is [-(1 + PADDING) / 2, (1 + PADDING) / 2]^3
REGULARISE = 1e-3       # a choice, not a tuned value: pulls a badly conditioned quadric solve towards the weighted mean


def default_cube(K, cells, padding=PADDING):
    """the generator's cube for K meshes -> lo (K,3) f64, h (K,) f64"""
    box = 1.0 + padding
    return np.full((K, 3), -box / 2, dtype=np.float64), np.full(K, box / cells, dtype=np.float64)


@torch.no_grad()
def decimate_meshes(v, f, vend, tend, cells, lo=None, h=None, regularise=REGULARISE):
    """v (V,3) f64 / f32 vertices, f (F,3) i32 faces with indices local to their mesh, vend / tend the K + 1 vertex / face
    offsets (Generator3D.last_buffers), cells: the grid of every mesh's cube, lo (K,3) / h (K,): origin and cell size of
    every mesh (default: default_cube()), regularise: see REGULARISE
    -> (v2 (V2,3) f32, f2 (F2,3) i32, vend2, tend2): the decimated batch in the same layout; the offsets (Python lists)
    come back through one small D2H copy.  ValueError for cells < 1 or K cells^3 >= 2^31, before anything is allocated."""
    vend, tend, K = mesh_batch.check_offsets(vend, tend)
    cells = int(cells)
    if cells < 1:
        raise ValueError("cells must be >= 1, not %d" % cells)
    if K * cells ** 3 >= ragged.INT32_END:
        raise ValueError("%d meshes of %d^3 cells: the keys must stay below 2^31 (int32)" % (K, cells))
    mesh_batch.check_tensors(v, f)
    if lo is None or h is None:
        dlo, dh = default_cube(K, cells)
        lo, h = dlo if lo is None else lo, dh if h is None else h
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (K, 3)))
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (K,)))
    with np.errstate(all='ignore'):
        inv_h = 1.0 / h
    if not (np.isfinite(lo).all() and np.isfinite(h).all() and (h > 0).all() and np.isfinite(inv_h).all()):
        raise ValueError("lo must be finite and h finite and positive (with a finite reciprocal)")
    regularise = float(regularise)
    if not regularise >= 0.0:
        raise ValueError("regularise must be >= 0")
    dev = v.device
    V, F = int(vend[-1]), int(tend[-1])
    assert v.shape[0] >= V and f.shape[0] >= F

    def empty():
        return (torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                [0] * (K + 1), [0] * (K + 1))
    if K == 0 or V == 0 or F == 0:          # nothing a face could name
        return empty()
    vv = v[:V].contiguous()
    ff = f[:F].to(torch.int32).contiguous()
    is_f32 = int(vv.dtype == torch.float32)
    vend_d, tend_d = ragged.to_int32(np.stack([vend, tend]), dev)
    par = torch.from_numpy(np.concatenate([lo.reshape(-1), h, inv_h])).to(dev)
    lo_d, h_d, inv_d = par[:3 * K], par[3 * K:4 * K], par[4 * K:]

    # rules 1 and 2: keys, then the occupied cells in ascending key order
    per = cells ** 3
    key = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.call("rfd_decimate_vertex_keys", dev, V, K, cells, is_f32, vv.data_ptr(), vend_d.data_ptr(), lo_d.data_ptr(),
              inv_d.data_ptr(), key.data_ptr())
    skey, order = torch.sort(key, stable=True)
    cellkey, group = torch.unique_consecutive(skey, return_inverse=True)
    C = cellkey.numel() - int(cellkey[-1] == K * per)                       # the last group: vertices without a cell
    if C == 0:
        return empty()
    cellkey = cellkey[:C].contiguous()
    vcell = torch.empty(V, dtype=torch.int32, device=dev)
    vcell[order] = torch.where(group < C, group, torch.full_like(group, -1)).int()

    # rule 4: remap and flag, then the survivors grouped by candidate set (two stable sorts: top, then pair)
    fcell = torch.empty(F, 3, dtype=torch.int32, device=dev)
    pair = torch.empty(F, dtype=torch.int64, device=dev)
    top = torch.empty(F, dtype=torch.int32, device=dev)
    alive = torch.empty(F, dtype=torch.uint8, device=dev)
    _lib.call("rfd_decimate_face_remap", dev, F, K, C, ff.data_ptr(), tend_d.data_ptr(), vend_d.data_ptr(),
              vcell.data_ptr(), fcell.data_ptr(), pair.data_ptr(), top.data_ptr(), alive.data_ptr())
    keep = torch.zeros(F, dtype=torch.uint8, device=dev)
    used = torch.zeros(C, dtype=torch.int32, device=dev)
    live = torch.nonzero(alive).view(-1)                                    # ascending face index
    n = live.numel()
    if n == 0:
        return empty()
    by_top = torch.sort(top[live], stable=True).indices
    by_pair = torch.sort(pair[live][by_top], stable=True).indices
    s_face = live[by_top[by_pair]]
    s_pair, s_top, s_face = pair[s_face].contiguous(), top[s_face].contiguous(), s_face.int().contiguous()
    _lib.call("rfd_decimate_parity", dev, n, C, F, s_pair.data_ptr(), s_top.data_ptr(), s_face.data_ptr(),
              fcell.data_ptr(), keep.data_ptr(), used.data_ptr())

    # rule 5: the new offsets (the one D2H copy), then positions of the used cells and the kept faces
    first_cell = torch.searchsorted(cellkey, torch.arange(K + 1, dtype=torch.int64, device=dev).mul_(per).int())
    vincl, fincl, bounds = mesh_batch.compacted_offsets(used, keep, first_cell, tend_d.long())
    vend2, tend2 = bounds.cpu().tolist()
    V2, F2 = vend2[-1], tend2[-1]
    if F2 == 0:
        return empty()
    v2 = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    f2 = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    rowptr, col = mesh_batch.corner_csr(fcell, C)                           # cell -> corners 3 face + c, ascending
    dst = torch.where(used > 0, vincl - 1, torch.full_like(vincl, -1))
    _lib.call("rfd_decimate_cell_solve", dev, C, K, F, cells, is_f32, vv.data_ptr(), ff.data_ptr(), vend_d.data_ptr(),
              cellkey.data_ptr(), rowptr.data_ptr(), col.data_ptr(), dst.data_ptr(), lo_d.data_ptr(), h_d.data_ptr(),
              regularise, v2.data_ptr())
    _lib.call("rfd_decimate_compact_faces", dev, F, K, tend_d.data_ptr(), fcell.data_ptr(), keep.data_ptr(),
              fincl.data_ptr(), vincl.data_ptr(), bounds[0].data_ptr(), f2.data_ptr())
    return v2, f2, vend2, tend2
