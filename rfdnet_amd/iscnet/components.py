"""Connected components of a mesh batch on the device: label the faces of all K meshes of a scene at once, measure every
component, and drop the floaters -- keep the largest component of every mesh, or every one above a fraction of it -- on
the flat buffers marching cubes leaves (csrc/mesh_components.hip, include/rfd_components.h: the six rules;
tests/components_f64.py restates them in numpy float64).

Meshes that come out of marching cubes over a learned or fused field carry small detached blobs and inside-out inner
shells; every later stage pays for them.  Two faces belong together if they name a common vertex index (positions play
no part).  The labelling is a lock-free union-find over the vertex indices whose result is unique (the root of a set is
its smallest index), the measures are fixed-shape sums, and between the kernels stand stable sorts and prefix sums: the
result does not depend on the grid, the batch or the order of execution.  No floating-point atomics.  A call reads back
from the device twice at most, whatever K: the component offsets, and the new mesh offsets with the kept counts."""
import math
import numbers

import numpy as np
import torch

from .. import _lib, mesh_batch, ragged

MEASURES = {'faces': 0, 'area': 1, 'abs_volume': 2}            # RFD_COMPONENTS_BY_* of include/rfd_components.h


def parse_keep(keep):
    """'largest' or a fraction t in [0, 1] -> (largest_only, t); ValueError for anything else"""
    if isinstance(keep, str):
        if keep != 'largest':
            raise ValueError("keep must be 'largest' or a fraction in [0, 1], not %r" % (keep,))
        return True, 1.0
    if isinstance(keep, bool) or not isinstance(keep, numbers.Real):
        raise ValueError("keep must be 'largest' or a fraction in [0, 1], not %r" % (keep,))
    t = float(keep)
    if math.isnan(t) or t < 0.0 or t > 1.0:
        raise ValueError("the fraction to keep must lie in [0, 1], not %r" % (keep,))
    return False, t


def parse_measure(measure):
    if measure not in MEASURES:
        raise ValueError("measure must be one of %s, not %r" % (sorted(MEASURES), measure))
    return MEASURES[measure]


def _batch(f, vend, tend):
    """the checked offsets and the faces as the kernels read them"""
    vend, tend, K = mesh_batch.check_offsets(vend, tend)
    V, F = int(vend[-1]), int(tend[-1])
    assert f.shape[0] >= F
    return vend, tend, K, V, F


def _label(ff, vend, tend, K, V, F):
    """rules 1 to 3 for F > 0 faces over V > 0 vertices -> dict: glabel, llabel (F) i32, vlabel (V) i32, corner (F,3) i32,
    cbase_d (K + 1) i32 on the device, cbase (list), C, vend_d, tend_d.  One D2H copy: cbase."""
    dev = ff.device
    vend_d, tend_d = ragged.to_int32(np.stack([vend, tend]), dev)
    parent = torch.arange(V, dtype=torch.int32, device=dev)
    _lib.call("rfd_components_union", dev, F, K, V, ff.data_ptr(), tend_d.data_ptr(), vend_d.data_ptr(), parent.data_ptr())
    root = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.call("rfd_components_flatten", dev, V, parent.data_ptr(), root.data_ptr())
    froot = torch.empty(F, dtype=torch.int32, device=dev)
    corner = torch.empty(F, 3, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, V, dtype=torch.int32, device=dev)
    is_root, named = flags[0], flags[1]
    _lib.call("rfd_components_face_roots", dev, F, K, V, ff.data_ptr(), tend_d.data_ptr(), vend_d.data_ptr(),
              root.data_ptr(), froot.data_ptr(), corner.data_ptr(), is_root.data_ptr(), named.data_ptr())
    # rule 3: a root is its set's smallest index, so the roots in ascending order are the components in theirs
    rincl = torch.cumsum(is_root, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    cbase_d = torch.cat([zero, rincl])[vend_d.long()].contiguous()
    glabel = torch.empty(F, dtype=torch.int32, device=dev)
    llabel = torch.empty(F, dtype=torch.int32, device=dev)
    vlabel = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.call("rfd_components_labels", dev, F, K, V, froot.data_ptr(), root.data_ptr(), named.data_ptr(),
              rincl.data_ptr(), tend_d.data_ptr(), cbase_d.data_ptr(), glabel.data_ptr(), llabel.data_ptr(),
              vlabel.data_ptr())
    cbase = cbase_d.cpu().tolist()
    return {'glabel': glabel, 'llabel': llabel, 'vlabel': vlabel, 'corner': corner, 'cbase_d': cbase_d, 'cbase': cbase,
            'C': cbase[-1], 'vend_d': vend_d, 'tend_d': tend_d}


def _measure(vv, lab, F, V):
    """rule 4 for C > 0 components -> faces, vertices (C) i32, area, volume (C) f64, lo, hi (C,3) f64"""
    dev, C = vv.device, lab['C']
    rowptr, col = mesh_batch.corner_csr(lab['glabel'], C)                   # component -> faces, ascending
    vptr, _ = mesh_batch.corner_csr(lab['vlabel'], C)                       # component -> the vertices it names
    faces = torch.empty(C, dtype=torch.int32, device=dev)
    sums = torch.empty(2, C, dtype=torch.float64, device=dev)
    box = torch.empty(2, C, 3, dtype=torch.float64, device=dev)
    _lib.call("rfd_components_measure", dev, C, F, V, int(vv.dtype == torch.float32), vv.data_ptr(),
              lab['corner'].data_ptr(), rowptr.data_ptr(), col.data_ptr(), faces.data_ptr(), sums[0].data_ptr(),
              sums[1].data_ptr(), box[0].data_ptr(), box[1].data_ptr())
    return faces, vptr[1:] - vptr[:-1], sums[0], sums[1], box[0], box[1]


@torch.no_grad()
def label_components(f, vend, tend):
    """f (F,3) integer faces with indices local to their mesh, vend / tend the K + 1 vertex / face offsets
    -> (local (F,) i32: the component of every face within its mesh, -1 for a face with an index outside its mesh;
        glob (F,) i32: the same counted over the batch, cbase[k] + local;  n_components: K ints;  cbase: K + 1 ints, their
        prefix sum).  Components are numbered in ascending order of the smallest vertex index they name."""
    vend, tend, K, V, F = _batch(f, vend, tend)
    _lib.need_gpu(f)
    if K == 0 or F == 0 or V == 0:                      # no face, or none that could be valid
        none = torch.full((F,), -1, dtype=torch.int32, device=f.device)
        return none, none.clone(), [0] * K, [0] * (K + 1)
    lab = _label(f[:F].to(torch.int32).contiguous(), vend, tend, K, V, F)
    cbase = lab['cbase']
    return lab['llabel'], lab['glabel'], [cbase[k + 1] - cbase[k] for k in range(K)], cbase


def _from_labels(labels, ff, vend, tend, K, V, F):
    """what _label returns, from the tuple label_components returned for the same batch (no kernel, no D2H copy)"""
    dev = ff.device
    glabel, cbase = labels[1], [int(c) for c in labels[3]]
    if glabel.shape[0] != F or len(cbase) != K + 1 or glabel.device != dev:
        raise ValueError("labels: not what label_components returned for this batch")
    glabel = glabel.to(torch.int32).contiguous()
    vend_d, tend_d = ragged.to_int32(np.stack([vend, tend]), dev)
    first = torch.repeat_interleave(vend_d[:-1], (tend_d[1:] - tend_d[:-1]).long(), output_size=F)
    valid = (glabel >= 0)[:, None]
    corner = torch.where(valid, ff + first[:, None], torch.full_like(ff, -1)).contiguous()
    vlabel = torch.full((V + 1,), -1, dtype=torch.int32, device=dev)        # row V: where the invalid faces' corners go
    vlabel[torch.where(valid, corner, torch.full_like(corner, V)).reshape(-1).long()] = \
        torch.where(valid, glabel[:, None], torch.full_like(corner, -1)).reshape(-1)
    return {'glabel': glabel, 'vlabel': vlabel[:V].contiguous(), 'corner': corner, 'cbase': cbase, 'C': cbase[-1],
            'cbase_d': ragged.to_int32(np.asarray(cbase), dev), 'vend_d': vend_d, 'tend_d': tend_d}


@torch.no_grad()
def component_measures(v, f, vend, tend, labels=None):
    """v (V,3) f64 / f32, f, vend, tend as in label_components; labels: what label_components returned for this batch
    (default: it is called here) -> dict of tensors over the C components of the batch: 'mesh' (C,) i32, 'faces', 'vertices'
    (C,) i32, 'area', 'volume' (C,) f64 (volume is signed, and means something for a closed component only), 'lo', 'hi'
    (C,3) f64: the bounding box of the finite coordinates."""
    vend, tend, K, V, F = _batch(f, vend, tend)
    mesh_batch.check_tensors(v, f)
    dev = v.device
    assert v.shape[0] >= V
    lab = None
    if K and F and V:
        ff = f[:F].to(torch.int32).contiguous()
        lab = _label(ff, vend, tend, K, V, F) if labels is None else _from_labels(labels, ff, vend, tend, K, V, F)
    if lab is None or lab['C'] == 0:
        i, d = (lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)), \
               (lambda *s: torch.empty(*s, dtype=torch.float64, device=dev))
        return {'mesh': i(0), 'faces': i(0), 'vertices': i(0), 'area': d(0), 'volume': d(0), 'lo': d(0, 3), 'hi': d(0, 3)}
    faces, vertices, area, volume, lo, hi = _measure(v[:V].contiguous(), lab, F, V)
    ids = torch.arange(lab['C'], dtype=torch.int32, device=dev)
    mesh = torch.searchsorted(lab['cbase_d'][1:].contiguous(), ids, right=True).int()
    return {'mesh': mesh, 'faces': faces, 'vertices': vertices, 'area': area, 'volume': volume, 'lo': lo, 'hi': hi}


@torch.no_grad()
def keep_components(v, f, vend, tend, keep='largest', measure='area', drop_cavities=False, return_info=False):
    """v (V,3) f64 / f32 vertices, f (F,3) i32 faces with indices local to their mesh, vend / tend the K + 1 vertex / face
    offsets (Generator3D.last_buffers).  keep: 'largest' (the largest component of every mesh alone) or a fraction t in
    [0, 1] (every component with measure >= t times the largest's: 0 keeps all); measure: 'faces', 'area' or 'abs_volume';
    drop_cavities: also drop every component whose signed volume has the other sign than the largest's (an inside-out
    shell inside an object)
    -> (v2 (V2,3) in v's dtype, the kept rows of v bit for bit; f2 (F2,3) i32; vend2, tend2): the filtered batch in the same
    layout [, {'found': components of every mesh, 'kept': how many of them stay}].  Faces with an index outside their mesh
    are never kept.  ValueError for an unknown measure or keep, before anything is allocated."""
    vend, tend, K, V, F = _batch(f, vend, tend)
    largest_only, t = parse_keep(keep)
    by = parse_measure(measure)
    mesh_batch.check_tensors(v, f)
    dev = v.device
    assert v.shape[0] >= V

    def answer(v2, f2, vend2, tend2, found, kept):
        return (v2, f2, vend2, tend2, {'found': found, 'kept': kept}) if return_info else (v2, f2, vend2, tend2)

    def empty():
        return answer(torch.empty(0, 3, dtype=v.dtype, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                      [0] * (K + 1), [0] * (K + 1), [0] * K, [0] * K)
    if K == 0 or V == 0 or F == 0:          # nothing a face could name
        return empty()
    vv = v[:V].contiguous()
    ff = f[:F].to(torch.int32).contiguous()
    lab = _label(ff, vend, tend, K, V, F)                                   # the first D2H copy
    C, cbase = lab['C'], lab['cbase']
    if C == 0:
        return empty()
    flags = _select(lab, _measure(vv, lab, F, V), K, F, V, by, largest_only, t, drop_cavities)
    v2, f2, vend2, tend2, kept = _compact(vv, lab, flags, K, F, V)         # the second D2H copy
    return answer(v2, f2, vend2, tend2, [cbase[k + 1] - cbase[k] for k in range(K)], kept)


def _select(lab, measures, K, F, V, by, largest_only, t, drop_cavities):
    """rule 5 and rule 6's flags -> keep (F) u8, used (V) i32, kept (K) i32, on the device"""
    faces, _, area, volume, _, _ = measures
    dev, C = faces.device, lab['C']
    keep_comp = torch.empty(C, dtype=torch.uint8, device=dev)
    kept_d = torch.empty(K, dtype=torch.int32, device=dev)
    _lib.call("rfd_components_select", dev, K, C, by, int(largest_only), t, int(bool(drop_cavities)),
              lab['cbase_d'].data_ptr(), faces.data_ptr(), area.data_ptr(), volume.data_ptr(), keep_comp.data_ptr(),
              kept_d.data_ptr())
    keep_f = torch.empty(F, dtype=torch.uint8, device=dev)
    used = torch.zeros(V, dtype=torch.int32, device=dev)
    _lib.call("rfd_components_mark", dev, F, C, V, lab['glabel'].data_ptr(), lab['corner'].data_ptr(),
              keep_comp.data_ptr(), keep_f.data_ptr(), used.data_ptr())
    return keep_f, used, kept_d


def _compact(vv, lab, flags, K, F, V):
    """rule 6: the new offsets and the kept counts (one D2H copy), then the kept faces and vertices"""
    keep_f, used, kept_d = flags
    dev = vv.device
    vincl, fincl, bounds = mesh_batch.compacted_offsets(used, keep_f, lab['vend_d'].long(), lab['tend_d'].long())
    back = torch.cat([bounds.reshape(-1), kept_d]).cpu().tolist()
    vend2, tend2, kept = back[:K + 1], back[K + 1:2 * K + 2], back[2 * K + 2:]
    V2, F2 = vend2[-1], tend2[-1]
    v2 = torch.empty(V2, 3, dtype=vv.dtype, device=dev)
    f2 = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    if F2 and V2:
        _lib.call("rfd_components_compact_faces", dev, F, K, V, lab['tend_d'].data_ptr(), lab['corner'].data_ptr(),
                  keep_f.data_ptr(), fincl.data_ptr(), vincl.data_ptr(), bounds[0].data_ptr(), f2.data_ptr())
        _lib.call("rfd_components_gather_vertices", dev, V, V2, int(vv.dtype == torch.float32), vv.data_ptr(),
                  used.data_ptr(), vincl.data_ptr(), v2.data_ptr())
    return v2, f2, vend2, tend2, kept
