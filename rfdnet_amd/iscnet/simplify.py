"""Mesh simplification on the device: quadric edge collapse to a face budget, in parallel rounds, for all K meshes of a
ragged batch at once (csrc/mesh_simplify.hip, include/rfd_simplify.h: rules S0-S7; tests/simplify_f64.py restates them).

The reference thins a mesh with external/libsimplify (generator.py:189-191, simplify_mesh; 3_simplify_fusion.py): every
edge whose quadric error is under a rising threshold is collapsed, one after another on the host.  Here a round ranks
every legal edge by its cost and collapses those that are the cheapest in the one-rings of both their ends, so their stars
are disjoint and the round is one launch per step; the link condition keeps the topology, the reference's flip guard the
normals, frozen vertices the borders and whatever is not manifold.  Unlike clustering (decimate.py) it meets a face
budget, spends the faces where the curvature is and leaves a watertight mesh watertight.  Deterministic: stable sorts and
prefix sums between the kernels, integer minima inside them."""
import numpy as np
import torch

from .. import _lib, mesh_batch, ragged

MAX_ROUNDS = 1000       # a bound, not a tuned value: a round removes a few per cent of the faces, or nothing (then it stops)
INT32_MAX = 2 ** 31 - 1


def _targets(n_faces, K):
    n = np.asarray(n_faces)
    if n.dtype.kind not in 'iu':
        raise TypeError("n_faces must be an int or K ints, not %s" % n.dtype)
    if n.ndim > 1 or (n.ndim == 1 and n.size != K):
        raise ValueError("n_faces: one target, or one per mesh (%d)" % K)
    n = np.ascontiguousarray(np.broadcast_to(n.astype(np.int64), (K,)))
    if (n < 0).any():
        raise ValueError("n_faces must be >= 0")
    return np.minimum(n, INT32_MAX)


@torch.no_grad()
def simplify_meshes(v, f, vend, tend, n_faces, max_rounds=MAX_ROUNDS, stats=None):
    """v (V,3) f64 / f32 vertices, f (F,3) i32 faces with indices local to their mesh, vend / tend the K + 1 vertex / face
    offsets (Generator3D.last_buffers), n_faces: the target of every mesh (an int, or K ints)
    -> (v2 (V2,3) f64, f2 (F2,3) i32, vend2, tend2, reached (K,) bool tensor on the host): the simplified batch in the
    same layout.  A mesh with no more faces than its target comes back bit for bit; reached[k] says whether mesh k got
    down to its target (a mesh of frozen vertices, or one whose every collapse would pinch or flip, cannot).  One small
    D2H copy per round.  stats: a dict that receives 'rounds', 'launches' (of this module's kernels) and 'host_syncs'.
    ValueError / TypeError for bad offsets or targets before anything is allocated."""
    vend, tend, K = mesh_batch.check_offsets(vend, tend)
    n_faces = _targets(n_faces, K)
    max_rounds = int(max_rounds)
    if max_rounds < 0:
        raise ValueError("max_rounds must be >= 0")
    mesh_batch.check_tensors(v, f)
    dev = v.device
    V, F = int(vend[-1]), int(tend[-1])
    assert v.shape[0] >= V and f.shape[0] >= F
    count = {'rounds': 0, 'launches': 0, 'host_syncs': 0}
    takes_part = np.diff(tend) > n_faces
    if F == 0 or not takes_part.any():
        if stats is not None:
            stats.update(count)
        return (v[:V].double().clone(), f[:F].to(torch.int32).clone(), vend.tolist(), tend.tolist(),
                torch.ones(K, dtype=torch.bool))

    def call(name, *args):
        count['launches'] += 1
        _lib.call(name, dev, *args)

    vv = v[:V].contiguous() if V else torch.zeros(1, 3, dtype=v.dtype, device=dev)      # a vertex of no mesh
    V1 = max(V, 1)
    ff = f[:F].to(torch.int32).contiguous()
    is_f32 = int(vv.dtype == torch.float32)
    small = ragged.to_int32(np.stack([vend, tend, np.append(n_faces, 0), np.append(takes_part, 0)]), dev)
    vend_d, tend_d, nf_d, takes_d = small[0], small[1], small[2, :K], small[3, :K].to(torch.uint8)
    pos = torch.empty(V1, 3, dtype=torch.float64, device=dev)
    nonfinite = torch.empty(V1, dtype=torch.uint8, device=dev)
    face = torch.empty(F, 3, dtype=torch.int32, device=dev)
    call("rfd_simplify_init", V1, F, K, is_f32, vv.data_ptr(), ff.data_ptr(), vend_d.data_ptr(), tend_d.data_ptr(),
         nf_d.data_ptr(), pos.data_ptr(), nonfinite.data_ptr(), face.data_ptr())
    rowptr, col = mesh_batch.corner_csr(face, V1)                           # dead faces (-1 -1 -1) are in no row
    Q = torch.empty(V1, 10, dtype=torch.float64, device=dev)
    call("rfd_simplify_quadrics", V1, F, pos.data_ptr(), face.data_ptr(), rowptr.data_ptr(), col.data_ptr(), Q.data_ptr())

    n = 3 * F
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    tend_l = tend_d.long()
    slots = torch.arange(n, dtype=torch.int64, device=dev)
    meshes = torch.arange(K + 1, dtype=torch.int64, device=dev)

    def alive_and_need():
        incl = torch.cat([zero, torch.cumsum(face[:, 0] >= 0, 0)])[tend_l]
        alive = incl[1:] - incl[:-1]
        return alive, torch.clamp((alive - nf_d + 1) // 2, min=0)       # a mesh that takes no part has no alive face

    ea, eb, emesh, rank = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    eface, eapex = (torch.empty(n, 2, dtype=torch.int32, device=dev) for _ in range(2))
    efrozen, legal, sel = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    epos = torch.empty(n, 3, dtype=torch.float64, device=dev)
    need = alive_and_need()[1]
    pending = int(need.sum())
    count['host_syncs'] += 1
    while pending > 0 and count['rounds'] < max_rounds:
        count['rounds'] += 1
        if count['rounds'] > 1:
            rowptr, col = mesh_batch.corner_csr(face, V1)
        # S0: the half-edges 3 face + c (corner c to the next) grouped by edge, dead ones last
        a, b = face.reshape(-1).long(), face[:, [1, 2, 0]].reshape(-1).long()
        key = torch.where(a >= 0, torch.minimum(a, b) * V1 + torch.maximum(a, b), torch.full_like(a, V1 * V1))
        skey, horder = torch.sort(key, stable=True)
        horder = horder.int()
        vfrozen = nonfinite.clone()
        call("rfd_simplify_edges", V1, F, skey.data_ptr(), horder.data_ptr(), face.data_ptr(), ea.data_ptr(), eb.data_ptr(),
             eface.data_ptr(), eapex.data_ptr(), efrozen.data_ptr(), vfrozen.data_ptr())
        # S2, S3
        call("rfd_simplify_edge_costs", V1, F, K, vend_d.data_ptr(), ea.data_ptr(), eb.data_ptr(), eapex.data_ptr(),
             efrozen.data_ptr(), vfrozen.data_ptr(), face.data_ptr(), pos.data_ptr(), Q.data_ptr(), rowptr.data_ptr(),
             col.data_ptr(), cost.data_ptr(), epos.data_ptr(), legal.data_ptr(), emesh.data_ptr())
        # S4: the slots are in (a, b) order, so a stable sort by cost ranks by (cost, a, b)
        order = torch.sort(cost, stable=True).indices
        rank[order] = slots.int()
        m1 = torch.full((V1,), INT32_MAX, dtype=torch.int32, device=dev)
        call("rfd_simplify_vertex_min", V1, F, 0, ea.data_ptr(), eb.data_ptr(), legal.data_ptr(), rank.data_ptr(), None,
             m1.data_ptr())
        m2 = m1.clone()
        call("rfd_simplify_vertex_min", V1, F, 1, ea.data_ptr(), eb.data_ptr(), None, None, m1.data_ptr(), m2.data_ptr())
        call("rfd_simplify_select", V1, F, ea.data_ptr(), eb.data_ptr(), legal.data_ptr(), rank.data_ptr(), m2.data_ptr(),
             sel.data_ptr())
        # the budget: the selected edges in rank order, grouped by mesh; the first need[k] of mesh k are kept
        by_mesh = torch.where(sel[order] > 0, emesh[order].long(), torch.full_like(order, K))
        s_mesh, idx = torch.sort(by_mesh, stable=True)
        first = torch.searchsorted(s_mesh, meshes)
        within = (slots - first[s_mesh]) < torch.cat([need, zero])[s_mesh]
        keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        keep[order[idx]] = within.to(torch.uint8)
        # S5
        call("rfd_simplify_apply", V1, F, keep.data_ptr(), ea.data_ptr(), eb.data_ptr(), eface.data_ptr(), epos.data_ptr(),
             rowptr.data_ptr(), col.data_ptr(), pos.data_ptr(), Q.data_ptr(), face.data_ptr())
        need = alive_and_need()[1]
        kept, pending = torch.stack([keep.sum(), need.sum()]).cpu().tolist()      # the round's one D2H copy
        count['host_syncs'] += 1
        if kept == 0:
            break

    # S7 (a mesh that takes no part keeps every face and every vertex)
    alive_k = alive_and_need()[0]
    part_f = takes_d[torch.bucketize(torch.arange(F, device=dev), tend_l[1:], right=True).clamp_(max=K - 1)] > 0
    part_v = takes_d[torch.bucketize(torch.arange(V1, device=dev), vend_d.long()[1:], right=True).clamp_(max=K - 1)] > 0
    keep_f = ((face[:, 0] >= 0) | ~part_f).to(torch.uint8)
    used = torch.zeros(V1 + 1, dtype=torch.bool, device=dev)
    flat = face.reshape(-1).long()
    used[torch.where(flat >= 0, flat, torch.full_like(flat, V1))] = True
    used = used[:V1] | ~part_v
    if V == 0:
        used[:] = False
    vincl, fincl, bounds = mesh_batch.compacted_offsets(used, keep_f, vend_d.long(), tend_l)
    vend2, tend2, alive_h = torch.cat([bounds, torch.cat([alive_k, zero]).int()[None]]).cpu().tolist()
    count['host_syncs'] += 1
    v2 = pos[used]
    f2 = torch.empty(tend2[-1], 3, dtype=torch.int32, device=dev)
    if tend2[-1]:
        call("rfd_simplify_compact_faces", V1, F, K, ff.data_ptr(), face.data_ptr(), vend_d.data_ptr(), tend_d.data_ptr(),
             takes_d.data_ptr(), keep_f.data_ptr(), fincl.data_ptr(), vincl.data_ptr(), bounds[0].data_ptr(), f2.data_ptr())
    if stats is not None:
        stats.update(count)
    return v2, f2, vend2, tend2, torch.from_numpy(np.asarray(alive_h[:K], dtype=np.int64) <= n_faces)


def simplify_mesh(vertices, faces, n_faces, max_rounds=MAX_ROUNDS):
    """the one-mesh form, named after the reference's (libsimplify's simplify_mesh(mesh, f_target)): vertices (V,3) f64 /
    f32 and faces (F,3) integer tensors on the device -> (vertices (V2,3) f64, faces (F2,3) i32)"""
    _lib.need_gpu(vertices, faces)
    v2, f2, _, _, _ = simplify_meshes(vertices.reshape(-1, 3), faces.reshape(-1, 3), [0, vertices.reshape(-1, 3).shape[0]],
                                      [0, faces.reshape(-1, 3).shape[0]], int(n_faces), max_rounds=max_rounds)
    return v2, f2
