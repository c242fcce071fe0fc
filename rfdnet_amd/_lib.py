"""ctypes binding of librfd_hip.so -- the C-ABI boundary (include/*.h).

The product path has NO CPU fallback: if the HIP library is missing or fails to
load, importing an op raises.  (The CPU oracle under oracle/ is test
infrastructure and is never imported from this package.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RFD_HIP_LIB: load another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("RFD_HIP_LIB") or os.path.join(_HERE, "lib", "librfd_hip.so")

_f = C.c_void_p      # device pointers travel as integers (tensor.data_ptr())
_i = C.c_int
_fl = C.c_float
_sz = C.c_size_t
_d = C.c_double

# name -> (restype, argtypes[, OPTIONAL]): exactly the prototypes of include/rfd_pointnet2.h / rfd_occ.h /
# rfd_chamfer.h / rfd_eval.h / rfd_latent.h / rfd_loss.h / rfd_fit.h / rfd_render.h / rfd_decimate.h / rfd_simplify.h / rfd_fuse.h / rfd_sample.h / rfd_labels.h / rfd_mesh_eval.h / rfd_objgrid.h / rfd_mesh_dist.h / rfd_components.h / rfd_knn.h.  OPTIONAL marks the test hooks, which a deployment build (RFD_NO_TEST_HOOKS=1, build.py)
# leaves out.
OPTIONAL = "optional"
ABI = {
    "furthest_point_sampling_kernel_wrapper": (_i, [_i, _i, _i, _f, _f, _f, _f]),
    "gather_points_kernel_wrapper": (_i, [_i, _i, _i, _i, _f, _f, _f, _f]),
    "gather_points_grad_kernel_wrapper": (_i, [_i, _i, _i, _i, _f, _f, _f, _f]),
    "query_ball_point_kernel_wrapper": (_i, [_i, _i, _i, _fl, _i, _f, _f, _f, _f]),
    "group_points_kernel_wrapper": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f]),
    "group_points_grad_kernel_wrapper": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f]),
    "three_nn_kernel_wrapper": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "three_interpolate_kernel_wrapper": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f]),
    "three_interpolate_grad_kernel_wrapper": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_group_concat": (_i, [_i, _i, _i, _i, _i, _fl, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_furthest_point_sampling_gather": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_chamfer_forward": (_i, [_i, _i, _f, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_chamfer_backward": (_i, [_i, _i, _f, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_sa_fused": (_i, [_i, _i, _i, _i, _i, _fl, _i, _f, _f, _f, _f, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_occ_pack_weights": (_i, [_f, _f, C.POINTER(C.c_int), _i, _f, _f]),
    "rfd_occ_decode": (_i, [_i, _f, _f, _f, _f, _f, _f, _f, _fl, _f, _i, _f]),
    "rfd_occ_pack_weights_w8": (_i, [_f, _f, C.POINTER(C.c_int), _i, _f, _f]),
    "rfd_occ_decode_w8": (_i, [_i, _f, _f, _f, _f, _f, _f, _f, _fl, _f, _i, _f]),
    "rfd_occ_decode_scatter_w8": (_i, [_i, _f, _f, _f, _f, _f, _f, _f, _fl, _f, _f, _f, C.c_longlong, _i, _f]),
    "rfd_occ_chunk_range": (_i, [_i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rfd_occ_chunk_range_capped": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rfd_occ_set_launch_shape": (_i, [_i, _i, _i]),
    "rfd_occ_set_tail_tiles": (_i, [_i]),
    "rfd_occ_normals_w8": (_i, [_i, _f, _f, _f, _i, _f, _f, C.POINTER(C.c_int), _f, _f, _f, _f, _f, _i, _f]),
    "rfd_refine_sample": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_refine_face_backward": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _fl, _f, _f]),
    "rfd_refine_vertex_step": (_i, [_i, _f, _f, _i, _f, _f, _f, _f, _f]),
    "rfd_refine_dirichlet": (_i, [_i, C.c_ulonglong, _i, _f, _f]),
    "rfd_fps_set_timeout_ms": (_i, [_i]),
    "rfd_fps_set_geometry": (_i, [_i]),
    "rfd_test_hold_cus": (_i, [_i, _f, _i, _f], OPTIONAL),
    "rfd_fps_test_phantom_units": (_i, [_i], OPTIONAL),
    "rfd_make_grid_points": (_i, [_i, _fl, _fl, _fl, _f, _i, _f]),
    "rfd_mise_init": (_i, [_i, _i, _i, _f, _f, _f]),
    "rfd_mise_count": (_i, [_i, _i, _i, _f, _f, _f]),
    "rfd_mise_collect": (_i, [_i, _i, _i, _f, _f, _f, _fl, _f, _f, _f]),
    "rfd_mise_scatter": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_mise_subdivide": (_i, [_i, _i, _i, C.c_double, _f, _f, _f, _f]),
    "rfd_mise_subdivide_active": (_i, [_i, _i, _i, C.c_double, _f, _f, _f, _f, _f]),
    "rfd_mise_subdivide_dirty": (_i, [_i, _i, _i, C.c_double, _f, _f, _f, _f, C.c_longlong, _f, _f, _f, _f, _i, _f]),
    "rfd_mise_to_dense": (_i, [_i, _i, _i, _f, _f, _f]),
    "rfd_points_in_boxes": (_i, [_i, _i, _i, _i, _f, _f, _f, _f]),
    "rfd_nms3d": (_i, [_i, _i, C.c_double, _i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_gemm_pack_w": (_i, [_i, _i, _i, _f, _f, _f]),
    "rfd_gemm_f16x3": (_i, [_i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _i, _f, _i, _i, _i, _i, _i, _f, _i, _f]),
    "rfd_mc_classify": (_i, [_i, _i, _fl, C.c_double, _f, _f, _f, _f, _f]),
    "rfd_mc_emit_affine": (_i, [_i, _i, _fl, C.c_double, _f, _f, _f, _f, _f, _f, _f, C.c_double, C.c_double, _f]),
    "rfd_mc_blocks": (_i, [_i]),
    "rfd_occ_fold_rows": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _i, _f, _f]),
    "rfd_rows3_rotate_z": (_i, [_i, _i, _f, _f, _f, _f]),
    "rfd_rows3_affine": (_i, [_i, _i, _f, _f, _f, _f]),
    "rfd_mlp_cols": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_three_interpolate_cat": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_chain_pack_n": (_i, [_i, _i, _f, _f, _f, _i, _i, _i, _f, _f]),
    "rfd_chain_pool_n": (_i, [_i, _i, _i, _i, _i, _f, _i, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f]),
    "rfd_head_pack": (_i, [_f, _f, _f, _i, _i, _i, _f, _f]),
    "rfd_head_scores": (_i, [_i, _i, _f, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, _i, _i, _f, _f]),
    "rfd_pos_embed": (_i, [_i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _i, _f, _i, _i, _f]),
    "rfd_pos_embed_frag": (_i, [_i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _i, _f, C.c_long, _i, _f]),
    "rfd_rows_to_frag": (_i, [_i, _i, _f, _i, _i, _i, _f, C.c_long, _f]),
    "rfd_frag_to_rows": (_i, [_i, _i, _f, C.c_long, _i, _f, _i, _f]),
    "rfd_gemm_f16x3_frag": (_i, [_i, _i, _i, _f, C.c_long, _f, _f, C.c_long, _f, _f, _i, _i, _i, _i, _f, _i, _f]),
    "rfd_box3d_iou": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_ap_match": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_latent_prep": (_i, [_i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_latent_stage": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_latent_head": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_bce_logits_rowsum": (_i, [_i, _i, _f, _i, _f, _i, _f, _f]),
    "rfd_voxel_iou": (_i, [_i, _i, _f, _i, _fl, _f, _f, _f, _f]),
    "rfd_vote_loss_partial": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_proposal_loss_partial": (_i, [_i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, C.POINTER(C.c_int), _f, _i, _f, _f,
                                       _f, _f, _f, _f, _f, _f, _f, _f, _i, _f, _f]),
    "rfd_detection_loss_finish": (_i, [_i, _i, _i, _f, _f, _f]),
    "rfd_mask_loss_partial": (_i, [_i, _i, _f, _f, _i, _f, _f, _f, _f]),
    "rfd_mask_loss_finish": (_i, [_i, _i, _fl, _f, _f, _f]),
    "rfd_fit_pose_run": (_i, [_i, _i, _i, _i, _i, _i, C.c_double, C.c_double, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f,
                              _f, _f]),
    "rfd_raster_project": (_i, [_i, _i, _i, _f, _f, C.POINTER(C.c_double), C.c_double, _f, _f, _f, _f]),
    "rfd_raster_triangles": (_i, [_i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_raster_shade": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, C.POINTER(C.c_double), _f, _f, _f, _f, _f]),
    "rfd_decimate_vertex_keys": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_decimate_face_remap": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_decimate_parity": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_decimate_cell_solve": (_i, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, C.c_double, _f, _f]),
    "rfd_decimate_compact_faces": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_init": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_quadrics": (_i, [_i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_edges": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_edge_costs": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_vertex_min": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_select": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_apply": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_simplify_compact_faces": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_depth_from_keys":(_i, [_i, _i, _f, _fl, _fl, _f, _f]),
    "rfd_tsdf_fuse": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _i, _fl, _fl, _i, _fl, _i, _f, _f, _f]),
    "rfd_sample_rescale": (_i, [_i, _f, _d, _d, _d, _d, _d, _d, _i, _f, _f, _f]),
    "rfd_sample_cells": (_i, [_i, _f, _i, _f, _f, _f]),
    "rfd_sample_contains": (_i, [_i, _f, _d, _d, _d, _d, _d, _d, _i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_sample_voxelize": (_i, [_i, _f, _i, _f, _f]),
    "rfd_sample_face_areas": (_i, [_i, _f, _f, _f]),
    "rfd_sample_surface": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_labels_instance_aabb": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_labels_cad_extents": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_labels_match_instances": (_i, [_i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_labels_point_votes": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_labels_sample": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _d, _d, _fl, C.POINTER(C.c_double), _f, _f, _f, _f, _f,
                               _f, _f, _f, _f]),
    "rfd_objgrid_pack": (_i, [_i, _f, _f, _f, C.c_longlong, C.c_longlong, _f, _f]),
    "rfd_objgrid_surface": (_i, [_i, _f, _f, _i, _f, _f, _f, _f, C.c_longlong, _f, _f]),
    "rfd_objgrid_bins": (_i, [_i, _f, _f, _i, _f, _f, _f, _f, _f, _i, _f]),
    "rfd_objgrid_interior": (_i, [_i, _f, _i, _f, _f, _f, _f, C.c_longlong, _f, _f, _f, _i, _f, _f]),
    "rfd_objgrid_finish": (_i, [_i, _f, _f, _f, _f, C.c_longlong, _f, _f, _f, _f]),
    "rfd_mesh_iou_counts": (_i, [_i, _i, _f, _f, _f, _f, C.c_longlong, _f, _f, _f, _f, C.c_longlong, _f, _f]),
    "rfd_mesh_iou_finalize": (_i, [_i, _i, _f, _f, _f, _f, _f, _i, _i, _f, _f]),
    "rfd_mdist_faces": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_mdist_cells": (_i, [_i, _f, _i, _f, _f, _f]),
    "rfd_mdist_query": (_i, [_i, _f, _f, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_mdist_sample": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_mdist_sums": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _i, _f, _f, _f, _f]),
    "rfd_components_union": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_components_flatten": (_i, [_i, _f, _f, _f]),
    "rfd_components_face_roots": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_components_labels": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_components_measure": (_i, [_i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_components_select": (_i, [_i, _i, _i, _i, _d, _i, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_components_mark": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "rfd_components_compact_faces": (_i, [_i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_components_gather_vertices": (_i, [_i, _i, _i, _f, _f, _f, _f, _f]),
    "rfd_knn_points": (_i, [_i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "rfd_knn_cells": (_i, [_i, _f, _i, _f, _f, _i, _f, _f, _f]),
    "rfd_knn_query": (_i, [_i, _f, _f, _i, _d, _f, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f, _i, _f, _f, _f, _f]),
    "rfd_knn_sums": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _f, _f, _f, _i, _f, _f, _f, _f]),
    "rfd_last_error_string": (C.c_char_p, []),
    "rfd_build_arch": (C.c_char_p, []),
    "rfd_device_status": (_i, []),
    "rfd_occ_packed_bytes": (_sz, []),
    "rfd_stream_status": (_i, [_f]),
    "rfd_release_stream": (_i, [_f]),
    "rfd_stream_status_snapshot": (_i, [_f, _f]),
    "rfd_mise_vstate_elems": (_sz, [_i, _i]),
    "rfd_mise_dirty_elems": (_sz, [_i, _i]),
    "rfd_gemm_packed_bytes": (_sz, [_i, _i]),
    "rfd_chain_packed_bytes_n": (_sz, [_i]),
    "rfd_head_packed_bytes": (_sz, []),
    "rfd_fit_pose_workspace_bytes": (_sz, [_i, _i]),
}
SIGNATURES = {name: entry[1] for name, entry in ABI.items()}      # name -> argtypes (tests read it)

_lib = None

# Lazily built, cached artefacts (packed weight streams, folded BatchNorms, stacked weights) are shared by every host
# thread that runs the same network (bench.py: several scenes in flight on one model): build_once() builds them.
import threading as _threading
BUILD_LOCK = _threading.RLock()


def publish(device=None):
    """drain the current stream of `device`: what was just built on it is complete for every other stream"""
    import torch
    if torch.cuda.is_available():
        torch.cuda.current_stream(device).synchronize()


def sync_device(device):
    """wait for everything queued on `device`, by any host thread on any stream (ArtefactCache's eviction)"""
    import torch
    torch.cuda.synchronize(device)


def tensor_key(*tensors):
    """(address, version, shape, device) of each tensor, None for None: a cache key for what was built from them.  The
    address is part of it, so the tensors must live as long as the entry (ArtefactCache's `keep`)."""
    return tuple(None if t is None else (t.data_ptr(), t._version, t.shape, t.device) for t in tensors)


def build_once(store, slot, key, build, device):
    """store[slot] = (key, build()) unless it already holds `key`; -> the value.  The one way a shared artefact is
    built: a miss is built under BUILD_LOCK, published on `device` (if a CUDA device: build() need not wait for its
    own launches) and stored in one assignment, so a thread that finds it may use it on its own stream at once.  A
    per-object cache passes its __dict__ and a fixed slot name: the slot's old value is dropped, unsynchronised, when
    the key changes, i.e. only when the object's parameters change, and they must not change under scenes in flight."""
    hit = store.get(slot)
    if hit is None or hit[0] != key:
        with BUILD_LOCK:
            hit = store.get(slot)
            if hit is None or hit[0] != key:
                value = build()
                if getattr(device, "type", None) == "cuda":
                    publish(device)
                hit = store[slot] = (key, value)
    return hit[1]


class ArtefactCache(object):
    """get(key, build, device, keep) -> build()'s value, built by build_once, for at most `limit` keys; `keep` (the
    tensors the key was made of) is held with it.  A miss on a full cache evicts ONE entry, the least recently built,
    and releases it only after sync_device() if it was built for a CUDA device: other host threads launch on streams
    of their own and torch's allocator tracks the allocating stream only, so a device-wide wait is the one condition
    under which no queued kernel can still read the tensor.  It costs the inference path nothing: a cache fills only
    after hundreds of distinct weights (repeated checkpoint loads).  All of this runs under BUILD_LOCK."""

    def __init__(self, limit):
        self.limit, self.store = limit, {}

    def get(self, key, build, device, keep=None):
        def build_entry():
            entry = (build(), keep)
            while len(self.store) >= self.limit:
                _, (old, old_device) = self.store.pop(next(iter(self.store)))      # dicts keep insertion order
                if getattr(old_device, "type", None) == "cuda":
                    sync_device(old_device)
                del old
            return entry, device
        return build_once(self.store, key, key, build_entry, device)[0][0]


class RfdHipError(RuntimeError):
    pass


def lib():
    """Load librfd_hip.so (once).  Raises if it is absent -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RfdHipError(
                "librfd_hip.so not built (%s). Run `python -m rfdnet_amd.build` "
                "or __graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so).  It must
        # be in the process BEFORE our library is loaded so the dynamic loader
        # resolves our DT_NEEDED libamdhip64 to that same copy: two HIP
        # runtimes in one process cannot share device pointers or streams (the
        # second one reports "no ROCm-capable device").
        import torch  # noqa: F401
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def bind(cdll):
    """Give every ABI entry of `cdll` its restype / argtypes; -> cdll.  A required symbol that is missing raises; a
    missing OPTIONAL one (a test hook of a deployment build) is bound to a function that raises when called."""
    for name, (restype, argtypes, *optional) in ABI.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
        elif optional:
            setattr(cdll, name, _absent_hook(name))
        else:
            raise RfdHipError("%s: symbol %s is missing (stale build? run `python -m rfdnet_amd.build --force`)"
                              % (getattr(cdll, "_name", None) or LIB_PATH, name))
    return cdll


def _absent_hook(name):
    def absent(*args):
        raise RfdHipError("%s is a test hook: this library was built with RFD_NO_TEST_HOOKS" % name)
    return absent


def exported_symbols():
    return sorted(ABI)


def ptr(t):
    """the device pointer of an optional tensor argument"""
    return None if t is None else t.data_ptr()


def rows(t):
    """(K,T) tensor -> (t', ld): the rows as a kernel reads them, `ld` elements apart.  A row-strided view (unit stride
    along T, rows that do not overlap) is read in place, anything else through a contiguous copy; one row, or one
    column, has no stride to respect."""
    K, T = t.shape
    if (T > 1 and t.stride(1) != 1) or (K > 1 and t.stride(0) < T):
        t = t.contiguous()
    return t, int(t.stride(0)) if K > 1 else T


def as_tensor(a, device, dtype):
    """numpy (or anything numpy converts) or a tensor -> a tensor on `device` of `dtype`; no copy when it already is"""
    import numpy as np
    import torch
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device, dtype)


def need_gpu(*tensors):
    """The one guard of the host modules: RuntimeError("CPU not supported") (the reference's wording, sampling.cpp:34 et
    al.) unless every argument is a tensor on a CUDA device.  None is refused too: pass only what the call requires."""
    import torch
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("CPU not supported")


def call(name, device, *args):
    """The one way a host module launches: ABI entry `name` (one whose last C parameter is the stream) with `args` and
    the current stream of `device`, on that device; a non-zero return raises, naming `name`."""
    import torch
    with torch.cuda.device(device):
        rc = getattr(lib(), name)(*args, current_stream())
    check(rc, name)


def check(rc, what):
    """hipError_t -> Python exception (the reference exit(-1)s instead,
    cuda_utils.h:30-39)."""
    if rc != 0:
        msg = lib().rfd_last_error_string()
        raise RfdHipError("%s failed (hipError %d): %s" % (what, rc, (msg or b"").decode()))


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# flags of the device status word (include/rfd_pointnet2.h)
STATUS_FPS_ABORT = 1
STATUS_DECODER_RANGE = 2
STATUS_GEMM_RANGE = 4


def _raise_status(st):
    if st < 0:
        raise RfdHipError("rfd_device_status failed")
    msgs = []
    if st & STATUS_FPS_ABORT:
        msgs.append("furthest point sampling aborted: its workgroups were not resident together within the "
                    "exchange time-out (partitioned / CU-masked / oversubscribed GPU?)")
    if st & STATUS_DECODER_RANGE:
        msgs.append("occupancy decoder: activation exceeded the f16 range")
    if st & STATUS_GEMM_RANGE:
        msgs.append("split-precision GEMM: activation exceeded the f16 range")
    if msgs:
        e = RfdHipError("; ".join(msgs))
        e.status = st
        raise e
    return st


def raise_status(st):
    """Raise for the flags in `st` (as returned by *_status_bits)."""
    return _raise_status(st)


def stream_status_bits():
    """The current stream's status word (waits for that stream, clears the word), no exception for set flags."""
    st = lib().rfd_stream_status(current_stream())
    if st < 0:
        raise RfdHipError("rfd_stream_status failed")
    return st


_snap_pool = []
_snap_lock = _threading.Lock()


class StatusSnapshot(object):
    """The current stream's status word as it stood when the snapshot was taken (and reset, in stream order).
    Every snapshot has a pinned word of its own (from a small pool it goes back to at the first read()), so a second
    snapshot on the same stream cannot overwrite the first one's flags before they are read, and
    read() waits for the snapshot's own event: the caller need not have synchronised the stream."""

    def __init__(self):
        import torch
        s = torch.cuda.current_stream()
        with _snap_lock:
            buf = _snap_pool.pop() if _snap_pool else None
        if buf is None:
            buf = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.buf, self.value = buf, None
        st = lib().rfd_stream_status_snapshot(s.cuda_stream, buf.data_ptr())
        if st < 0:
            raise RfdHipError("rfd_stream_status_snapshot failed")
        self.event = torch.cuda.Event()
        self.event.record(s)

    def read(self):
        if self.value is None:
            self.event.synchronize()
            self.value = int(self.buf[0]) & 0xffffffff
            with _snap_lock:
                if len(_snap_pool) < 64:
                    _snap_pool.append(self.buf)
            self.buf = None
        return self.value


def release_stream(stream=None):
    """Return the status slot of `stream` (default: the current one) to the pool; raises for flags still pending."""
    import torch
    st = lib().rfd_release_stream((stream or torch.cuda.current_stream()).cuda_stream)
    return _raise_status(st)


def device_status():
    """Synchronises the DEVICE; raises if a persistent kernel flagged a problem."""
    return _raise_status(lib().rfd_device_status())


def stream_status():
    """Waits for the current stream only, then reads the same status word."""
    return _raise_status(lib().rfd_stream_status(current_stream()))
