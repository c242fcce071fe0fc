"""Batched mesh generator: the counterpart of Generator3D
(models/iscnet/modules/generator.py:14-197) with the reference's constructor
keywords and entry points (generate_mesh / generate_from_latent / eval_points /
extract_mesh).

The reference walks the proposals one by one (generator.py:71-74), decodes
<=100 000 points per call, copies every chunk to the host (:139) and drives a
CPU octree per proposal (:99-117).  Here ALL proposals advance together: one
fused decode launch per MISE round over the concatenated query lists, the MISE
state (values / point flags / octree flags) is dense and device-resident
(csrc/mise.hip), and only K 4-byte counters per round cross PCIe.
"""
import os

import numpy as np
import torch

from .. import _lib
from .occ_decoder import TILE, run_with_range_fallback


class Mesh(object):
    """Minimal stand-in for trimesh.Trimesh(process=False) (generator.py:181-183):
    the reference only stores vertices/faces and exports them."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = vertices
        self.faces = faces
        self.vertex_normals = vertex_normals


class Generator3D(object):
    def __init__(self, model, points_batch_size=100000, threshold=0.5, refinement_step=0,
                 resolution0=16, upsampling_steps=3, with_normals=False, padding=0.1,
                 sample=False, use_cls_for_completion=False, simplify_nfaces=None,
                 preprocessor=None):
        if refinement_step or simplify_nfaces is not None:
            # disabled by ISCNet_test.yaml:64-66; refine_mesh / libsimplify are out of scope
            raise NotImplementedError("refinement / simplification are not on the hot path")
        self.model = model
        self.round_hook = None
        self.points_batch_size = points_batch_size      # kept for signature parity; no chunking needed
        self.refinement_step = refinement_step
        self.threshold = threshold
        self.resolution0 = resolution0
        self.upsampling_steps = upsampling_steps
        self.with_normals = with_normals
        self.padding = padding
        self.sample = sample
        self.simplify_nfaces = simplify_nfaces
        self.preprocessor = preprocessor
        self.use_cls_for_completion = use_cls_for_completion
        # a MISE round that evaluated at most this many points per proposal on average runs its subdivision pass over the
        # dirty slabs only (identical result; 0 = never)
        self.sparse_round_points = int(os.environ.get('RFD_MISE_SPARSE_POINTS', 1024))     # (the variable: A/B runs only)
        self.stats = {}
        self.last_normals = None        # with_normals: the (V,3) f32 normals of the last extract_meshes(), all meshes
        self._round0_cache = _lib.ArtefactCache(64)     # made here: the worker views of one network share it

    # ---- reference-shaped entry points ------------------------------------------
    def generate_mesh(self, object_features, cls_codes, return_stats=True):
        """object_features (K, c_dim) -> list of K meshes (generator.py:54-76).  with_normals: every mesh's
        vertex_normals (generator.py:173-176), all K meshes in one launch after marching cubes."""
        fold = []
        grids = self.generate_grids(object_features, cls_codes, fold_out=fold)
        return self.extract_meshes(grids, fold=fold[0] if self.with_normals else None)

    def generate_from_latent(self, z, c=None, device='cuda', **kwargs):
        fold = []
        grids = self._grids(z, c, fold_out=fold)
        return self.extract_meshes(grids, fold=fold[0] if self.with_normals else None)[0]

    def eval_points(self, p, z, c=None, device='cuda', **kwargs):
        """p (T,3) -> logits (T,) for one code (generator.py:123-143)."""
        with torch.no_grad():
            return self.model.decode(p.unsqueeze(0).to(c.device), z, c, **kwargs).logits.squeeze(0)

    # ---- batched implementation --------------------------------------------------
    def logit_threshold(self):
        return float(np.log(self.threshold) - np.log(1. - self.threshold))   # generator.py:85

    def generate_grids(self, object_features, cls_codes=None, fold_out=None):
        """-> value grids (K, n, n, n) float32 on the device; n = resolution0 for
        the dense path, (resolution0 << upsampling_steps) + 1 for MISE."""
        self.model.eval()
        if getattr(self.model, 'use_cls_for_completion', False):
            object_features = torch.cat([object_features, cls_codes], dim=-1)
        K = object_features.size(0)
        z = self.model.get_z_from_prior((K,), sample=self.sample, device=object_features.device)
        return self._grids(z, object_features, fold_out=fold_out)

    @torch.no_grad()
    def _grids(self, z, c, fold_out=None):
        """fold_out (a list): receives the (table, fc_p_w) this call folded -- passed along by argument, not kept in an
        attribute (worker_view() copies the generator per host thread)"""
        dec = self.model.decoder
        dev = c.device
        K = c.size(0)
        box_size = 1 + self.padding                                         # generator.py:88
        table, fc_p_w = dec.fold(z.float(), c.float())
        if fold_out is not None:
            fold_out.append((table, fc_p_w))
        if self.upsampling_steps == 0:                                      # :91-97 dense shortcut
            nx = self.resolution0
            total = nx ** 3
            tiles_per = (total + TILE - 1) // TILE
            pts = torch.empty(tiles_per * TILE, 3, dtype=torch.float32, device=dev)
            _lib.call("rfd_make_grid_points", dev, nx, -0.5, 0.5, float(box_size), pts.data_ptr(),
                      tiles_per * TILE)
            tile_prop = torch.arange(K, dtype=torch.int32, device=dev).repeat_interleave(tiles_per)
            tile_src = torch.arange(tiles_per, dtype=torch.int32, device=dev).repeat(K)
            logits = dec.decode_tiles(pts, tile_prop, table, fc_p_w, tile_src=tile_src)
            self.stats = {'n_queries': K * total, 'rounds': 1, 'per_round': [K * total]}
            return logits.view(K, tiles_per * TILE)[:, :total].reshape(K, nx, nx, nx)
        return self._grids_mise(dec, table, fc_p_w, K, dev, box_size)

    def _grids_mise(self, dec, table, fc_p_w, K, dev, box_size):
        res0, depth = self.resolution0, self.upsampling_steps
        R1 = (res0 << depth) + 1
        n_per = R1 ** 3
        lib = _lib.lib()
        v_per = lib.rfd_mise_vstate_elems(res0, depth)
        values = torch.empty(K, n_per, dtype=torch.float32, device=dev)
        pstate = torch.empty(K, n_per, dtype=torch.uint8, device=dev)
        vstate = torch.empty(K, v_per, dtype=torch.uint8, device=dev)
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        # dirty-slab maps of the subdivision passes (csrc/mise.hip "dirty slabs"): two, swapped every round
        dirty = torch.zeros(2, K, lib.rfd_mise_dirty_elems(res0, depth), dtype=torch.uint8, device=dev)
        _lib.call("rfd_mise_init", dev, K, res0, depth, pstate.data_ptr(), vstate.data_ptr())
        thr = self.logit_threshold()
        n_queries, rounds = 0, 0
        per_round = []                      # real query points of each round (the rounds of generator.py:99-117)
        while True:
            shared = rounds == 0 and self._round0(res0, depth, box_size, K, dev)
            if shared:
                # round 0: every proposal asks for the same (res0+1)^3 level-0 lattice -- one
                # cached query list (points, lattice indices, tile maps), no count / collect
                # launches, no host sync, and the decoder reads 0.4 MB instead of K copies
                pts, lin, tile_prop, tile_src, total = shared
                n_tiles = tile_prop.numel()
            else:
                _lib.call("rfd_mise_count", dev, K, res0, depth, pstate.data_ptr(), counts.data_ptr())
                cnt = counts.cpu().numpy().astype(np.int64)                  # the one sync per round
                total = int(cnt.sum())
                if total == 0:                                               # generator.py:104
                    break
                tiles = (cnt + TILE - 1) // TILE
                offs = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * TILE
                n_tiles = int(tiles.sum())
                tile_prop = torch.from_numpy(np.repeat(np.arange(K, dtype=np.int32), tiles)).to(dev)
                tile_src = None
                offsets = torch.from_numpy(offs.astype(np.int32)).to(dev)
                cursors = torch.zeros(K, dtype=torch.int32, device=dev)
                pts = torch.zeros(n_tiles * TILE, 3, dtype=torch.float32, device=dev)
                lin = torch.full((n_tiles * TILE,), -1, dtype=torch.int32, device=dev)
                _lib.call("rfd_mise_collect", dev, K, res0, depth, pstate.data_ptr(), offsets.data_ptr(),
                          cursors.data_ptr(), float(box_size), pts.data_ptr(), lin.data_ptr())
            if self.round_hook is not None:           # e.g. release a host copy behind the long decode
                self.round_hook(rounds, depth)
            if dec.can_scatter():
                # MISE.update's value / known part rides in the decoder's epilogue (no logits buffer,
                # no scatter launch)
                dec.decode_tiles(pts, tile_prop, table, fc_p_w, tile_src=tile_src, scatter=(lin, values, pstate))
            else:
                logits = dec.decode_tiles(pts, tile_prop, table, fc_p_w, tile_src=tile_src)
                _lib.call("rfd_mise_scatter", dev, n_tiles, res0, depth, tile_prop.data_ptr(),
                          _lib.ptr(tile_src), lin.data_ptr(), logits.data_ptr(), values.data_ptr(), pstate.data_ptr())
            # proposals whose query was empty this round are finished (the reference's per-object loop has ended for
            # them, generator.py:104): the pass skips them; round 0 evaluates every proposal's lattice
            # a round that evaluated few points (the tail of the octree): only the slabs its points touch, and the ones the
            # previous pass created voxels in, are examined -- identical result, a fraction of the lattice traffic
            sparse = (not shared) and total <= K * self.sparse_round_points
            _lib.call("rfd_mise_subdivide_dirty", dev, K, res0, depth, float(thr), values.data_ptr(),
                      pstate.data_ptr(), vstate.data_ptr(), None if shared else counts.data_ptr(),
                      int(lin.numel()) if sparse else 0, lin.data_ptr() if sparse else None,
                      tile_prop.data_ptr() if sparse else None, dirty[rounds & 1].data_ptr(),
                      dirty[(rounds + 1) & 1].data_ptr(), int(sparse))
            n_queries += total
            per_round.append(total)
            rounds += 1
        _lib.call("rfd_mise_to_dense", dev, K, res0, depth, values.data_ptr(), pstate.data_ptr())
        self.stats = {'n_queries': n_queries, 'rounds': rounds, 'per_round': per_round}
        return values.view(K, R1, R1, R1)

    def _round0(self, res0, depth, box_size, K, dev):
        """The query list of MISE round 0 for K proposals: the list of ONE freshly initialised
        proposal (built once per configuration by the ordinary count / collect kernels, so it is
        bit-identical to what they would produce for every proposal) plus tile maps that make
        all K proposals read it.  Returns (pts, lin, tile_prop, tile_src, K * points)."""
        def build():
            R1 = (res0 << depth) + 1
            ps = torch.empty(1, R1 ** 3, dtype=torch.uint8, device=dev)
            vs = torch.empty(1, _lib.lib().rfd_mise_vstate_elems(res0, depth), dtype=torch.uint8, device=dev)
            cnt = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.call("rfd_mise_init", dev, 1, res0, depth, ps.data_ptr(), vs.data_ptr())
            _lib.call("rfd_mise_count", dev, 1, res0, depth, ps.data_ptr(), cnt.data_ptr())
            n = int(cnt.item())
            tiles_per = (n + TILE - 1) // TILE
            pts = torch.zeros(tiles_per * TILE, 3, dtype=torch.float32, device=dev)
            lin = torch.full((tiles_per * TILE,), -1, dtype=torch.int32, device=dev)
            offsets = torch.zeros(1, dtype=torch.int32, device=dev)
            cursors = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call("rfd_mise_collect", dev, 1, res0, depth, ps.data_ptr(), offsets.data_ptr(),
                      cursors.data_ptr(), float(box_size), pts.data_ptr(), lin.data_ptr())
            tile_prop = torch.arange(K, dtype=torch.int32, device=dev).repeat_interleave(tiles_per)
            tile_src = torch.arange(tiles_per, dtype=torch.int32, device=dev).repeat(K)
            return pts, lin, tile_prop, tile_src, K * n
        return self._round0_cache.get((res0, depth, float(box_size), K, str(dev)), build, dev)   # per K: NMS changes it

    # ---- mesh extraction ------------------------------------------------------------
    def extract_meshes(self, grids, fold=None):
        """fold = (table, fc_p_w) of the codes the grids came from: vertex normals from the decoder's gradient
        (Generator3D.estimate_normals), one launch for all meshes"""
        from .mcubes import marching_cubes_batch
        thr = self.logit_threshold()
        n = grids.shape[1]
        box_size = 1 + self.padding
        # generator.py:163-168, all four steps: `-= 0.5` ("libmcubes shifts by 0.5" -- the library
        # returns plain index coordinates, so this IS part of the reference's result: its demo
        # meshes sit half a cell low, tests/test_mcubes_golden.py), `-= 1` (padding),
        # `/= n - 1`, `box * (v - 0.5)`: box * ((v - 1.5) / (n - 1) - 0.5) = a * v + c, applied by the
        # emitting kernel itself as one fma per coordinate (differs from the four-op form by rounding
        # only, ~1e-16; until round 6 a second pass over the 24 B / vertex buffer of all K meshes)
        a = box_size / (n - 1)
        v, f, vend, tend = marching_cubes_batch(grids, thr, pad_value=-1e6, return_flat=True,
                                                affine=(a, -1.5 * a - 0.5 * box_size))
        self.last_buffers = (v, f, vend, tend)
        self.last_normals = None
        if fold is None:
            return [Mesh(v[vend[k]:vend[k + 1]], f[tend[k]:tend[k + 1]]) for k in range(len(vend) - 1)]
        # generator.py:173-176: normals of every non-empty mesh; the reference leaves them None on an empty one
        nrm = self.last_normals = self.model.decoder.normals(v, vend, fold[0], fold[1])
        return [Mesh(v[vend[k]:vend[k + 1]], f[tend[k]:tend[k + 1]],
                     nrm[vend[k]:vend[k + 1]] if vend[k + 1] > vend[k] else None) for k in range(len(vend) - 1)]

    def estimate_normals(self, vertices, z, c=None, device='cuda'):
        """generator.py:200-224: vertices (V,3) numpy (rounded to fp32 like torch.FloatTensor), one code z (Z,), c (C,)
        -> numpy (V,3) f32 normals -g / |g| of the decoder's logit (NaN where the gradient is exactly zero)."""
        dec = self.model.decoder
        dev = c.device if c is not None and c.is_cuda else torch.device(device)
        v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float64)).to(dev)
        with torch.no_grad():
            z, c = z.reshape(1, -1).float().to(dev), c.reshape(1, -1).float().to(dev)
            nrm = run_with_range_fallback(dec, lambda: dec.normals(v, [0, v.shape[0]], *dec.fold(z, c)), dev)
        return nrm.cpu().numpy()

    def extract_mesh(self, occ_hat, z=None, c=None):
        g = torch.as_tensor(occ_hat, dtype=torch.float32)
        if not g.is_cuda:
            g = g.cuda()
        return self.extract_meshes(g.unsqueeze(0))[0]
