"""Batched mesh generator: the counterpart of Generator3D
(models/iscnet/modules/generator.py:14-197) with the reference's constructor
keywords and entry points (generate_mesh / generate_from_latent / eval_points /
extract_mesh).

The reference walks the proposals one by one (generator.py:71-74), decodes
<=100 000 points per call, copies every chunk to the host (:139) and drives a
CPU octree per proposal (:99-117).  Here ALL proposals advance together: one
fused decode launch per MISE round over the concatenated query lists, the MISE
state (values / point flags / octree flags) is dense and device-resident
(csrc/mise.hip), and only K 4-byte counters per round cross PCIe.  The optional mesh
refinement (generator.py:226-289, one autograd loop per mesh in the reference) is
one device loop over all K meshes as well: set_refinement() / refine_meshes().
"""
import os

import numpy as np
import torch

from .. import _lib, mesh_batch, ragged
from .occ_decoder import GROUP, MODE_F16X3, TILE, logit_threshold, run_with_range_fallback


class Mesh(object):
    """Minimal stand-in for trimesh.Trimesh(process=False) (generator.py:181-183):
    the reference only stores vertices/faces and exports them."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = vertices
        self.faces = faces
        self.vertex_normals = vertex_normals


def draw_dirichlet(face_counts, steps):
    """The barycentric weights of `steps` refinement steps for meshes of face_counts faces -> (steps, sum, 3) f32, drawn from
    numpy's global stream mesh by mesh, step by step: the order of the reference's per-object loop (generator.py:71-74 around
    :254-260), so a seeded run consumes the same stream.  Rounded to f32 as the reference uploads them (:260)."""
    total = int(sum(face_counts))
    out = np.empty((steps, total, 3), dtype=np.float32)
    at = 0
    for n in face_counts:
        for it in range(steps):
            if n:                   # the reference never refines an empty mesh (generator.py:186-187)
                out[it, at:at + n] = np.random.dirichlet((0.5, 0.5, 0.5), size=n)
        at += n
    return out


class Generator3D(object):
    def __init__(self, model, points_batch_size=100000, threshold=0.5, refinement_step=0,
                 resolution0=16, upsampling_steps=3, with_normals=False, padding=0.1,
                 sample=False, use_cls_for_completion=False, simplify_nfaces=None,
                 preprocessor=None):
        if refinement_step or simplify_nfaces is not None:
            # disabled by ISCNet_test.yaml:64-66; both are switched on by setters: simplification by set_simplification()
            # (edge collapse on the device, not libsimplify's collapse order), refinement by set_refinement() (ONet does,
            # from generation.refinement_step)
            raise NotImplementedError("simplification is not implemented; refinement is enabled with "
                                      "Generator3D.set_refinement(steps), not by the constructor")
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
        self.refine_eps_source, self.refine_seed = 'numpy', None       # set_refinement()
        self.decimate_cells = 0         # set_decimation()
        self.simplify_faces = 0         # set_simplification()
        self.components = None          # set_components(): (keep, measure, drop_cavities)
        self.last_components = None     # {'found': [...], 'kept': [...]} of the last extract_meshes(); None when off
        self._round0_cache = _lib.ArtefactCache(64)     # made here: the worker views of one network share it

    def set_refinement(self, steps, eps_source='numpy', seed=None):
        """Refine every extracted mesh by `steps` RMSprop steps (the reference's refinement_step; 0 = off).  eps_source: where
        the steps' barycentric weights come from -- 'numpy' (np.random.dirichlet from the global stream in the reference's
        order, draw_dirichlet()) or 'device' (drawn by the GPU from `seed`: same distribution, another stream; for scenes
        whose host draw would be too large.  seed=None: taken from numpy's global stream at every call).
        'numpy' reproduces a seeded reference run with ONE scene in flight: numpy's global stream is shared by every host
        thread, so scenes refined concurrently interleave their draws.  A stage that is run again by the f16-range fallback
        starts from the stream's state at its first run (ISCNet.complete, refine_mesh): the stream is consumed once."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("refinement steps must be >= 0")
        if eps_source not in ('numpy', 'device'):
            raise ValueError("eps_source must be 'numpy' or 'device'")
        self.refinement_step, self.refine_eps_source, self.refine_seed = steps, eps_source, seed
        return self

    def set_decimation(self, cells):
        """Thin every extracted mesh by vertex clustering on a `cells`^3 grid over the generator's cube (decimate.py), between
        marching cubes and the normals / the refinement: where the reference calls simplify_mesh (generator.py:189-191).
        0 or None = off (the default).  Not the reference's algorithm: edge collapse to a face budget is set_simplification()
        (the constructor's simplify_nfaces raises)."""
        cells = int(cells or 0)
        if cells < 0:
            raise ValueError("decimation cells must be >= 0")
        self.decimate_cells = cells
        return self

    def set_components(self, keep, measure='area', drop_cavities=False):
        """Drop the floaters of every extracted mesh (components.py): keep='largest' keeps the largest connected component
        of every mesh alone, a fraction t in (0, 1] every component whose `measure` ('faces', 'area' or 'abs_volume') is at
        least t times the largest's; drop_cavities also drops inside-out inner shells.  It runs directly after marching
        cubes, BEFORE set_decimation() / set_simplification(), so their budgets go to the object; normals, refinement,
        last_buffers and the Mesh list are those of the filtered meshes, and last_components holds what was found and
        kept.  None / 0 / False = off (the default).  The reference has no such step."""
        from .components import parse_keep, parse_measure
        if keep is None or keep is False or (not isinstance(keep, str) and keep == 0):
            self.components = None
            return self
        parse_keep(keep)
        parse_measure(measure)
        self.components = (keep if isinstance(keep, str) else float(keep), measure, bool(drop_cavities))
        return self

    def set_simplification(self, n_faces):
        """Simplify every extracted mesh to at most `n_faces` faces by quadric edge collapse on the device (simplify.py),
        where the reference calls simplify_mesh (generator.py:189-191): before the normals and the refinement, and after
        set_decimation()'s clustering when both are set (cluster coarsely, then collapse to the budget).  0 or None = off
        (the default).  The reference's result class, not its collapse order; the constructor's
        simplify_nfaces still raises."""
        n_faces = int(n_faces or 0)
        if n_faces < 0:
            raise ValueError("simplification target must be >= 0 faces")
        self.simplify_faces = n_faces
        return self

    def _needs_fold(self):
        return self.with_normals or self.refinement_step > 0

    # ---- reference-shaped entry points ------------------------------------------
    def generate_mesh(self, object_features, cls_codes, return_stats=True):
        """object_features (K, c_dim) -> list of K meshes (generator.py:54-76).  with_normals: every mesh's
        vertex_normals (generator.py:173-176), all K meshes in one launch after marching cubes."""
        fold = []
        grids = self.generate_grids(object_features, cls_codes, fold_out=fold)
        return self.extract_meshes(grids, fold=fold[0] if self._needs_fold() else None)

    def generate_from_latent(self, z, c=None, device='cuda', **kwargs):
        fold = []
        grids = self._grids(z, c, fold_out=fold)
        return self.extract_meshes(grids, fold=fold[0] if self._needs_fold() else None)[0]

    def eval_points(self, p, z, c=None, device='cuda', **kwargs):
        """p (T,3) -> logits (T,) for one code (generator.py:123-143)."""
        with torch.no_grad():
            return self.model.decode(p.unsqueeze(0).to(c.device), z, c, **kwargs).logits.squeeze(0)

    # ---- batched implementation --------------------------------------------------
    def logit_threshold(self):
        return logit_threshold(self.threshold)

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
        attribute (worker_view() copies the generator per host thread).  The query lists are padded 128-point tiles
        (DESIGN.md "Ragged batches"): uniform here, per proposal and per round in _grids_mise."""
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
            tiles_per = int(ragged.blocks(total, TILE))
            pts = torch.empty(tiles_per * TILE, 3, dtype=torch.float32, device=dev)
            _lib.call("rfd_make_grid_points", dev, nx, -0.5, 0.5, float(box_size), pts.data_ptr(),
                      tiles_per * TILE)
            tile_prop, tile_src = ragged.uniform_maps(K, tiles_per, dev)
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
                tiles = ragged.padded_tiles(cnt, TILE)                       # DESIGN.md "Ragged batches"
                n_tiles = int(tiles.prefix[-1])
                tile_prop = ragged.to_int32(tiles.owner, dev)
                tile_src = None
                offsets = ragged.to_int32(tiles.slot[:-1], dev)
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
        all K proposals read it (the uniform maps of DESIGN.md "Ragged batches").  Returns (pts, lin, tile_prop,
        tile_src, K * points)."""
        def build():
            R1 = (res0 << depth) + 1
            ps = torch.empty(1, R1 ** 3, dtype=torch.uint8, device=dev)
            vs = torch.empty(1, _lib.lib().rfd_mise_vstate_elems(res0, depth), dtype=torch.uint8, device=dev)
            cnt = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.call("rfd_mise_init", dev, 1, res0, depth, ps.data_ptr(), vs.data_ptr())
            _lib.call("rfd_mise_count", dev, 1, res0, depth, ps.data_ptr(), cnt.data_ptr())
            n = int(cnt.item())
            tiles_per = int(ragged.blocks(n, TILE))
            pts = torch.zeros(tiles_per * TILE, 3, dtype=torch.float32, device=dev)
            lin = torch.full((tiles_per * TILE,), -1, dtype=torch.int32, device=dev)
            offsets = torch.zeros(1, dtype=torch.int32, device=dev)
            cursors = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call("rfd_mise_collect", dev, 1, res0, depth, ps.data_ptr(), offsets.data_ptr(),
                      cursors.data_ptr(), float(box_size), pts.data_ptr(), lin.data_ptr())
            return (pts, lin) + ragged.uniform_maps(K, tiles_per, dev) + (K * n,)
        return self._round0_cache.get((res0, depth, float(box_size), K, str(dev)), build, dev)   # per K: NMS changes it

    # ---- mesh extraction ------------------------------------------------------------
    def extract_meshes(self, grids, fold=None):
        """fold = (table, fc_p_w) of the codes the grids came from: vertex normals from the decoder's gradient
        (Generator3D.estimate_normals), one launch for all meshes; with set_refinement(), the refinement of all meshes
        (refine_meshes) -- after the normals, which belong to the unrefined vertices as in the reference (generator.py:173-195).
        With set_decimation() / set_simplification() the meshes are thinned first: normals, refinement, last_buffers and the
        Mesh list are those of the thinned meshes.  With set_components() the floaters are dropped before all of that."""
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
        self.last_components = None
        if self.components is not None:
            from .components import keep_components
            keep, measure, drop_cavities = self.components
            v, f, vend, tend, self.last_components = keep_components(v, f, vend, tend, keep=keep, measure=measure,
                                                                     drop_cavities=drop_cavities, return_info=True)
        if self.decimate_cells:
            from .decimate import decimate_meshes
            K = len(vend) - 1
            v, f, vend, tend = decimate_meshes(v, f, vend, tend, self.decimate_cells, lo=np.full((K, 3), -box_size / 2),
                                               h=np.full(K, box_size / self.decimate_cells))
        if self.simplify_faces:
            from .simplify import simplify_meshes
            v, f, vend, tend, _ = simplify_meshes(v, f, vend, tend, self.simplify_faces)
        self.last_normals = None
        refine = self.refinement_step > 0
        if refine and fold is None:
            raise ValueError("refinement needs fold = (table, fc_p_w) of the meshes' codes (DecoderCBatchNorm.fold)")
        nrm = None
        if fold is not None and (self.with_normals or not refine):
            # generator.py:173-176: normals of every non-empty mesh; the reference leaves them None on an empty one
            # (decimated vertices are f32, simplified ones f64; the normals kernel reads f64: widened, exact)
            nrm = self.last_normals = self.model.decoder.normals(v if v.dtype == torch.float64 else v.double(), vend,
                                                                 fold[0], fold[1])
        if refine:
            v = self.refine_meshes(v, f, vend, tend, fold, self.refinement_step)
        self.last_buffers = (v, f, vend, tend)
        return [Mesh(v[vend[k]:vend[k + 1]], f[tend[k]:tend[k + 1]],
                     nrm[vend[k]:vend[k + 1]] if nrm is not None and vend[k + 1] > vend[k] else None)
                for k in range(len(vend) - 1)]

    # ---- refinement (generator.py:226-289) -----------------------------------------------
    def device_weights(self, n, seed, step, device):
        """(n,3) f32 Dirichlet(1/2,1/2,1/2) rows of refinement step `step` drawn on `device` (eps_source='device')"""
        out = torch.empty(n, 3, dtype=torch.float32, device=device)
        _lib.call("rfd_refine_dirichlet", device, n, int(seed) & (2 ** 64 - 1), int(step), out.data_ptr())
        return out

    @torch.no_grad()
    def refine_meshes(self, v, f, vend, tend, fold, steps, eps=None, return_grad=False):
        """Generator3D.refine_mesh for ALL meshes of the flat marching-cubes buffers in one device loop (csrc/mesh_refine.hip):
        v (V,3) f64 / f32 vertices, f (F,3) i32 faces with indices local to their mesh, vend / tend the K + 1 vertex / face
        offsets (the tile and group maps made from them here: DESIGN.md "Ragged batches"), fold = (table, fc_p_w) of the K
        codes.  -> refined vertices (V,3) f32 (a new tensor: v is the kept v0) [, the first step's vertex gradient (V,3) f32].  eps: the weights, (steps, F, 3), instead of a draw (set_refinement's
        eps_source).  Every mesh has its own loss (its own means) and its own RMSprop state, as in the reference's per-object
        loop; empty meshes take no part.  Asynchronous, no host round trip inside the loop: the f16-range flag (STATUS_DECODER_RANGE)
        is left in the stream's status word for the caller's run_with_range_fallback, which starts again from v0."""
        dec = self.model.decoder
        if dec.mode != MODE_F16X3:
            raise NotImplementedError("mesh refinement needs the parity mode (MODE_F16X3); MODE_F16X1 is not supported")
        if dec.kernel != "w8":
            raise NotImplementedError("mesh refinement uses the eight-wave decoder's weight stream (kernel 'w8')")
        vend, tend = [int(x) for x in vend], [int(x) for x in tend]
        K, V, F = len(vend) - 1, vend[-1], tend[-1]
        assert len(tend) == K + 1 and vend[0] == 0 and tend[0] == 0 and v.is_cuda and v.shape[0] >= V and f.shape[0] >= F
        dev = v.device
        vr = v[:V].to(torch.float32, copy=True).contiguous()                     # generator.py:245-246
        grad0 = torch.zeros(V, 3, dtype=torch.float32, device=dev) if return_grad else None
        if steps > 0 and F > 0:
            table, fc_p_w = fold
            assert table.shape[0] >= K
            counts = [tend[k + 1] - tend[k] for k in range(K)]
            tiles = ragged.padded_tiles(counts, TILE)
            gprefix = ragged.offsets(ragged.blocks(counts, GROUP))
            fend_d, vend_d, tprefix_d, gprefix_d = ragged.to_int32(np.stack([tend, vend, tiles.prefix, gprefix]), dev)
            tile_prop = ragged.to_int32(tiles.owner, dev)
            faces = f[:F].to(torch.int32).contiguous()
            first = torch.repeat_interleave(vend_d[:-1].long(), torch.as_tensor(counts, device=dev), output_size=F)
            rowptr, col = mesh_batch.corner_csr(faces.long() + first[:, None], V)
            if eps is not None:
                eps = torch.as_tensor(np.ascontiguousarray(eps, dtype=np.float32)) if not torch.is_tensor(eps) else eps
                assert tuple(eps.shape) == (steps, F, 3)
                eps = eps.to(dev, torch.float32).contiguous()
            elif self.refine_eps_source == 'numpy':
                eps = torch.from_numpy(draw_dirichlet(counts, steps)).to(dev)
            else:
                seed = self.refine_seed if self.refine_seed is not None else int(np.random.randint(0, 2 ** 31 - 1))
            qd = torch.empty(F, 3, dtype=torch.float64, device=dev)
            qt = torch.zeros(int(tiles.slot[-1]), 3, dtype=torch.float32, device=dev)     # padding slots stay zero
            cg = torch.empty(F, 3, 3, dtype=torch.float64, device=dev)     # f64: csrc/mesh_refine.hip's header says why
            sq = torch.zeros(V, 3, dtype=torch.float32, device=dev)
            g = torch.empty(F, 3, dtype=torch.float32, device=dev)
            nrm = torch.empty(F, 3, dtype=torch.float32, device=dev)                          # the normals kernel's other output
            input_grad = dec.input_grad_launcher(table, fc_p_w, K, int(gprefix[-1]), fend_d, gprefix_d)
            tau = float(self.threshold)
            for it in range(steps):
                e = eps[it] if eps is not None else self.device_weights(F, seed, it, dev)
                _lib.call("rfd_refine_sample", dev, F, K, vr.data_ptr(), faces.data_ptr(), fend_d.data_ptr(),
                          vend_d.data_ptr(), tprefix_d.data_ptr(), e.data_ptr(), qd.data_ptr(), qt.data_ptr())
                logits = dec.decode_tiles(qt, tile_prop, table, fc_p_w)
                input_grad(qd, nrm, g)
                _lib.call("rfd_refine_face_backward", dev, F, K, vr.data_ptr(), faces.data_ptr(), fend_d.data_ptr(),
                          vend_d.data_ptr(), tprefix_d.data_ptr(), e.data_ptr(), logits.data_ptr(), g.data_ptr(), tau,
                          cg.data_ptr())
                _lib.call("rfd_refine_vertex_step", dev, V, rowptr.data_ptr(), col.data_ptr(), 3 * F, cg.data_ptr(),
                          vr.data_ptr(), sq.data_ptr(), grad0.data_ptr() if return_grad and it == 0 else None)
        return (vr, grad0) if return_grad else vr

    def refine_mesh(self, mesh, occ_hat, z, c=None, device='cuda'):
        """generator.py:226-289: moves mesh.vertices (numpy or tensor (V,3); mesh.faces (F,3)) by self.refinement_step steps
        for one code z (Z,), c (C,); occ_hat is not used (the reference only reads its shape).  -> mesh"""
        dec = self.model.decoder
        if c is None:
            raise ValueError("refinement needs the code c (the decoder is conditioned on it)")
        dev = c.device if c.is_cuda else torch.device(device)
        as_numpy = not torch.is_tensor(mesh.vertices)
        v = torch.as_tensor(np.ascontiguousarray(mesh.vertices) if as_numpy else mesh.vertices).to(dev)
        f = torch.as_tensor(np.ascontiguousarray(mesh.faces) if not torch.is_tensor(mesh.faces) else mesh.faces)
        f = f.to(dev, torch.int32).reshape(-1, 3)
        if v.shape[0] == 0 or not self.refinement_step:
            return mesh
        with torch.no_grad():
            z, c = z.reshape(1, -1).float().to(dev), c.reshape(1, -1).float().to(dev)
            # the numpy stream must not be drawn from twice when the range fallback runs the loop again
            eps = None
            if self.refine_eps_source == 'numpy':
                eps = draw_dirichlet([f.shape[0]], self.refinement_step)
            out = run_with_range_fallback(dec, lambda: self.refine_meshes(
                v, f, [0, v.shape[0]], [0, f.shape[0]], dec.fold(z, c), self.refinement_step, eps=eps), dev)
        mesh.vertices = out.cpu().numpy() if as_numpy else out
        return mesh

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
        fold = None
        if self.refinement_step > 0:                                 # generator.py:194-195
            if c is None:
                raise ValueError("refinement needs the code c (the decoder is conditioned on it)")
            with torch.no_grad():
                fold = self.model.decoder.fold(z.reshape(1, -1).float().to(g.device), c.reshape(1, -1).float().to(g.device))
        return self.extract_meshes(g.unsqueeze(0), fold=fold)[0]
