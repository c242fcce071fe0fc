"""DecoderCBatchNorm with the reference's constructor, forward signature and
state_dict keys (models/iscnet/modules/occ_decoder.py:72-123, layers.py:51-107,
193-242), evaluated by ONE fused HIP kernel: csrc/occ_decoder8.hip by default
(launches of few tiles: csrc/occ_decoder_tail.hip; csrc/occ_decoder.hip, the
four-wave kernel, is kept as the independent cross-check).

state_dict keys (verified against the reference class by
tests/golden/make_fixtures.py):  fc_p.{weight(256,3,1),bias}, fc_z.{weight
(256,Z),bias}, blocks.{0-4}.{bn_0,bn_1}.{conv_gamma,conv_beta}.{weight
(256,C,1),bias}, blocks.{i}.{bn_0,bn_1}.bn.{running_mean,running_var,
num_batches_tracked}, blocks.{i}.{fc_0,fc_1}.{weight(256,256,1),bias}, bn.*,
fc_out.{weight(1,256,1),bias}.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, occ_fold, ragged

MODE_F16X3 = 3   # parity mode (fp32-class logits)
MODE_F16X1 = 1   # throughput mode
TILE = 128       # RFD_OCC_TILE: query points of a decoder tile (include/rfd_occ.h)
GROUP = 16       # vertices of a group of rfd_occ_normals_w8's `gprefix` (include/rfd_occ.h)


def logit_threshold(threshold):
    """probs >= threshold as a comparison of logits (generator.py:85)"""
    return float(np.log(threshold) - np.log(1. - threshold))


def run_with_range_fallback(dec, run, device, before=None):
    """out = run() (the fold and the launches) with the stream's status read that must follow it.  An activation beyond
    the f16 range (_lib.STATUS_DECODER_RANGE) does not fail the call: run() is called once more when the decoder's scale has come
    down since the first run began -- by this call (dec.lower_activation_scale()), or by another host thread sharing
    the decoder (its run was folded at the OLD scale).  Only a flag raised at the fallback scale is a real overflow.
    before(): called after the status read and before the scale is looked at -- it raises for the flags of earlier
    stages, which must not lower the decoder's scale."""
    ka_used = dec.ka
    out = run()
    with torch.cuda.device(device):
        st = _lib.stream_status_bits()
    if before is not None:
        before()
    if st & _lib.STATUS_DECODER_RANGE:
        with _lib.BUILD_LOCK:
            lowered = dec.lower_activation_scale()
        if lowered or dec.ka < ka_used:
            out = run()
            with torch.cuda.device(device):
                st = (st & ~_lib.STATUS_DECODER_RANGE) | _lib.stream_status_bits()
    _lib.raise_status(st)
    return out


class CBatchNorm1d(nn.Module):
    """Parameter container of layers.py:193-242 (conv_gamma, conv_beta, bn)."""

    def __init__(self, c_dim, f_dim, norm_method='batch_norm'):
        super().__init__()
        if norm_method != 'batch_norm':
            raise NotImplementedError("only batch_norm is on the inference path")
        self.c_dim = c_dim
        self.f_dim = f_dim
        self.norm_method = norm_method
        self.conv_gamma = nn.Conv1d(c_dim, f_dim, 1)
        self.conv_beta = nn.Conv1d(c_dim, f_dim, 1)
        self.bn = nn.BatchNorm1d(f_dim, affine=False)
        self.reset_parameters()

    def reset_parameters(self):            # layers.py:219-224
        nn.init.zeros_(self.conv_gamma.weight)
        nn.init.zeros_(self.conv_beta.weight)
        nn.init.ones_(self.conv_gamma.bias)
        nn.init.zeros_(self.conv_beta.bias)


class CResnetBlockConv1d(nn.Module):
    """Parameter container of layers.py:51-107 (size_in == size_h == size_out)."""

    def __init__(self, c_dim, size_in, size_h=None, size_out=None,
                 norm_method='batch_norm', legacy=False):
        super().__init__()
        if legacy:
            raise NotImplementedError("legacy CBN is not on the inference path")
        size_h = size_in if size_h is None else size_h
        size_out = size_in if size_out is None else size_out
        if not (size_in == size_h == size_out):
            raise NotImplementedError("shortcut blocks are not used by DecoderCBatchNorm")
        self.size_in, self.size_h, self.size_out = size_in, size_h, size_out
        self.bn_0 = CBatchNorm1d(c_dim, size_in, norm_method=norm_method)
        self.bn_1 = CBatchNorm1d(c_dim, size_h, norm_method=norm_method)
        self.fc_0 = nn.Conv1d(size_in, size_h, 1)
        self.fc_1 = nn.Conv1d(size_h, size_out, 1)
        self.shortcut = None
        nn.init.zeros_(self.fc_1.weight)   # layers.py:96


class DecoderCBatchNorm(nn.Module):
    def __init__(self, dim=3, z_dim=128, c_dim=128, hidden_size=256, n_blocks=5,
                 leaky=False, legacy=False):
        super().__init__()
        if dim != 3 or hidden_size != 256 or n_blocks != 5 or leaky or legacy:
            raise NotImplementedError(
                "the fused HIP decoder is built for dim=3, hidden_size=256, "
                "n_blocks=5, ReLU (the configuration RfD-Net instantiates, "
                "occupancy_net.py:45)")
        self.z_dim = z_dim
        if not z_dim == 0:
            self.fc_z = nn.Linear(z_dim, hidden_size)
        self.fc_p = nn.Conv1d(dim, hidden_size, 1)
        self.blocks = nn.ModuleList([CResnetBlockConv1d(c_dim, hidden_size)
                                     for _ in range(n_blocks)])
        self.bn = CBatchNorm1d(c_dim, hidden_size)
        self.fc_out = nn.Conv1d(hidden_size, 1, 1)
        self.mode = MODE_F16X3
        # which kernel: 'w4' = four 496-register waves per workgroup (csrc/occ_decoder.hip),
        # 'w8' = eight waves, two per SIMD (csrc/occ_decoder8.hip); same results
        self.kernel = os.environ.get("RFD_DECODER_KERNEL", "w8")
        # activation scale 2^ka of the split-f16 arithmetic (occ_fold.py): lowered ONCE, for good, by
        # lower_activation_scale() when a launch reports an activation beyond the f16 range at the current scale --
        # the reference's fp32 decoder (occ_decoder.py:110-123) cannot overflow, so neither may this one fail a scene
        self.ka = occ_fold.KA
        self.check_range = True        # forward() reads the stream's status word after the launch

    # ---- weight stream (re-packed only when the parameters change) -----------
    def packed_weights(self):
        """The decoder kernels' weight stream: -> (packed, kw0, kw1)."""
        return self._packed_stream('_packed', bwd=False)

    def packed_weights_bwd(self):
        """The weight stream of the normals kernel's backward pass (csrc/occ_normals.hip): rfd_occ_pack_weights_w8 of
        fc0' = blocks[4-j].fc_1.weight^T and fc1' = blocks[4-j].fc_0.weight^T.  Cached under packed_weights()'s key.
        Returns (packed, kb0, kb1)."""
        return self._packed_stream('_packed_bwd', bwd=True)

    def _packed_stream(self, slot, bwd):
        key = _lib.tensor_key(*(getattr(b, fc).weight for fc in ("fc_0", "fc_1") for b in self.blocks)) + (self.kernel,)

        def build():
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            fc0, fc1 = occ_fold.stacked_fc_weights(sd)
            _lib.need_gpu(fc0)
            if bwd:
                fc0, fc1 = (fc1.flip(0).transpose(1, 2).contiguous(),      # W1^T of blocks 4 .. 0
                            fc0.flip(0).transpose(1, 2).contiguous())      # W0^T of blocks 4 .. 0
            k0 = [occ_fold.choose_kw([fc0[i]]) for i in range(5)]
            k1 = occ_fold.choose_kw([fc1])
            packed = torch.empty(_lib.lib().rfd_occ_packed_bytes(), dtype=torch.uint8, device=fc0.device)
            name = "rfd_occ_pack_weights_w8" if bwd or self.kernel == "w8" else "rfd_occ_pack_weights"
            _lib.call(name, fc0.device, fc0.data_ptr(), fc1.data_ptr(), (C.c_int * 5)(*k0), k1, packed.data_ptr())
            return packed, k0, k1
        return _lib.build_once(self.__dict__, slot, key, build, self.blocks[0].fc_0.weight.device)

    def normals(self, verts, vend, table, fc_p_w, return_grad=False):
        """Vertex normals -g / |g|, g = d logit / d p, of K meshes in one launch (csrc/occ_normals.hip;
        Generator3D.estimate_normals, generator.py:200-224).
        verts (V,3) f64 device tensor (all meshes back to back), vend: K + 1 vertex offsets (list or sequence; the group
        prefix they imply: DESIGN.md "Ragged batches"), table /
        fc_p_w: the fold of the meshes' codes (fold()).  -> normals (V,3) f32 [, grad (V,3) f32].  A vertex whose gradient
        is exactly zero gets NaN (0/0, as in the reference).  Asynchronous: the f16-range flag (STATUS_DECODER_RANGE) is left in
        the stream's status word for the caller to read, like decode_tiles()."""
        if self.mode != MODE_F16X3:
            raise NotImplementedError("vertex normals need the parity mode (MODE_F16X3); MODE_F16X1 is not supported")
        if self.kernel != "w8":
            raise NotImplementedError("vertex normals use the eight-wave decoder's weight stream (kernel 'w8')")
        assert verts.is_cuda and verts.dtype == torch.float64 and verts.is_contiguous() and verts.dim() == 2
        assert table.is_contiguous() and table.dtype == torch.float32 and fc_p_w.is_contiguous()
        vend = [int(x) for x in vend]
        K = len(vend) - 1
        assert K >= 1 and vend[0] == 0 and vend[-1] <= verts.shape[0] and table.shape[0] >= K
        gprefix = ragged.offsets(ragged.blocks(np.diff(vend), GROUP))
        V = vend[-1]
        dev = verts.device
        normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
        grad = torch.empty(V, 3, dtype=torch.float32, device=dev) if return_grad else None
        if gprefix[-1]:
            vend_d, gprefix_d = ragged.to_int32(np.stack([vend, gprefix]), dev, non_blocking=True)
            self.input_grad_launcher(table, fc_p_w, K, int(gprefix[-1]), vend_d, gprefix_d)(verts, normals, grad)
        return (normals, grad) if return_grad else normals

    def input_grad_launcher(self, table, fc_p_w, K, n_groups, vend, gprefix):
        """-> launch(verts (V,3) f64, normals (V,3) f32 out, grad (V,3) f32 out or None): rfd_occ_normals_w8 for K meshes
        whose vertex / 16-group offsets are the DEVICE int32 tensors vend / gprefix (K + 1 each, n_groups = the last group
        offset).  For callers that launch many times on the same offsets (the refinement loop): nothing is uploaded per
        launch."""
        packed, kw0, kw1 = self.packed_weights()
        packed_b, kb0, kb1 = self.packed_weights_bwd()
        wo = self.fc_out.weight.detach().reshape(-1).contiguous()
        kw = (C.c_int * 12)(*(list(kw0) + [kw1] + list(kb0) + [kb1]))
        assert vend.dtype == torch.int32 and gprefix.dtype == torch.int32 and vend.is_cuda and gprefix.is_cuda

        def launch(verts, normals, grad):
            assert verts.dtype == torch.float64 and verts.is_contiguous() and normals.dtype == torch.float32
            _lib.call("rfd_occ_normals_w8", verts.device, n_groups, verts.data_ptr(), vend.data_ptr(), gprefix.data_ptr(),
                      K, packed.data_ptr(), packed_b.data_ptr(), kw, fc_p_w.data_ptr(), table.data_ptr(), wo.data_ptr(),
                      normals.data_ptr(), _lib.ptr(grad), self.mode)
        return launch

    def input_grad(self, p, z, c):
        """d logit / d p of forward(p, z, c) (p (B,T,3)) -> (B,T,3) f32, with the f16-range flag answered like forward()'s."""
        B, T, _ = p.shape
        if c.dim() == 3:
            c = c.squeeze(2)
        verts = p.detach().reshape(-1, 3).double().contiguous()
        vend = [b * T for b in range(B + 1)]

        def run():
            table, fc_p_w = self.fold(z.detach().float(), c.detach().float())
            return self.normals(verts, vend, table, fc_p_w, return_grad=True)[1]
        grad = run_with_range_fallback(self, run, p.device) if self.check_range else run()
        return grad.view(B, T, 3)

    def _fc_out_bias(self):
        b = self.fc_out.bias
        return _lib.build_once(self.__dict__, '_fc_out_b', _lib.tensor_key(b), lambda: float(b.detach().item()),
                               b.device)                       # one sync per weight load

    def fold(self, z, c):
        """Per-proposal table (K,23,256) + scaled fc_p weight for codes z, c."""
        _, kw0, kw1 = self.packed_weights()
        if self.training:                  # parameters may move under us: fold from the live tensors
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            if self.z_dim == 0:
                sd["fc_z.weight"] = torch.zeros(256, 0, device=c.device)
                sd["fc_z.bias"] = torch.zeros(256, device=c.device)
            return occ_fold.fold_table(sd, z, c, kw0, kw1, ka=self.ka)
        ka = self.ka
        key = _lib.tensor_key(*self.parameters(), *self.buffers()) + (ka,)

        def build():
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            return occ_fold.stacked_constants(sd, kw0, kw1, ka=ka)
        return occ_fold.fold_table_stacked(_lib.build_once(self.__dict__, '_fold_cache', key, build, c.device), z, c)

    def lower_activation_scale(self):
        """After STATUS_DECODER_RANGE (an activation * 2^ka reached the f16 limit): switch to the fallback scale, once.
        Returns True if the caller should run the launch again, False if the fallback scale is already in use
        (then the overflow is real: |activation| >= 8190)."""
        if self.ka <= occ_fold.KA_FALLBACK:
            return False
        import warnings
        warnings.warn("occupancy decoder: an activation exceeded the f16 range at scale 2^%d; re-running at 2^%d "
                      "(kept for this decoder from now on)" % (self.ka, occ_fold.KA_FALLBACK), RuntimeWarning)
        self.ka = occ_fold.KA_FALLBACK
        return True

    def can_scatter(self):
        """the eight-wave kernel can write MISE's value / known arrays itself (decode_tiles(scatter=...))"""
        return self.kernel == "w8" and getattr(self, "fuse_scatter", True)

    def decode_tiles(self, pts, tile_prop, table, fc_p_w, mode=None, tile_src=None, scatter=None):
        """pts (n_src_tiles*128,3) f32, tile_prop (n_tiles,) i32 [, tile_src
        (n_tiles,) i32: which source tile each tile reads] -> logits (n_tiles*128,).
        scatter = (lin i32 indexed like pts, values (K,n_per) f32, pstate (K,n_per) u8): the logits go
        straight to values[prop, lin] and the points are marked known (returns None)."""
        packed, _, _ = self.packed_weights()
        n_tiles = tile_prop.shape[0]
        assert pts.is_contiguous() and pts.dtype == torch.float32
        assert tile_src is not None or pts.shape[0] == n_tiles * TILE
        assert tile_prop.dtype == torch.int32 and table.is_contiguous()
        wo = self.fc_out.weight.detach().reshape(-1).contiguous()
        bo = self._fc_out_bias()
        if scatter is not None:
            lin, values, pstate = scatter
            assert self.can_scatter() and lin.dtype == torch.int32 and lin.shape[0] == pts.shape[0]
            assert values.dtype == torch.float32 and pstate.dtype == torch.uint8 and values.is_contiguous()
            _lib.call("rfd_occ_decode_scatter_w8", pts.device, n_tiles, pts.data_ptr(), tile_prop.data_ptr(),
                      _lib.ptr(tile_src), packed.data_ptr(), fc_p_w.data_ptr(), table.data_ptr(), wo.data_ptr(), bo,
                      lin.data_ptr(), values.data_ptr(), pstate.data_ptr(), int(values.shape[1]),
                      self.mode if mode is None else mode)
            return None
        logits = torch.empty(n_tiles * TILE, dtype=torch.float32, device=pts.device)
        _lib.call("rfd_occ_decode_w8" if self.kernel == "w8" else "rfd_occ_decode", pts.device, n_tiles, pts.data_ptr(),
                  tile_prop.data_ptr(), _lib.ptr(tile_src), packed.data_ptr(), fc_p_w.data_ptr(), table.data_ptr(),
                  wo.data_ptr(), bo, logits.data_ptr(), self.mode if mode is None else mode)
        return logits

    def forward(self, p, z, c, **kwargs):
        """p (B,T,3), z (B,Z), c (B,C) -> logits (B,T).  occ_decoder.py:110-123.  B uniform segments of padded tiles
        (DESIGN.md "Ragged batches").

        Gradients: when p requires grad (and grad mode is on) the logits carry a grad_fn whose backward gives
        dL/dp = dL/dlogit * d logit / d p through the normals kernel (csrc/occ_normals.hip) -- what the reference's
        Generator3D.estimate_normals needs (vi.requires_grad_(); decode(vi).logits.sum().backward(); -vi.grad).  That is
        the ONLY gradient this module has: none for z, c (an error if either requires grad) and none for the parameters."""
        _lib.need_gpu(p)
        if torch.is_grad_enabled() and p.requires_grad:
            if z.requires_grad or c.requires_grad:
                raise NotImplementedError("DecoderCBatchNorm: only the gradient with respect to the query points p is "
                                          "implemented (not z or c)")
            return _DecodeWithInputGrad.apply(p, z, c, self)
        B, T, _ = p.shape
        if c.dim() == 3:
            c = c.squeeze(2)
        tiles_per = int(ragged.blocks(T, TILE))
        tpad = tiles_per * TILE
        if tpad != T:
            pp = torch.zeros(B, tpad, 3, dtype=torch.float32, device=p.device)
            pp[:, :T] = p
        else:
            pp = p.contiguous().float()
        tile_prop, _ = ragged.uniform_maps(B, tiles_per, p.device, src=False)

        def run():
            table, fc_p_w = self.fold(z.float(), c.float())
            return self.decode_tiles(pp.reshape(-1, 3), tile_prop, table, fc_p_w)
        # the module's own forward is synchronous about the f16-range flag (one 4-byte read on this stream): an
        # overflow at the default scale is answered by the fallback scale, not by an exception
        logits = run_with_range_fallback(self, run, p.device) if self.check_range else run()
        return logits.view(B, tpad)[:, :T]


class _DecodeWithInputGrad(torch.autograd.Function):
    """logits = decoder(p, z, c) with backward dL/dp = dL/dlogits * d logit / d p (normals kernel); no other gradient."""

    @staticmethod
    def forward(ctx, p, z, c, dec):
        ctx.dec = dec
        ctx.save_for_backward(p, z, c)
        with torch.no_grad():
            return dec(p.detach(), z.detach(), c.detach())

    @staticmethod
    def backward(ctx, grad_out):
        p, z, c = ctx.saved_tensors
        g = ctx.dec.input_grad(p, z, c)
        return (grad_out.to(g.dtype).unsqueeze(-1) * g).to(p.dtype), None, None, None
