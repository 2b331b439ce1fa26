"""
Frozen ExtendedDINOSAUR decoder for the image-loss term of the predictor training step: forward of
ExtendedDINOSAUR.decode = MLPPatchDecoder.forward + its CNN image head (reference decoders.py:264-365) that keeps the
activations of one chunk of frames, the per-pixel MSE gradient, and the hand-written backward w.r.t. the slots (the
decoder's weights are frozen, 04_train_predictor.py:62-75; BatchNorm runs in eval mode, base/basePredictorTrainer.py:
139-141).  Chunk-local like DecoderLoss: the loss is a sum over frames, so every chunk is decoded, differentiated and
dropped before the next one.

  slots --broadcast + pos, LayerNorm--> MLP (3 x Linear+ReLU, head) --> softmax_K(alpha) / weighted feature sum
        --> [Conv3x3 + BN + ReLU (+ nearest x2)] x 4 --> (x2) Conv3x3 -> RGB --> bilinear resize --> sum (img - target)^2

Backward, all on HIP kernels:
  bilinear adjoint (gather form, NCHW -> NHWC)                          tocvp_bilinear_resize_bwd_f32
  conv data gradients, ReLU gate of the block below in the store:       tocvp_conv3x3_dgrad_bf16x3_f32
    behind an upsampling: the adjoint of the four-phase conv (16 taps per input pixel, low resolution written directly),
    block 0 a plain 3x3 data gradient; eval BatchNorm scale folded into the transposed weights
  composite adjoint into the zero-padded head layout                    tocvp_slot_composite_bwd_f32
  head + hidden Linear data gradients (ReLU gate in the GEMM epilogue)  linear(..., ACT_GATE), bf16x3
  LayerNorm backward summed over the patches per slot                   tocvp_ln_bcast_bwd_f32
Every backward product runs on bf16x3 split operands: fp32-class per product with the fp32 exponent range, so the
~2 / numel incoming gradient needs no operand scale.  The backward weights live in the decoder's Derived cache like its
forward weights: they follow load_state_dict, .to() and in-place updates.

Default chunk (TOCVP_PATCH_DEC_CHUNK_MB, KNOBS.md): as many frames as fit in that many MiB of chunk activations, counted
per frame as 4 bytes x [K N (2 D + 5 hidden + 2 ld)  (LayerNorm in/out, three hidden activations + two gradient
buffers, head output + its gradient, ld = 832) + 2 x every image-head activation (value + gradient) + 3 x the image].
"""

import os

import torch

from .. import kernels as K
from . import autograd as ag

__all__ = ["PatchDecoderLoss"]

_L = K.lib
_CHUNK_MB = int(os.environ.get("TOCVP_PATCH_DEC_CHUNK_MB", "4096"))
# head width (F + 1 = 769) zero-padded to 832: a multiple of 64 is what the fragment-order split GEMM of the head's data
# gradient needs (and the only one of the split GEMMs that applies the ReLU gate of the layer below in its epilogue)
_HEAD_MULT = 64

# tap r of the up2 data gradient (high-resolution row 2 y + r - 1) sums the 3x3 rows {2 - r, 3 - r} & [0, 2]
_UP2_ROWS = ((2,), (1, 2), (0, 1), (0,))


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dgrad_weights(w, scale, up2):
    """ (Cout, Cin, 3, 3) forward weights (x BatchNorm scale per Cout) -> (9 or 16 taps, Cin, Cout) data-gradient weights """
    w = w.detach().double()
    if scale is not None:
        w = w * scale.detach().double()[:, None, None, None]
    if not up2:
        return w.flip(-1, -2).permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).float().contiguous()
    m = torch.zeros((4, 3), dtype=torch.float64, device=w.device)
    for r, rows in enumerate(_UP2_ROWS):
        m[r, list(rows)] = 1.0
    wd = torch.einsum("ra,sb,oiab->rsio", m, m, w)
    return wd.reshape(16, w.shape[1], w.shape[0]).float().contiguous()


class PatchDecoderLoss:
    def __init__(self, model, frames_per_chunk=None):
        dec = model.decoder
        if type(dec).__name__ != "MLPPatchDecoder" or not dec.initial_layer_norm or not dec.reconstruct_images:
            raise NotImplementedError("training step: MLPPatchDecoder with initial_layer_norm and the CNN image head")
        self.model, self.dec = model, dec
        self.frames_per_chunk = frames_per_chunk

    # ---- derived backward weights (decoder's Derived cache) ----------------------------------------------------
    def _blocks(self):
        from ..models.Blocks.model_blocks import ConvBlock
        return [m for m in self.dec.conv_patch_decoder if isinstance(m, ConvBlock)]

    def _block_dgrad(self, i, blk, up2):
        conv = blk.conv
        srcs = [conv.weight] + [t for t in blk.block[1].state_dict().values() if t.is_floating_point()]
        return self.dec._derived.get(("bwd_dgrad", i, up2), srcs,
                                     lambda: _dgrad_weights(conv.weight, blk.folded_scale_shift()[0], up2))

    def _final_dgrad(self, up2):
        final = self.dec.conv_patch_decoder[-1]

        def build():
            w = torch.zeros((32,) + tuple(final.weight.shape[1:]), device=final.weight.device)
            w[:3] = final.weight.detach()
            return _dgrad_weights(w, None, up2)
        return self.dec._derived.get(("bwd_final", up2), [final.weight], build)

    def _linear_t(self, j, lin):
        """ W^T of hidden Linear j: the weight operand of its data gradient g W """
        return self.dec._derived.get(("bwd_lin_t", j), [lin.weight], lambda: lin.weight.detach().t().contiguous())

    def _head(self, head):
        from ..models.EncodersDecoders.decoders import _pad_rows32
        return self.dec._derived.get(("head_pad", _HEAD_MULT), [head.weight, head.bias],
                                     lambda: _pad_rows32(head.weight, head.bias, _HEAD_MULT))

    def _head_t(self, head):
        return self.dec._derived.get(("bwd_head_t", _HEAD_MULT), [head.weight],
                                     lambda: self._head(head)[0].t().contiguous())

    # ---- chunking ------------------------------------------------------------------------------------------------
    def _frame_bytes(self, Ks):
        dec = self.dec
        N, D, hid = dec.num_patches, dec.in_dim, dec.hidden_dim
        ld = (dec.out_dim + _HEAD_MULT - 1) // _HEAD_MULT * _HEAD_MULT
        mlp = Ks * N * (2 * D + 5 * hid + 2 * ld)
        size, cnn = dec.patch_grid[0], 0
        for blk, up in zip(self._blocks(), dec._upsample_after):
            cnn += 2 * size * size * blk.conv.weight.shape[0]
            size = size * 2 if up else size
        cnn += 2 * size * size * 32 + 3 * 3 * dec.image_size ** 2
        return 4 * (mlp + cnn)

    def chunk_frames(self, Ks):
        return self.frames_per_chunk or max(1, (_CHUNK_MB << 20) // self._frame_bytes(Ks))

    # ---- forward + backward ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def loss_and_slot_grad(self, slots, targets, grad_scale):
        """
        slots (F, K, D) fp32, targets (F, 3, S, S).  Returns (sum of squared pixel errors as a (1,) tensor,
        dslots (F, K, D) = the gradient of grad_scale/2 * sum (img - target)^2; pass grad_scale = 2 * weight / numel
        for weight * MSE), as DecoderLoss.loss_and_slot_grad.
        """
        dec = self.dec
        F_, Ks, D = slots.shape
        N, Fd = dec.num_patches, dec.out_dim - 1
        ln = dec.mlp[0]
        linears = [m for m in dec.mlp[1:] if isinstance(m, torch.nn.Linear)]
        head = linears[-1]
        pos = dec.pos_embed.detach().reshape(N, D)
        if not pos.is_contiguous():
            pos = pos.contiguous()
        blocks = self._blocks()
        ups = dec._upsample_after
        fpc = self.chunk_frames(Ks)
        dslots = torch.empty_like(slots)
        sq = torch.zeros(1, device=slots.device, dtype=torch.float32)
        for f0 in range(0, F_, fpc):
            f1 = min(F_, f0 + fpc)
            nf = f1 - f0
            n = nf * Ks
            sl = slots[f0:f1].reshape(n, D).contiguous()
            # forward (MLPPatchDecoder.forward with fp32 hand-overs between the layers), hidden activations kept
            with K.gemm_precision(dec.mlp_precision, owner=(dec, "mlp_precision")):
                x = sl.reshape(n, 1, D).expand(n, N, D).contiguous()
                x = K.layer_norm(x, ln.weight, ln.bias, ln.eps, add=pos)
                hs = []
                for lin in linears[:-1]:
                    x = K.linear(x, lin.weight, lin.bias, act=K.ACT_RELU)
                    hs.append(x)
                wpad, bpad = self._head(head)
                y = K.linear(x, wpad, bpad)                                   # (n, N, ld)
            ld = wpad.shape[0]
            y = y.reshape(nf, Ks, N, ld)
            recons, masks = K.slot_composite(y, feat_dim=Fd)
            acts = []
            imgs = dec._render(recons, keep=acts)                             # acts: block outputs, final conv output
            # per-pixel loss gradient: dimg = grad_scale * (img - target)
            tgt = targets[f0:f1].contiguous()
            nel = imgs.numel()
            nblocks = min(1024, (nel + 255) // 256)
            part = torch.empty(nblocks, device=slots.device, dtype=torch.float32)
            dimg = torch.empty_like(imgs)
            K._check(_L().tocvp_mse_f32(imgs.data_ptr(), tgt.data_ptr(), part.data_ptr(), nblocks,
                                        dimg.data_ptr(), nel, float(grad_scale), _s()), "tocvp_mse_f32")
            ag.axpby(ag.colsum(part.reshape(nblocks, 1)), sq, 1.0, 1.0)
            # image head backward: resize adjoint, final conv, blocks last to first (gate = the block below's output)
            fin = acts.pop()
            g = K.bilinear_resize_bwd(dimg, fin.shape[1:3], fin.shape[3])
            del dimg, imgs, fin
            a = acts[-1]
            g = K.conv3x3_dgrad(g, self._final_dgrad(ups[-1]), a.shape[1:3], gate=a, up2=ups[-1])
            for i in range(len(blocks) - 1, -1, -1):
                up2 = i > 0 and ups[i - 1]
                below = acts[i - 1] if i > 0 else None
                hw = below.shape[1:3] if below is not None else dec.patch_grid
                g = K.conv3x3_dgrad(g, self._block_dgrad(i, blocks[i], up2), hw, gate=below, up2=up2)
                acts.pop()
            # composite adjoint, then the MLP data gradients (ReLU gates in the GEMM epilogues), LayerNorm + broadcast
            dy = K.slot_composite_bwd(g.reshape(nf, N, Fd), y, masks, Fd)
            del g, y, recons, masks
            dh = K.linear(dy.reshape(n * N, ld), self._head_t(head), residual=hs[-1].reshape(n * N, -1),
                          act=K.ACT_GATE, precision="bf16x3")
            del dy
            for j in range(len(linears) - 2, 0, -1):
                dh = K.linear(dh, self._linear_t(j, linears[j]), residual=hs[j - 1].reshape(n * N, -1),
                              act=K.ACT_GATE, precision="bf16x3")
            del hs
            dln = K.linear(dh, self._linear_t(0, linears[0]), precision="bf16x3")        # (n N, D)
            dslots[f0:f1] = K.ln_bcast_bwd(sl, pos, ln.weight, dln, ln.eps).reshape(nf, Ks, D)
        return sq, dslots
