"""
Frozen SAVi decoder on the generic ConvDecoder path -- the variants of the reference factory: kernel 3 / 7, ``upsample: 2``,
eval ``batch_norm``, widths 32 / 64 / 128 (decoders.py:85-120) -- for the image-loss term of the predictor training step.
The forward of one chunk of frames recomputes ConvDecoder._decode_generic with the same kernel calls (so the images are
bit-identical to SAVi.decode) and keeps every hidden activation; the backward w.r.t. the slots is hand-written, the
decoder's weights are frozen (04_train_predictor.py:62-75).  Chunk-local like DecoderLoss.

  slots --(tap-sum GEMM)--> S --relu((cpos + S[cls]) sc_0 + sh_0)--> y_0
        --> [nearest x2 ->] conv_k, relu(. sc_j + sh_j) --> y_j  (j = 1 .. L - 1)
        --> 3x3 tail --> softmax over slots / compositing --> img --> sum (img - target)^2

Backward, all on HIP kernels (csrc/convk_bwd.hip, train.hip):
  compositing / softmax adjoint                                      tocvp_dec_tail_grad_f32
  tail conv 4 -> C, ReLU gate of y_{L-1}                             tocvp_conv3x3_t4w_f32
  block j >= 1: g_{j-1} = [y_{j-1} > 0] conv_k^T(g_j sc_j), with x2  tocvp_convk_dgrad_bf16x3_f32
    upsampling the stride-2 (k+1)^2-tap adjoint of the phase convs     (block 1 ungated: layer 0's gate is applied below)
  layer 0 collapsed over the k x k border classes                    tocvp_dec_class_reduce_k_f32, then dS @ tapsum
The data-gradient weights (transposed and flipped, or phase-summed, BatchNorm scale folded) live in the decoder's Derived
cache with the dependencies of ConvDecoder._block_params, so they follow load_state_dict, .to() and in-place updates.
"""

import torch

from .. import kernels as K
from . import autograd as ag

__all__ = ["GenericDecoderLoss"]

_L = K.lib


def _s():
    return torch.cuda.current_stream().cuda_stream


class GenericDecoderLoss:
    def __init__(self, savi, frames_per_chunk=None):
        dec = savi.decoder
        if type(dec).__name__ != "ConvDecoder" or not getattr(dec, "generic", False):
            raise NotImplementedError("GenericDecoderLoss: a ConvDecoder on the generic path (kernel 3 / 7, upsample 2, "
                                      "batch_norm or widths other than the shipped ones); the shipped one is DecoderLoss")
        self.savi, self.dec = savi, dec
        self.frames_per_chunk = frames_per_chunk

    def _dgrad_weights(self, j):
        """ bf16 planes of the data-gradient weights of hidden block j >= 1 (kernels.pack_convk_dgrad_weights) """
        dec = self.dec
        blk, deps = dec._block_params(j)
        return dec._derived.get(("bwd_convk", j), deps,
                                lambda: K.pack_convk_dgrad_weights(blk.conv.weight, blk.folded_scale_shift()[0],
                                                                   up2=bool(dec.upsample)))

    def chunk_frames(self, Ks):
        return self.frames_per_chunk or max(1, self.dec.max_slot_images // Ks)

    @torch.no_grad()
    def loss_and_slot_grad(self, slots, targets, grad_scale):
        """
        slots (F, K, D) fp32, targets (F, 3, H, W) at the decoder's output size.  Returns (sum of squared pixel errors as
        a (1,) tensor, dslots (F, K, D) = the gradient of grad_scale/2 * sum (img - target)^2), as
        DecoderLoss.loss_and_slot_grad.  The forward runs under the decoder's range owner: a saturating f16x3 operand
        raises kernels.TocvpRangeError naming ``generic_precision`` (its fallback is fp32, ConvDecoder.range_fallbacks).
        """
        dec = self.dec
        pos = self.savi.decoder_pos_embedding.table()
        H, W = dec.output_size(tuple(pos.shape[:2]))
        if tuple(targets.shape[-2:]) != (H, W):
            raise ValueError(f"GenericDecoderLoss: the decoder renders {H}x{W} images, the targets are "
                             f"{tuple(targets.shape[-2:])}")
        with K.range_owner(dec, "generic_precision"):
            return self._run(slots, targets, grad_scale, pos, H, W)

    def _run(self, slots, targets, grad_scale, pos, H, W):
        dec = self.dec
        F_, Ks, D = slots.shape
        k, prec, up = dec.kernel_size, dec.generic_precision, bool(dec.upsample)
        cpos, tapsum = dec._generic_layer0(pos)
        C0 = cpos.shape[-1]
        L = len(dec.hidden_dims)
        tail = dec.decoder[dec._tail_idx]
        fpc = self.chunk_frames(Ks)
        dslots = torch.empty_like(slots)
        sq = torch.zeros(1, device=slots.device, dtype=torch.float32)
        for f0 in range(0, F_, fpc):
            f1 = min(F_, f0 + fpc)
            nf = f1 - f0
            n = nf * Ks
            # forward: the calls of ConvDecoder._decode_generic, every hidden activation kept
            S = K.linear(slots[f0:f1].reshape(n, D), tapsum).reshape(n, k * k, C0)
            sc0, sh0 = dec._scale_shift(0)
            acts = [K.dec_layer0_expand(cpos, S, sc0, sh0, k, relu=True)]
            for j in range(1, L):
                sc, sh = dec._scale_shift(j)
                acts.append(K.convk(acts[-1], dec._generic_weights(j, prec), sc, sh, k, relu=True, upsample2=up,
                                    precision=prec))
            imgs, recons, masks = K.dec_tail(acts[-1], tail.weight, tail.bias, nf, Ks)
            # per-pixel loss gradient: dimg = grad_scale * (img - target)
            tgt = targets[f0:f1].contiguous()
            nel = imgs.numel()
            nblocks = min(1024, (nel + 255) // 256)
            part = torch.empty(nblocks, device=slots.device, dtype=torch.float32)
            dimg = torch.empty_like(imgs)
            K._check(_L().tocvp_mse_f32(imgs.data_ptr(), tgt.data_ptr(), part.data_ptr(), nblocks,
                                        dimg.data_ptr(), nel, float(grad_scale), _s()), "tocvp_mse_f32")
            ag.axpby(ag.colsum(part.reshape(nblocks, 1)), sq, 1.0, 1.0)
            # tail backward: compositing / softmax, then the 4 -> C transposed conv gated by the last hidden activation
            dy = torch.empty((n, H, W, 4), device=slots.device, dtype=torch.float32)
            K._check(_L().tocvp_dec_tail_grad_f32(dimg.data_ptr(), recons.data_ptr(), masks.data_ptr(),
                                                  dy.data_ptr(), nf, Ks, H, W, _s()), "tocvp_dec_tail_grad_f32")
            del imgs, recons, masks, dimg
            g = K.conv3x3_t4w(dy, tail.weight, acts[-1])
            del dy
            # hidden blocks, last to first: data gradient with the ReLU gate of the block below in the store
            for j in range(L - 1, 0, -1):
                below = acts[j - 1]
                g = K.convk_dgrad(g, self._dgrad_weights(j), tuple(below.shape[1:3]), k,
                                  gate=below if j > 1 else None, up2=up)
                acts.pop()
            del acts
            # collapsed layer 0: per-class sums (its ReLU gate and BatchNorm scale), then through the tap sums
            dS = K.dec_class_reduce_k(g, cpos, S, sc0, sh0, k)
            del g
            ds = torch.empty((n, D), device=slots.device, dtype=torch.float32)
            ag.bmm(dS, tapsum, ds, n, D, k * k * C0, k * k * C0, D, D)
            dslots[f0:f1] = ds.reshape(nf, Ks, D)
        return sq, dslots
