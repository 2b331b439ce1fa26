"""
Frozen SAVi decoder for the image-loss term of the predictor training step: forward of SAVi.decode
(SAVi.py:241-275, decoders.py:85-120) that keeps the layer activations of one chunk, the per-pixel MSE
gradient, and the hand-written backward w.r.t. the slots (the decoder's own weights are frozen,
04_train_predictor.py:62-75).  Chunk-local: the MSE gradient of a pixel depends on that pixel only, so
every chunk of frames is decoded, differentiated and dropped before the next one.

  slots --(tap-sum GEMM)--> S --relu(cpos + S[cls])--> conv1+relu --> conv2+relu --> conv3+relu
        --> 3x3 tail --> softmax over slots / compositing --> img --> sum (img - target)^2
Data gradients of the 5x5 convs = the same conv operators with transposed, flipped weights: by default the Winograd
kernel with an operand scale measured on the device per chunk (f16x3 decoder with conv_wino), else the direct bf16x3
kernel (its bf16 planes keep the fp32 exponent range per element).  The backward weights are derived from the live conv
weights through the decoder's Derived cache, so they follow load_state_dict, .to() and in-place updates as the forward
weights do.
"""

import os

import torch

from .. import kernels as K
from . import autograd as ag

__all__ = ["DecoderLoss"]

_L = K.lib
# 0: data gradients of the decoder convs on the direct bf16x3 kernel (rounds 2-4) instead of the Winograd form.
# Error model of the Winograd data gradient: one operand scale per chunk and layer, the power of two that maps max |g|
# over the whole chunk to ~4096; the fp16 planes then hold an element to fp32-class precision down to ~2^-15 of that
# maximum, coarser below (the matrix core flushes fp16 values under 2^-14), and nothing below ~2^-26 of it.  A slot
# image whose gradient is small shares the scale of the largest image in its chunk, so its own relative precision
# drops once it is below ~2^-15 of that image.  Measured against fp64 autograd (tests/test_decoder_backward_gpu.py,
# 30 saturated slots, error relative to each image's own maximum): 1.1e-4 or better down to 2^-20 of the chunk maximum
# (the same as with the bf16x3 data gradient), 5e-3 between 2^-20 and 2^-30 (bf16x3: 4e-5), 3e-2 below (bf16x3: 1e-5);
# relative to a frame's maximum, 2.4e-6 at worst.
_WINO_DGRAD = os.environ.get("TOCVP_TRAIN_WINO_DGRAD", "1") != "0"


def _s():
    return torch.cuda.current_stream().cuda_stream


class DecoderLoss:
    def __init__(self, savi, frames_per_chunk=None):
        dec = savi.decoder
        if type(dec).__name__ != "ConvDecoder" or len(dec.hidden_dims) != 4:
            raise NotImplementedError("training step: SAVi ConvDecoder with 4 conv blocks (reference config)")
        opts = [name for name, on in (("kernel_size=%d" % dec.kernel_size, dec.kernel_size != 5),
                                      ("upsample=%s" % dec.upsample, dec.upsample is not None),
                                      ("batch_norm", dec.batch_norm)) if on]
        if opts:
            raise NotImplementedError("training step: the decoder backward covers kernel 5 without upsampling or "
                                      "batch-norm; this ConvDecoder has " + ", ".join(opts))
        self.savi, self.dec = savi, dec
        self.frames_per_chunk = frames_per_chunk

    # The backward weights live in the decoder's Derived cache like its forward weights: they are rebuilt when a
    # conv weight is replaced, moved or modified in place (load_state_dict, .to(device), an update under no_grad).
    def _transposed(self, i):
        """ W'[ci][co][dy][dx] = W[co][ci][4-dy][4-dx] of conv block i """
        return self.dec.decoder[i].conv.weight.detach().flip(-1, -2).transpose(0, 1).contiguous()

    def _backward_weights(self, i):
        """ the transposed, flipped weights of conv block i split for the bf16x3 kernel (planes, fragments) """
        def build():
            wt = self._transposed(i)
            return K.split_conv_weights_bf16(wt), K.split_conv_weights_frag_bf16(wt)
        return self.dec._derived.get(f"bwd_bf16x3_{i}", [self.dec.decoder[i].conv.weight], build)

    def _zero_bias(self):
        w = self.dec.decoder[1].conv.weight
        return self.dec._derived.get("bwd_zero_bias", [w],
                                     lambda: torch.zeros(64, device=w.device, dtype=torch.float32))

    def _conv_fwd(self, i, x, collapsed=None):
        conv = self.dec.decoder[i].conv
        if self.dec.conv_precision == "f16x3" and self.dec.conv_wino:
            return K.conv5x5_dec_wino(x, self.dec._wino(i), conv.bias, relu=True, collapsed=collapsed, in_mode=2)
        if self.dec.conv_precision == "f16x3":
            return K.conv5x5_dec_f16x3(x, self.dec._split16(i), conv.bias, relu=True, collapsed=collapsed)
        if self.dec.conv_precision == "f16f8":
            return K.conv5x5_f16f8(x, self.dec._hybrid(i), conv.bias, relu=True, collapsed=collapsed)
        return K.conv5x5_bf16x3(x, self.dec._split(i), conv.bias, relu=True, collapsed=collapsed,
                                wfrag=self.dec._split_frag(i))

    def _backward_weights_wino(self, i):
        """ the same transposed, flipped weights as a Winograd weight image (split-fp16 planes, per-row scales) """
        return self.dec._derived.get(f"bwd_wino_{i}", [self.dec.decoder[i].conv.weight],
                                     lambda: K.split_conv_weights_wino_f16x3(self._transposed(i)))

    def _conv_bwd(self, i, g, gate=None):
        """ data gradient of conv block i; ``gate`` = the block's input activation (post-ReLU): the gradient
        is masked by that ReLU in the store """
        if self.dec.conv_precision == "f16x3" and self.dec.conv_wino and _WINO_DGRAD:
            # the Winograd form of the same operator (2.5 x fewer matrix products, ~2^-21 per product instead of the
            # bf16 planes' ~2^-16); the gradient's magnitude is measured on the device and sets the operand scale
            wp = self._backward_weights_wino(i)
            return K.conv5x5_dec_wino(g, wp, self._zero_bias(), relu=False, in_mode=2, out_mode=0, auto_scale=True,
                                      gate=gate)
        ws, wf = self._backward_weights(i)
        return K.conv5x5_bf16x3(g, ws, self._zero_bias(), relu=False, wfrag=wf, gate=gate)

    @torch.no_grad()
    def loss_and_slot_grad(self, slots, targets, grad_scale):
        """
        slots (F, K, D) fp32, targets (F, 3, H, W).  Returns (sum of squared pixel errors as a (1,) tensor,
        dslots (F, K, D) = grad_scale * d(sum sq err)/d(slots) / 2 ... precisely: the gradient of
        grad_scale/2 * sum (img - target)^2, i.e. pass grad_scale = 2 * weight / numel for weight * MSE).
        """
        dec = self.dec
        F_, Ks, D = slots.shape
        pos = self.savi.decoder_pos_embedding.table()
        H, W, _ = pos.shape
        cpos, tapsum = dec._collapsed_layer0(pos)
        tail = dec.decoder[4]
        fpc = self.frames_per_chunk or max(1, dec.max_slot_images // Ks)
        dslots = torch.empty_like(slots)
        sq = torch.zeros(1, device=slots.device, dtype=torch.float32)
        for f0 in range(0, F_, fpc):
            f1 = min(F_, f0 + fpc)
            nf = f1 - f0
            n = nf * Ks
            sl = slots[f0:f1].reshape(n, D).contiguous()
            S = K.linear(sl, tapsum).reshape(n, 25, 64)
            x1 = self._conv_fwd(1, None, collapsed=(cpos, S))
            x2 = self._conv_fwd(2, x1)
            x3 = self._conv_fwd(3, x2)
            imgs, recons, masks = K.dec_tail(x3, tail.weight, tail.bias, nf, Ks)
            # per-pixel loss gradient: dimg = grad_scale * (img - target)
            tgt = targets[f0:f1].contiguous()
            nel = imgs.numel()
            nblocks = min(1024, (nel + 255) // 256)
            part = torch.empty(nblocks, device=slots.device, dtype=torch.float32)
            dimg = torch.empty_like(imgs)
            K._check(_L().tocvp_mse_f32(imgs.data_ptr(), tgt.data_ptr(), part.data_ptr(), nblocks,
                                        dimg.data_ptr(), nel, float(grad_scale), _s()), "tocvp_mse_f32")
            ag.axpby(ag.colsum(part.reshape(nblocks, 1)), sq, 1.0, 1.0)
            # tail backward
            dy = torch.empty((n, H, W, 4), device=slots.device, dtype=torch.float32)
            K._check(_L().tocvp_dec_tail_grad_f32(dimg.data_ptr(), recons.data_ptr(), masks.data_ptr(),
                                                  dy.data_ptr(), nf, Ks, H, W, _s()), "tocvp_dec_tail_grad_f32")
            g = torch.empty_like(x3)
            K._check(_L().tocvp_conv3x3_t4_f32(dy.data_ptr(), tail.weight.data_ptr(), x3.data_ptr(),
                                               g.data_ptr(), n, H, W, 64, _s()), "tocvp_conv3x3_t4_f32")
            del dy, x3, recons, masks, imgs, dimg
            # conv 3 and 2: data gradient, then the ReLU mask of the layer below
            for i, act in ((3, x2), (2, x1)):
                g = self._conv_bwd(i, g, gate=act)
            del x1, x2
            gin = self._conv_bwd(1, g)
            dS = torch.empty((n, 25, 64), device=slots.device, dtype=torch.float32)
            K._check(_L().tocvp_dec_class_reduce_f32(gin.data_ptr(), cpos.data_ptr(), S.data_ptr(),
                                                     dS.data_ptr(), n, H, W, 64, _s()),
                     "tocvp_dec_class_reduce_f32")
            ds = torch.empty((n, D), device=slots.device, dtype=torch.float32)
            ag.bmm(dS, tapsum, ds, n, D, 25 * 64, 25 * 64, D, D)
            dslots[f0:f1] = ds.reshape(nf, Ks, D)
        return sq, dslots
