"""
Slot decoders.  Reference: models/EncodersDecoders/decoders.py (get_decoder :20-48,
ConvDecoder :52-125).
"""

import os

import torch
import torch.nn as nn

from ... import kernels as K
from ...precision import knob
from ..Blocks.model_blocks import ConvBlock, Upsample
from ..Blocks.model_utils import Derived

# MLPPatchDecoder: hidden activations between its Linear layers as producer-written fp16 operand planes
# (TOCVP_DINO_MLP_PLANES=0 restores the fp32 hand-over): the 1024 -> 1024 layers then run the chunk-resident GEMM
# (gemm_f16c.hip), bit-identical to the fp32 hand-over
_MLP_PLANES = os.environ.get("TOCVP_DINO_MLP_PLANES", "1") != "0"
_MLP_PLANES_MIN_ROWS = int(os.environ.get("TOCVP_DINO_MLP_PLANES_MIN_ROWS", "16384"))
# image head: "Upsample(x2) -> Conv3x3" as four 2x2 phase convolutions (TOCVP_DINO_UP2_PHASES=0: 3x3 conv with the
# upsampling fused into its tile loader, round 1)
_UP2_PHASES = os.environ.get("TOCVP_DINO_UP2_PHASES", "1") != "0"

__all__ = ["get_decoder", "ConvDecoder", "MLPPatchDecoder"]


def get_decoder(in_channels, decoder, **kwargs):
    """ Factory; pops keys from the params dict like the reference (decoders.py:32-34). """
    name, params = decoder["decoder_name"], decoder["decoder_params"]
    if name == "ConvDecoder":
        return ConvDecoder(in_channels=in_channels, hidden_dims=params.pop("num_channels"),
                           kernel_size=params.pop("kernel_size"), upsample=params.pop("upsample"),
                           out_channels=kwargs.get("out_channels", 4), **params)
    if name == "MLPPatchDecoder":
        return MLPPatchDecoder(**params)
    raise NotImplementedError(f"Unknown decoder {name}...")


class ConvDecoder(nn.Module):
    """
    Spatial-broadcast conv decoder: 4x (Conv5x5 + ReLU) at full resolution, then Conv3x3 -> RGB+alpha.
    Layers are built from hidden_dims[-1] down to hidden_dims[0] (decoders.py:96-117).

    MI355X path (``decode_slots``):
      layer 0   never runs as a conv: its input is broadcast(slot) + pos, so its output is
                cpos[y,x,:] + tapsum[cls(y,x)] @ slot  (exact algebra, 25 border classes);
                cpos = conv0(pos)+b0 is computed ONCE per weight set with the MFMA conv kernel.
      layer 1   tocvp_conv5x5_f32 in collapsed-input mode (synthesises relu(layer 0) on the fly)
      layer 2-3 tocvp_conv5x5_f32
      tail      tocvp_dec_tail_f32: conv3x3 + softmax over slots + compositing, writing the
                reference's three output tensors directly.

    Variants of the reference factory (kernel 3 / 7, ``upsample: 2``, ``batch_norm``, widths 32 / 64 / 128) take the
    generic path (``_decode_generic``): layer 0 collapsed over k x k border classes, the hidden layers on
    kernels.convk (nearest x2 upsampling as four phase convolutions over the source image, eval BatchNorm folded into
    the epilogue), the exact fp32 tail at the output resolution ``resolution * 2 ** (L - 1)``.
    """

    def __init__(self, in_channels, hidden_dims, kernel_size=5, upsample=None, out_channels=4,
                 **kwargs):
        super().__init__()
        upsample = None if upsample is None or upsample < 2 else upsample
        batch_norm = bool(kwargs.get("batch_norm"))
        if upsample is not None and upsample != 2:
            raise NotImplementedError(f"ConvDecoder: upsample {upsample} (only nearest x2 is fused into the convs)")
        if kwargs.get("stride", 1) != 1:
            raise NotImplementedError("ConvDecoder: stride != 1")
        if kernel_size not in (3, 5, 7):
            raise NotImplementedError(f"ConvDecoder: kernel {kernel_size} (3, 5 or 7)")
        if out_channels != 4 or len(hidden_dims) < 2:
            raise NotImplementedError("ConvDecoder: RGB + alpha output, >= 2 hidden layers")
        # the shipped configuration (k 5, no upsampling, no batch-norm) keeps its dedicated path; every other one runs
        # the generic path, whose convs take 32 / 64 / 128 channels
        self.generic = kernel_size != 5 or upsample is not None or batch_norm
        if self.generic and any(c not in K.SAVI_WIDTHS for c in list(hidden_dims) + [in_channels]):
            raise NotImplementedError(f"ConvDecoder: widths {list(hidden_dims)} / slot dim {in_channels} "
                                      f"(the variants take {K.SAVI_WIDTHS})")
        self.in_channels = self.in_features = in_channels
        self.hidden_dims, self.kernel_size = hidden_dims, kernel_size
        self.out_features, self.out_channels = hidden_dims[0], out_channels
        self.upsample, self.batch_norm = upsample, batch_norm
        mods, c = [], in_channels
        self._block_idx = []
        for i in range(len(hidden_dims) - 1, -1, -1):
            self._block_idx.append(len(mods))
            mods.append(ConvBlock(c, hidden_dims[i], kernel_size, padding=kernel_size // 2, batch_norm=batch_norm))
            c = hidden_dims[i]
            if upsample is not None and i > 0:            # reference key layout: parameter-free entries in between
                mods.append(Upsample(scale_factor=upsample))
        self._tail_idx = len(mods)
        mods.append(nn.Conv2d(self.out_features, out_channels, kernel_size=3, stride=1, padding=1))
        self.decoder = nn.Sequential(*mods)
        self._derived = Derived()
        # slot images decoded per chunk (bounds HBM scratch: ~2.7 MB per slot image)
        self.max_slot_images = int(os.environ.get("TOCVP_DEC_MAX_SLOT_IMAGES", "2048"))
        # arithmetic of the 64->64 convs:
        #   "f16x3"  (default) split-fp16 operands, 3 f16 matrix products, ~2^-21 per product = fp32-class;
        #            the only split mode that holds the 1e-4 bar with margin on weights with an O(1) RGB
        #            head (profiles/r02_parity_by_mode.md).  Needs W % 64 == 0, H % 8 == 0 (else bf16x3).
        #   "fp32"   exact fp32 MFMA;
        #   "bf16x3" split-bf16 operands (~2^-16 per product), range-free;
        #   "f16f8"  f16 main product + two e4m3 cross products (2/3 of the matrix cycles, ~2^-15 per
        #            product): fastest, but beyond 1e-4 on recons / masks for un-damped heads -> opt-in.
        self.conv_precision = knob("TOCVP_DECODER_PRECISION", "f16x3")
        self.pass_major = os.environ.get("TOCVP_CONV_PASS_MAJOR", "1") != "0"
        # f16x3 layers hand their activations over as fp16 operand planes (the consumer stages them by LDS-DMA)
        self.conv_planes = os.environ.get("TOCVP_CONV_PLANES", "1") != "0"
        # the tail Conv2d(64 -> 4, k = 3) folded into the last hidden layer's epilogue (36 tap products per pixel leave
        # the chip instead of 64 channels; tocvp_dec_tail_sum_f32 adds the nine shifted planes)
        self.tail_fold = os.environ.get("TOCVP_DEC_TAIL_FOLD", "1") != "0"
        # the 64 -> 64 layers as vertical Winograd F(4, 5) x five horizontal taps (csrc/conv_wino.hip): 2.5 x fewer
        # matrix products in the same split-fp16 arithmetic, same error class (scripts/probes/winograd_numerics.py)
        self.conv_wino = os.environ.get("TOCVP_CONV_WINO", "1") != "0"
        # arithmetic of the generic path's convs: f16x3 or fp32 (bf16x3 -> fp32, f16f8 -> f16x3: KNOBS.md)
        self.generic_precision = {"bf16x3": "fp32", "f16f8": "f16x3"}.get(self.conv_precision, self.conv_precision)

    # -- derived weights -----------------------------------------------------------------------
    def _packed(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"wp{i}", [conv.weight], lambda: K.pack_conv_weights(conv.weight))

    def _split(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"ws{i}", [conv.weight],
                                 lambda: K.split_conv_weights_bf16(conv.weight))

    def _split_frag(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"wf{i}", [conv.weight],
                                 lambda: K.split_conv_weights_frag_bf16(conv.weight))

    def _hybrid(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"wh{i}", [conv.weight],
                                 lambda: K.split_conv_weights_f16f8(conv.weight))

    def _split16(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"w16{i}", [conv.weight],
                                 lambda: K.split_conv_weights_dec_f16x3(conv.weight))

    def _wino(self, i):
        conv = self.decoder[i].conv
        return self._derived.get(f"wino{i}", [conv.weight],
                                 lambda: K.split_conv_weights_wino_f16x3(conv.weight))

    def _tail_taps(self):
        tail = self.decoder[len(self.hidden_dims)]
        return self._derived.get("tail_taps", [tail.weight], lambda: K.pack_tail_taps_f16x3(tail.weight))

    def _collapsed_layer0(self, pos_table):
        """ (cpos (H,W,C0), tapsum (25*C0, D)) for the current weights / position table """
        c0 = self.decoder[0].conv

        def build():
            cpos = K.conv5x5(pos_table[None].contiguous(), K.pack_conv_weights(c0.weight), c0.bias,
                             relu=False)[0].contiguous()
            ts = K.dec_tapsum(c0.weight)
            return cpos, ts.reshape(25 * ts.shape[1], ts.shape[2])
        return self._derived.get("layer0", [c0.weight, c0.bias, pos_table], build)

    range_fallbacks = {"conv_precision": {"f16x3": "bf16x3", "f16f8": "bf16x3"},
                       "generic_precision": {"f16x3": "fp32"}}

    # -- forward -------------------------------------------------------------------------------
    def output_size(self, resolution):
        """ (H, W) of the decoded images for a broadcast ``resolution`` """
        s = 2 ** (len(self.hidden_dims) - 1) if self.upsample else 1
        return resolution[0] * s, resolution[1] * s

    def decode_slots(self, slots, pos_table, out=None):
        if self.generic:
            with K.range_owner(self, "generic_precision"):
                return self._decode_generic(slots, pos_table, out=out)
        with K.range_owner(self, "conv_precision"):
            return self._decode_slots(slots, pos_table, out=out)

    # -- generic path (variants) ---------------------------------------------------------------
    def _block_params(self, j):
        """ hidden block j (0 = the one fed by the broadcast): (block, [tensors its derived weights depend on]) """
        blk = self.decoder[self._block_idx[j]]
        deps = [blk.conv.weight, blk.conv.bias]
        if self.batch_norm:
            bn = blk.block[1]
            deps += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return blk, deps

    def _scale_shift(self, j):
        blk, deps = self._block_params(j)
        return self._derived.get(f"gss{j}", deps, blk.folded_scale_shift)

    def _generic_weights(self, j, precision):
        """ packed weights of hidden block j >= 1 for kernels.convk: phase form for f16x3 after an upsampling """
        blk, _ = self._block_params(j)
        w = blk.conv.weight
        if self.upsample and precision == "f16x3":
            return self._derived.get(f"gwu{j}", [w], lambda: K.pack_conv_up2_weights(w))
        return self._derived.get(f"gw{j}", [w], lambda: K.pack_conv_weights(w))

    def _generic_layer0(self, pos_table):
        """ (cpos (H, W, C0) = conv0(pos) without bias, tapsum (k k C0, D)) of the collapsed layer 0 """
        c0 = self.decoder[self._block_idx[0]].conv
        k = self.kernel_size

        def build():
            zero = torch.zeros(c0.weight.shape[0], device=c0.weight.device, dtype=torch.float32)
            cpos = K.convk(pos_table[None].contiguous(), K.pack_conv_weights(c0.weight), None, zero, k, relu=False,
                           precision="fp32")[0].contiguous()
            ts = K.dec_tapsum_k(c0.weight)
            return cpos, ts.reshape(k * k * ts.shape[1], ts.shape[2])
        return self._derived.get("glayer0", [c0.weight, pos_table], build)

    def _decode_generic(self, slots, pos_table, out=None):
        """ slots (F, K, D), pos_table (H0, W0, D) -> recons_imgs (F,3,H,W), recons (F,K,3,H,W), masks (F,K,1,H,W) at
        the output size; ``out`` as for _decode_slots """
        F_, Ks, D = slots.shape
        H0, W0, _ = pos_table.shape
        H, W = self.output_size((H0, W0))
        k, prec = self.kernel_size, self.generic_precision
        cpos, tapsum = self._generic_layer0(pos_table)
        C0 = cpos.shape[-1]
        dev = slots.device
        if out is not None:
            imgs, recons, masks = out[:3]
            clamped = out[3] if len(out) > 3 else None
        else:
            imgs = torch.empty((F_, 3, H, W), device=dev, dtype=torch.float32)
            recons = torch.empty((F_, Ks, 3, H, W), device=dev, dtype=torch.float32)
            masks = torch.empty((F_, Ks, 1, H, W), device=dev, dtype=torch.float32)
            clamped = None
        tail = self.decoder[self._tail_idx]
        fpc = max(1, self.max_slot_images // Ks)
        for f0 in range(0, F_, fpc):
            f1 = min(F_, f0 + fpc)
            n = (f1 - f0) * Ks
            S = K.linear(slots[f0:f1].reshape(n, D), tapsum).reshape(n, k * k, C0)
            sc, sh = self._scale_shift(0)
            x = K.dec_layer0_expand(cpos, S, sc, sh, k, relu=True)
            for j in range(1, len(self.hidden_dims)):
                sc, sh = self._scale_shift(j)
                x = K.convk(x, self._generic_weights(j, prec), sc, sh, k, relu=True, upsample2=bool(self.upsample),
                            precision=prec)
            dst = (imgs[f0:f1], recons[f0:f1], masks[f0:f1]) + ((clamped[f0:f1],) if clamped is not None else ())
            K.dec_tail(x, tail.weight, tail.bias, f1 - f0, Ks, out=dst)
        return imgs, recons, masks

    def _decode_slots(self, slots, pos_table, out=None):
        """
        slots (F, K, D), pos_table (H, W, D) -> recons_imgs (F,3,H,W), recons (F,K,3,H,W),
        masks (F,K,1,H,W)   (SAVi.decode, models/SAVi.py:241-261)
        ``out`` = optional (recons_imgs, recons, masks[, clamped_imgs]) destination views (kernels._tail_outputs).
        """
        F_, Ks, D = slots.shape
        H, W, _ = pos_table.shape
        dev = slots.device
        n_hidden = len(self.hidden_dims)
        cpos, tapsum = self._collapsed_layer0(pos_table)
        C0 = cpos.shape[-1]
        if out is not None:
            imgs, recons, masks = out[:3]
            clamped = out[3] if len(out) > 3 else None
        else:
            imgs = torch.empty((F_, 3, H, W), device=dev, dtype=torch.float32)
            recons = torch.empty((F_, Ks, 3, H, W), device=dev, dtype=torch.float32)
            masks = torch.empty((F_, Ks, 1, H, W), device=dev, dtype=torch.float32)
            clamped = None
        tail = self.decoder[n_hidden]
        fpc = max(1, self.max_slot_images // Ks)             # frames per chunk
        bufs = [None, None]
        prod = None
        for f0 in range(0, F_, fpc):
            f1 = min(F_, f0 + fpc)
            n = (f1 - f0) * Ks
            S = K.linear(slots[f0:f1].reshape(n, D), tapsum).reshape(n, 25, C0)
            x, which, pm_prev, folded, check_last, x16_prev = None, 0, False, False, False, False
            for i in range(1, n_hidden):
                conv = self.decoder[i].conv
                co = conv.weight.shape[0]
                out = bufs[which]
                if out is None or out.shape != (n, H, W, co):
                    out = torch.empty((n, H, W, co), device=dev, dtype=torch.float32)
                    bufs[which] = out
                c64 = conv.weight.shape[0] == 64 and conv.weight.shape[1] == 64
                split = self.conv_precision in ("bf16x3", "f16f8", "f16x3") and c64
                fold = (self.tail_fold and i == n_hidden - 1 and i > 1 and self.conv_precision == "f16x3" and c64
                        and W % 64 == 0 and H % 8 == 0 and tuple(tail.weight.shape) == (4, 64, 3, 3))
                if fold and K._CHECK_RANGE:
                    # range-checked pass: the folded epilogue turns relu(y3) into fp16 operand planes (saturating at
                    # 255.9) without ever materialising it, so THIS pass runs the layer unfolded below, verifies its
                    # output against the plane range and hands it to the exact fp32 tail -- a checkpoint whose last
                    # hidden activation leaves the range raises here and takes the decoder's fallback (bf16x3, no fold)
                    fold = False
                    check_last = True
                if self.conv_wino and self.conv_precision == "f16x3" and c64 and W % 64 == 0 and H % 8 == 0:
                    # Winograd layers hand 16 * activation over in the pass-major fp32 layout; the last one writes the
                    # folded tail's tap products (or NHWC fp32 for the exact tail on the range-checked pass)
                    nxt = self.decoder[i + 1].conv if i + 1 < n_hidden else None
                    last = nxt is None or tuple(nxt.weight.shape[:2]) != (64, 64)     # no Winograd layer behind this one
                    kw = dict(collapsed=(cpos, S)) if i == 1 else dict(in_mode=0 if x16_prev else 2)
                    x16_prev = not last
                    if fold:
                        if prod is None or prod.shape[0] != n:
                            prod = torch.empty((n, 36, H, W), device=dev, dtype=torch.float32)
                        K.conv5x5_dec_wino(x, self._wino(i), conv.bias, relu=True, out=prod, out_mode=3,
                                           tail_taps=self._tail_taps(), **kw)
                        folded = True
                        break
                    x = K.conv5x5_dec_wino(x, self._wino(i), conv.bias, relu=True,
                                           out=out if last else out.view(n, 4, H, W, 16), out_mode=0 if last else 1, **kw)
                    which ^= 1
                    continue
                if fold:
                    # last hidden layer: the tail's tap products leave its epilogue, the tail only sums them
                    if prod is None or prod.shape[0] != n:
                        prod = torch.empty((n, 36, H, W), device=dev, dtype=torch.float32)
                    planes_in = self.conv_planes and pm_prev and H * W <= 16384
                    K.conv5x5_dec_f16x3_tail(x, self._split16(i), conv.bias, self._tail_taps(), relu=True, out=prod,
                                             pm_in=pm_prev, planes=planes_in)
                    folded = True
                    break
                if self.conv_precision in ("f16f8", "f16x3") and c64 and W % 64 == 0 and H % 8 == 0:
                    # consecutive tiled layers hand their activations over in the pass-major layout
                    nxt = self.decoder[i + 1].conv if i + 1 < n_hidden else None
                    pm_out = self.pass_major and nxt is not None and tuple(nxt.weight.shape[:2]) == (64, 64)
                    if self.conv_precision == "f16x3":
                        x = K.conv5x5_dec_f16x3(x, self._split16(i), conv.bias, relu=True, out=out,
                                                collapsed=(cpos, S) if i == 1 else None,
                                                pm_in=pm_prev, pm_out=pm_out,
                                                planes=self.conv_planes and H * W <= 16384)
                    else:
                        x = K.conv5x5_f16f8(x, self._hybrid(i), conv.bias, relu=True, out=out,
                                            collapsed=(cpos, S) if i == 1 else None,
                                            pm_in=pm_prev, pm_out=pm_out)
                    pm_prev = pm_out
                elif split:
                    x = K.conv5x5_bf16x3(x, self._split(i), conv.bias, relu=True, out=out,
                                         collapsed=(cpos, S) if i == 1 else None,
                                         wfrag=self._split_frag(i))
                elif i == 1:
                    x = K.conv5x5_collapsed(cpos, S, self._packed(1), conv.bias, relu=True, out=out)
                else:
                    x = K.conv5x5(x, self._packed(i), conv.bias, relu=True, out=out)
                which ^= 1
            if check_last:
                K._check_f16_range(K.absmax(x), "decoder: last hidden activation (operand of the folded tail)")
            dst = (imgs[f0:f1], recons[f0:f1], masks[f0:f1]) + ((clamped[f0:f1],) if clamped is not None else ())
            if folded:
                K.dec_tail_sum(prod, tail.bias, f1 - f0, Ks, out=dst)
            else:
                K.dec_tail(x, tail.weight, tail.bias, f1 - f0, Ks, out=dst)
        return imgs, recons, masks

    def forward(self, x):
        raise NotImplementedError(
            "ConvDecoder.forward on a materialised (B*K, D, H, W) broadcast is deliberately not "
            "provided: use SAVi.decode / decode_slots (the broadcast tensor never exists here)")


def _pad_rows32(weight, bias, mult=32):
    """ (N, K) weight / (N,) bias zero-padded to the next multiple of ``mult`` output features """
    n = weight.shape[0]
    npad = (n + mult - 1) // mult * mult
    w = torch.zeros((npad, weight.shape[1]), device=weight.device, dtype=weight.dtype)
    w[:n] = weight.detach()
    b = torch.zeros((npad,), device=weight.device, dtype=weight.dtype)
    if bias is not None:
        b[:n] = bias.detach()
    return w.contiguous(), b


class MLPPatchDecoder(nn.Module):
    """
    Slot -> ViT-patch-feature decoder of ExtendedDINOSAUR (reference decoders.py:129-365):
    broadcast slots over the patches + learned position embedding -> [LayerNorm] -> MLP ->
    (features, alpha) -> softmax over slots -> weighted sum; optional CNN head that renders the
    image from the reconstructed feature grid (Conv3x3 + BatchNorm + ReLU blocks with nearest x2
    upsampling in between, final Conv3x3 -> RGB, bilinear resize to the image size).

    MI355X path: the position add is fused into the LayerNorm prologue, the MLP runs on the MFMA
    GEMMs with fused ReLU, the alpha-softmax + weighted sum is one kernel, eval-mode BatchNorm is
    folded into the conv epilogue and every nearest upsampling is fused into the NEXT conv's tile
    loader (the 4x larger tensors are never written).
    """

    def __init__(self, num_patches, in_dim, hidden_dim, out_dim, num_layers=4,
                 initial_layer_norm=False, reconstruct_images=False, **kwargs):
        super().__init__()
        self.num_patches, self.in_dim = num_patches, in_dim
        self.pos_embed = nn.Parameter(torch.randn(1, 1, num_patches, in_dim) / (in_dim ** 0.5))
        self.patch_grid = (int(num_patches ** 0.5), int(num_patches ** 0.5))
        self.hidden_dim, self.out_dim, self.num_layers = hidden_dim, out_dim, num_layers
        self.initial_layer_norm = initial_layer_norm
        mlp = [nn.LayerNorm(in_dim)] if initial_layer_norm else []
        for i in range(num_layers):
            d1 = hidden_dim if i > 0 else in_dim
            d2 = hidden_dim if i < num_layers - 1 else out_dim
            mlp.append(nn.Linear(d1, d2))
            if i < num_layers - 1:
                mlp.append(nn.ReLU())
        self.mlp = nn.Sequential(*mlp)
        self.reconstruct_images = reconstruct_images
        if reconstruct_images:
            self.patch_size = kwargs.get("patch_size")
            self.image_size = kwargs.get("img_size")
            self.num_layers_cnn = kwargs.get("num_layers_cnn")
            self.conv_patch_decoder, self._upsample_after = self._build_conv_patch_decoder(
                in_dim=out_dim - 1, hidden_dim=hidden_dim, num_layers=self.num_layers_cnn,
                patch_size=self.patch_size)
        self._derived = Derived()
        self.mlp_precision = knob("TOCVP_DECODER_MLP_PRECISION", "f16x3")
        self.conv_precision = knob("TOCVP_DECODER_CNN_PRECISION", "f16x3")   # image head convs

    def _build_conv_patch_decoder(self, in_dim, hidden_dim, num_layers, patch_size):
        """ same layer / channel / upsampling schedule as the reference (decoders.py:325-365) """
        from ..Blocks.model_blocks import Upsample
        mods, ups = [], []
        size = self.patch_grid[0]
        for i in range(num_layers):
            cin = in_dim if i == 0 else hidden_dim
            if i > 0 and (i + 1) * 2 < patch_size and size < self.image_size:
                hidden_dim = hidden_dim // 2
            mods.append(ConvBlock(cin, hidden_dim, kernel_size=3, stride=1, padding=1, batch_norm=True))
            if (i + 1) * 2 < patch_size and size < self.image_size:
                mods.append(Upsample(scale_factor=2))
                size *= 2
                ups.append(True)
            else:
                ups.append(False)
        mods.append(nn.Conv2d(hidden_dim, 3, kernel_size=3, stride=1, padding=1))
        return nn.Sequential(*mods), ups

    range_fallbacks = {"mlp_precision": {"f16x3": "fp32"}, "conv_precision": {"f16x3": "fp32"}}

    # -- image head on the kernels ---------------------------------------------------------------
    def _render(self, feats, keep=None):
        with K.range_owner(self, "conv_precision"):
            return self._render_impl(feats, keep)

    def _render_impl(self, feats, keep=None):
        """ feats (B, N, F) -> images (B, 3, S, S); ``keep`` (a list) receives every block's post-ReLU output and the
        final conv's (B, S', S', 32) output before the resize (the training step's backward reads them) """
        B = feats.shape[0]
        g = self.patch_grid[0]
        x = feats.reshape(B, g, g, feats.shape[-1]).contiguous()           # NHWC feature grid
        blocks = [m for m in self.conv_patch_decoder if isinstance(m, ConvBlock)]
        up_next = False
        # "Upsample(x2) -> Conv3x3" as four 2x2 phase convolutions over the source image (2.25x fewer FLOPs, same result up
        # to the fp32 rounding of the summed taps; f16x3 arithmetic only)
        phases = _UP2_PHASES and self.conv_precision == "f16x3"
        for blk, up in zip(blocks, self._upsample_after):
            conv = blk.conv
            wp = self._derived.get(("wp", id(blk)), [conv.weight],
                                   lambda c=conv: K.pack_conv_weights(c.weight))
            sc, sf = self._derived.get(
                ("ss", id(blk)), [conv.bias] + [t for t in blk.block[1].state_dict().values()
                                                if t.is_floating_point()],
                lambda b=blk: b.folded_scale_shift())
            if up_next and phases:
                wph = self._derived.get(("wph", id(blk)), [conv.weight], lambda c=conv: K.pack_conv3x3_up2_weights(c.weight))
                x = K.conv3x3_up2(x, wph, sc, sf, relu=True)
            else:
                x = K.conv3x3(x, wp, sc, sf, relu=True, upsample2=up_next, precision=self.conv_precision)
            if keep is not None:
                keep.append(x)
            up_next = up
        final = self.conv_patch_decoder[-1]

        def pack_final():
            w = torch.zeros((32,) + tuple(final.weight.shape[1:]), device=final.weight.device)
            w[:3] = final.weight
            b = torch.zeros(32, device=final.weight.device)
            b[:3] = final.bias
            return K.pack_conv_weights(w), b
        wp, bias = self._derived.get("final", [final.weight, final.bias], pack_final)
        if up_next and phases:
            def pack_final_up2():
                w = torch.zeros((32,) + tuple(final.weight.shape[1:]), device=final.weight.device)
                w[:3] = final.weight
                return K.pack_conv3x3_up2_weights(w)
            wph = self._derived.get("final_up2", [final.weight], pack_final_up2)
            x = K.conv3x3_up2(x, wph, None, bias, relu=False)                   # (B, S', S', 32), 3 used
        else:
            x = K.conv3x3(x, wp, None, bias, relu=False, upsample2=up_next,     # (B, S', S', 32), 3 used
                          precision=self.conv_precision)
        if keep is not None:
            keep.append(x)
        S = self.image_size
        return K.bilinear_resize_nhwc_to_nchw(x, 3, S, S)                  # also the NHWC->NCHW step

    def forward(self, slots):
        """ slots (B, K, D) -> {'recons_imgs', 'recons_feats' (B,N,F), 'masks' (B,K,1,g,g)} """
        B, Ks, D = slots.shape
        N = self.num_patches
        x = slots.reshape(B * Ks, 1, D).expand(B * Ks, N, D).contiguous()  # broadcast (data movement)
        pos = self.pos_embed.detach().reshape(N, D)
        if not self.initial_layer_norm:
            raise NotImplementedError("MLPPatchDecoder without initial_layer_norm (unused by the configs)")
        ln = self.mlp[0]
        linears = [m for m in self.mlp[1:] if isinstance(m, nn.Linear)]
        # 37 GFLOP per frame at config 4: f16x3 split operands (fp32-class) for the layers whose
        # shapes fit the fragment-order kernel; the 769-wide head stays on the exact fp32 MFMA
        with K.gemm_precision(self.mlp_precision, owner=(self, "mlp_precision")):
            # hidden activations handed from layer to layer as fp16 operand planes written by the producing
            # kernel (the split the consumer would compute while staging: bit-identical); the checked pass
            # keeps fp32 hand-overs so that every activation is verified by its consumer
            planes = (_MLP_PLANES and K.active_nsplit() == 22 and not K._CHECK_RANGE and
                      B * Ks * N >= _MLP_PLANES_MIN_ROWS and D % 64 == 0 and
                      all(l.weight.shape[0] % 32 == 0 and l.weight.shape[1] % 64 == 0 for l in linears[:-1]))
            x = K.layer_norm(x, ln.weight, ln.bias, ln.eps, add=pos, split=22 if planes else 0)
            for j, lin in enumerate(linears[:-1]):
                x = K.linear(x, lin.weight, lin.bias, act=K.ACT_RELU, out_split=22 if planes else 0)
            # the head is out_dim = F + 1 wide (769): zero-padded to a multiple of 32 so that it runs
            # the split kernel too; the compositing kernel skips the padding columns
            # (with plane hand-overs the padding goes to a multiple of 512 instead: the chunk-resident GEMM on 1024 columns
            # is faster than the 64 x 64-tiled one on 800 -- 497 vs 632 us per 98304 rows)
            head = linears[-1]
            mult = 512 if planes and K._GEMM_CHUNK and head.weight.shape[1] % 128 == 0 else 32
            wpad, bpad = self._derived.get(("head_pad", mult), [head.weight, head.bias],
                                           lambda: _pad_rows32(head.weight, head.bias, mult))
            x = K.linear(x, wpad, bpad)
        recons_feats, masks = K.slot_composite(x.reshape(B, Ks, N, wpad.shape[0]),
                                               feat_dim=self.out_dim - 1)
        recons_imgs = torch.tensor([])
        if self.reconstruct_images:
            recons_imgs = self._render(recons_feats)
        return {"recons_imgs": recons_imgs, "recons_feats": recons_feats,
                "masks": masks.reshape(B, Ks, 1, *self.patch_grid)}
