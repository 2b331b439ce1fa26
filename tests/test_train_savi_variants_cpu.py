"""
Predictor training on frozen SAVi variants, on the CPU: the data-gradient weights of the variant convolutions in fp64
against torch.autograd (plain k x k conv and "nearest x2 -> k x k conv", every width pairing, BatchNorm scale folded),
their agreement with the ExtendedDINOSAUR head's 3x3 packer, and the training step's decoder selection for every variant
manifest (tests/golden/state_dict_manifest_savi_<tag>.json).
"""

import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from textocvp_amd import kernels as K
from textocvp_amd.setup_model import default_exp_params, setup_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("up2", "k3", "bn_up2_128", "k7_mixed")
WIDTHS = (32, 64, 128)


def manifest(tag):
    with open(os.path.join(GOLDEN, f"state_dict_manifest_savi_{tag}.json")) as f:
        return json.load(f)


def _dgrad_by_taps(g, wd, k, up2, out_hw):
    """ the kernel's contract in fp64: dx[y, x] = sum_taps g[S y + ty - k // 2, S x + tx - k // 2] . wd[tap] (zero outside),
    g (n, Cg, GH, GW), wd (taps, Cout, Cg) -> (n, Cout, H, W) """
    S, nt, r = (2, k + 1, k // 2) if up2 else (1, k, k // 2)
    H, W = out_hw
    n, Cg, GH, GW = g.shape
    pad = nt                                                  # generous zero border
    gp = F.pad(g, (pad, pad, pad, pad))
    dx = torch.zeros((n, wd.shape[1], H, W), dtype=torch.float64)
    for ty in range(nt):
        for tx in range(nt):
            y0, x0 = pad + ty - r, pad + tx - r
            win = gp[:, :, y0:y0 + S * (H - 1) + 1:S, x0:x0 + S * (W - 1) + 1:S]           # (n, Cg, H, W)
            dx += torch.einsum("ncyx,oc->noyx", win, wd[ty * nt + tx])
    return dx


def _grid():
    cases, i = [], 0
    for k in (3, 5, 7):
        for up2 in (False, True):
            for cg in WIDTHS:
                for cout in WIDTHS:
                    cases.append((k, up2, cg, cout, i % 2 == 0))
                    i += 1
    return cases


@pytest.mark.parametrize("k,up2,cg,cout,bn", _grid())
def test_dgrad_weights_reproduce_autograd(k, up2, cg, cout, bn):
    """ forward conv Cout_fwd = cg channels out of Cin_fwd = cout channels in; the data gradient maps cg -> cout """
    gen = torch.Generator().manual_seed(100 * k + cg + cout + up2)
    H, W = (5, 6) if up2 else (7, 9)
    x = torch.randn((2, cout, H, W), generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn((cg, cout, k, k), generator=gen, dtype=torch.float64)
    scale = (0.5 + torch.rand(cg, generator=gen, dtype=torch.float64)) if bn else None
    u = F.interpolate(x, scale_factor=2, mode="nearest") if up2 else x
    y = F.conv2d(u, w, padding=k // 2)
    if scale is not None:
        y = y * scale[None, :, None, None]
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (ref,) = torch.autograd.grad(y, x, g)
    wd = K.convk_dgrad_weights64(w, scale, up2=up2)
    assert tuple(wd.shape) == (((k + 1) ** 2 if up2 else k * k), cout, cg)
    got = _dgrad_by_taps(g, wd, k, up2, (H, W))
    err = (got - ref).abs().max().item()
    assert err <= 1e-12 * ref.abs().max().item(), err


@pytest.mark.parametrize("up2", [False, True])
@pytest.mark.parametrize("bn", [False, True])
def test_k3_dgrad_weights_match_patch_decoder_packer(up2, bn):
    from textocvp_amd.train.patch_decoder import _dgrad_weights
    gen = torch.Generator().manual_seed(7 + up2 + 2 * bn)
    w = torch.randn((64, 32, 3, 3), generator=gen)
    scale = (0.5 + torch.rand(64, generator=gen)) if bn else None
    ref = _dgrad_weights(w, scale, up2)
    assert torch.equal(K.convk_dgrad_weights64(w, scale, up2=up2).float(), ref)
    planes = K.pack_convk_dgrad_weights(w, scale, up2=up2)
    assert planes.dtype == torch.bfloat16 and tuple(planes.shape) == (2,) + tuple(ref.shape)
    # hi + lo carries the fp32 weight to ~2^-16 relative
    assert ((planes[0].double() + planes[1].double()) - ref.double()).abs().max() <= 2 ** -15 * ref.abs().max()


def _savi(tag):
    model_params = copy.deepcopy(manifest(tag)["model_params"])
    exp = default_exp_params(num_slots=model_params["num_slots"], num_context=1, num_preds=2)
    exp["model"]["model_params"] = model_params
    return setup_model(exp["model"]).eval()


@pytest.mark.parametrize("tag", VARIANTS)
def test_training_step_selects_generic_decoder_loss(tag):
    """ the decoder selection of PredictorTrainStep (its constructor needs a GPU for the predictor's parameters) """
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    from textocvp_amd.train.step import decoder_loss
    savi = _savi(tag)
    loss = decoder_loss(savi)
    assert isinstance(loss, GenericDecoderLoss)
    assert loss.dec is savi.decoder
    # chunking as inference: max_slot_images // K frames
    assert loss.chunk_frames(7) == max(1, savi.decoder.max_slot_images // 7)


def test_shipped_decoder_keeps_decoder_loss():
    from textocvp_amd.train.decoder import DecoderLoss
    from textocvp_amd.train.step import decoder_loss
    assert type(decoder_loss(setup_model(default_exp_params(num_slots=7)["model"]))) is DecoderLoss


def test_generic_decoder_loss_refuses_the_shipped_decoder():
    from textocvp_amd.train.decoder_generic import GenericDecoderLoss
    savi = setup_model(default_exp_params(num_slots=7)["model"])
    with pytest.raises(NotImplementedError, match="generic"):
        GenericDecoderLoss(savi)
